"""Parity tests proper: the hand-written gfx950 kernels, called through the C ABI, against the checker (oracle/_ref =
the unmodified reference header) and the WASM golden vectors.  Run on a real MI355X: pytest -m gpu."""
import numpy as np
import pytest

from conftest import package, rel_rms, synth_input
import geometry_cases as gc
import parity_cases as pc
import scenarios

pytestmark = pytest.mark.gpu

D48 = dict(preset="default", sample_rate=48000.0)


@pytest.mark.parametrize("name", scenarios.golden_names())
def test_golden(hip, ref, name):
    pc.case_golden(hip, ref, name)


def test_api_surface_small(hip, ref):
    pc.case_api_surface(hip, ref)


def test_api_surface_d48(hip, ref):
    """The same API walk at presetDefault @ 48 kHz (the fast FFT kernels and the staged record producers)."""
    pc.case_api_surface(hip, ref, cfg=D48, scale=12)


def test_split_mode(hip, ref):
    pc.case_split_mode(hip, ref)


def test_pitch_and_formants_small(hip, ref):
    pc.case_pitch_and_formants(hip, ref)


def test_pitch_and_formants_preset_default(hip, ref):
    pc.case_pitch_and_formants(hip, ref, cfg=D48, n=20000)


def test_large_plan_mapped(hip, ref):
    pc.case_large_plan_mapped(hip, ref)


def test_silence(hip, ref):
    pc.case_silence(hip, ref)


def test_channels(hip, ref):
    pc.case_channels(hip, ref, channel_counts=(1, 2, 3, 4, 5, 6, 7, 8))
    pc.case_channels(hip, ref, channel_counts=(9, 12, 16))  # beyond the fused kernels' eight channels: kPredictB + kChain, records through HBM


def test_batch_ragged(hip, ref):
    pc.case_batch_ragged(hip, ref)
    pc.case_batch_ragged(hip, ref, cfg=dict(preset="configure", block=5760, interval=1440, split=False), S=6, n=30000)


def test_random_time_factor(hip, ref):
    pc.case_random_time_factor(hip, ref)


def _batch_vs_ref(hip, ref, S, C, sr, n, nout, cfg, preset, label, setup=None, per_stream_setup=None, cap=pc.CAP_TONAL):
    """Run a batch on the GPU and every stream through the checker (plus the checker's self-sensitivity run)."""
    pkg = package()
    xs = np.stack([synth_input(s, C, n, sr) for s in range(S)])
    nouts = [nout]*S if np.isscalar(nout) else list(nout)
    b = pkg.StretchBatch(S, C, preset=preset, sample_rate=sr, lib=hip)
    if setup:
        setup(b)
    if per_stream_setup:
        for s in range(S):
            per_stream_setup(b, s, s)
    y = b.process(xs, nouts)
    b.close()
    informative = []
    for s in range(S):
        def one(o, s=s):
            if setup:
                setup(o)
            if per_stream_setup:
                per_stream_setup(o, s, None)
        r = pc.make("ref", hip, ref, C, cfg, one, seed=s)  # stream s of a batch = the instance seeded seed + s
        o = r.process(xs[s], nouts[s])
        o2 = [pc.make("ref", hip, ref, C, cfg, one, seed=s).process(pc.perturbed(xs[s], seed), nouts[s]) for seed in pc.SELF_SEEDS]
        informative.append(pc.assert_parity(y[s][:, :nouts[s]], o, o2, r.intervalSamples(), "%s stream %d" % (label, s), cap=cap, require_informative=False))
        # phase-free check that survives decorrelation (SURVEY App. D.2 iv): output energy within 1 %
        ra, rb = np.sqrt(np.mean(y[s][:, :nouts[s]]**2)), np.sqrt(np.mean(o**2))
        assert abs(ra/rb - 1) < 0.01, (label, s, ra, rb)
    # how far the sample-domain comparison really went, per stream (hops up to which a bound was ASSERTED; beyond that the checker's own
    # response to a 1e-6 perturbation exceeds the cap and only the phase-free instruments speak): reported, and bounded from below --
    # the sine streams (s % 3 == 0) must be informative over at least the first 12 hops, and no more than a third of the streams may
    # be chaos-dominated from the first horizon on (the noise streams through a frequency map are)
    _report("free_running_horizons/" + label.replace(" ", "_"), dict(hops_asserted=informative, streams=S))
    assert all(h >= 12 for s, h in enumerate(informative) if s % 3 == 0), (label, informative)
    assert sum(1 for h in informative if h == 0) <= S//3, (label, informative)


def test_config2_subset(hip, ref):
    """BASELINE config 2 (256 stereo streams, 48 kHz, presetDefault, 1.5x): parity subset = first 8 streams (all three
    signal types) at the benchmark's own length, 10 s = 500 hops per stream."""
    _batch_vs_ref(hip, ref, 8, 2, 48000, 480000, 720000, D48, "default", "config2")


def test_config3_subset(hip, ref):
    """config 3: +12 semitones with 8 kHz tonality limit, stretch 1.0; first 6 streams at the bench's own length (10 s)."""
    _batch_vs_ref(hip, ref, 6, 2, 48000, 480000, 480000, D48, "default", "config3",
                  setup=lambda o: o.setTransposeSemitones(12, 8000/48000))


def test_config4_subset(hip, ref):
    """config 4 literal (0.75x, formant compensation inert) and 4b (+4 st so the formant kernel runs)."""
    for semis in (0.0, 4.0):
        def setup(o, semis=semis):
            if semis:
                o.setTransposeSemitones(semis, 8000/48000)
            o.setFormantFactor(1, True)
            o.setFormantBase(200/48000)
        _batch_vs_ref(hip, ref, 6, 2, 48000, 480000, 360000, D48, "default", "config4 (+%g st)" % semis, setup=setup,  # 10 s, as the bench
                      cap=pc.CAP_FORMANT if semis else pc.CAP_TONAL)


def test_config5_subset(hip, ref):
    """config 5 flavour: 8-channel streams, 96 kHz, presetCheaper (split), per-stream random stretch and transpose; 2 s as the bench.
    Nine streams: three of every signal type (round 5 had four: horizons 24 / 12 / 0 / 24)."""
    S, n = 9, 192000
    g = np.random.Generator(np.random.PCG64(5))
    stretch = g.uniform(0.75, 1.5, S)
    semis = g.uniform(-12, 12, S)
    nout = [int(round(n*stretch[s])) for s in range(S)]

    def per_stream(o, s, index):
        if index is None:
            o.setTransposeSemitones(float(semis[s]), 0.0)
        else:
            o.setTransposeSemitones(float(semis[s]), 0.0, stream=index)
    _batch_vs_ref(hip, ref, S, 8, 96000, n, nout, dict(preset="cheaper", sample_rate=96000.0), "cheaper", "config5",
                  per_stream_setup=per_stream)


def test_full_batch_identity_and_determinism(hip):
    """Size-independent known answers at BASELINE config-2 scale (256 stereo streams, presetDefault @ 48 kHz):
    1.0x / 0 st reproduces every input delayed by inputLatency+outputLatency; the same call twice is bit-identical;
    hop-aligned chunking is bit-identical to one call; a stream inside a batch equals the same stream run alone."""
    import torch
    pkg = package()
    S, C, sr, n = 256, 2, 48000, 48000
    dev = torch.device("cuda:0")
    gen = torch.Generator(device="cpu").manual_seed(7)
    base = torch.from_numpy(np.stack([synth_input(s, C, n, sr) for s in range(12)]))
    x = base.repeat(22, 1, 1)[:S].contiguous()
    x = (x*(0.5 + 0.5*torch.rand(S, 1, 1, generator=gen))).to(dev)
    b = pkg.StretchBatch(S, C, preset="default", sample_rate=sr, lib=hip)
    lag = b.inputLatency() + b.outputLatency()
    y = b.process(x, n)
    b.synchronize()
    err = torch.sqrt(((y[:, :, lag:] - x[:, :, :-lag])**2).mean(dim=(1, 2))/(x[:, :, :-lag]**2).mean(dim=(1, 2)))
    assert float(err.max()) < 4e-6, float(err.max())  # measured 1.6e-6 worst stream (6-pass fp32 FFT round trip)
    # determinism
    b.reset()
    y2 = b.process(x, n)
    b.synchronize()
    assert torch.equal(y, y2)
    # chunking invariance (hop-aligned chunks), 1.25x so the phase vocoder is active
    b.reset()
    whole = b.process(x[:, :, :28800], 36000)
    b.synchronize()
    b.reset()
    parts = []
    for k in range(5):
        parts.append(b.process(x[:, :, 5760*k:5760*(k + 1)].contiguous(), 7200))
    b.synchronize()
    chunked = torch.cat(parts, dim=2)
    # bit-identical: the library is built with -ffp-contract=on, so a (hop, bin) cell rounds the same way whichever
    # code path produces it (with the default contraction the first hop after a chunk boundary differed by 1 ulp, which the
    # recurrence amplified to 2e-4 over these 25 hops -- tools/diag/diag_stage.py)
    assert torch.equal(whole, chunked), float((whole - chunked).abs().max())
    b.close()
    # batch == single
    one = pkg.StretchBatch(1, C, preset="default", sample_rate=sr, lib=hip)
    for s in (0, 77, 255):
        one.reset()
        ys = one.process(x[s:s + 1, :, :28800].contiguous(), 36000)
        one.synchronize()
        assert torch.equal(ys[0], whole[s]), s
    one.close()


def test_host_and_device_memory_agree(hip):
    import torch
    pkg = package()
    S, C, sr, n = 3, 2, 48000, 20000
    xs = np.stack([synth_input(s, C, n, sr) for s in range(S)])
    b = pkg.StretchBatch(S, C, preset="default", sample_rate=sr, lib=hip)
    yh = b.process(xs, 25000)
    b.reset()
    yd = b.process(torch.from_numpy(xs).cuda(), 25000)
    b.synchronize()
    assert np.array_equal(yh, yd.cpu().numpy())
    b.close()


def test_sub_batches(hip, ref, monkeypatch):
    pc.case_sub_batches(hip, ref, monkeypatch)


def test_cmd_main_flow_config1(hip, ref):
    """BASELINE config 1 (1 mono stream, 44.1 kHz, presetDefault, 1.0x / 0 st via the cmd/main.cpp call sequence)."""
    pc.case_cmd_main_flow(hip, ref)
    pc.case_cmd_main_flow(hip, ref, sr=48000, seconds=2.0, time_factor=1.3, semitones=3.0, channels=2)


@pytest.mark.gpu
@pytest.mark.parametrize("preset,C", [("default", 2), ("default", 1), ("cheaper", 2)])
def test_staged_producers_equal_gathered(hip, monkeypatch, preset, C):
    """The fused recurrence kernel has three record producers: whole lines in LDS with a wavefront lag of 8 bins (plain tiles of the
    L = 4 geometries by default; SMST_ALIGN_ALL=1 wherever valid, as here for presetCheaper's L = 3), per-row windows staged in LDS
    with lag L+1 (SMST_NO_ALIGN=1; the only staged form for L = 5) and direct gathers (SMST_NO_STAGE=1).  Same arithmetic, so the
    outputs must be bit-identical -- over two calls, so that the carried state is exercised; the launch counters prove that each
    form really ran.  (The aligned form waits for its loads by count, smst_async.h: this is its correctness test on hardware.)"""
    import torch
    pkg = package()
    S, sr = 8, 48000
    x = torch.from_numpy(np.stack([synth_input(s, C, 24000, sr) for s in range(S)])).cuda()
    outs = []
    monkeypatch.setenv("SMST_ALIGN_ALL", "1")
    for env, counter in ((None, "vocoder_aligned"), ("SMST_NO_ALIGN", "vocoder_staged"), ("SMST_NO_STAGE", "vocoder_gather")):
        if env:
            monkeypatch.setenv(env, "1")
        before = pkg.launch_count(counter, hip)
        b = pkg.StretchBatch(S, C, preset=preset, sample_rate=sr, lib=hip)
        y1 = b.process(x[:, :, :9000].contiguous(), 11000)
        y2 = b.process(x[:, :, 9000:].contiguous(), 21000)
        b.synchronize()
        outs.append(torch.cat([y1, y2], dim=2).clone())
        b.close()
        assert pkg.launch_count(counter, hip) > before, counter
    assert torch.equal(outs[0], outs[1]), float((outs[0] - outs[1]).abs().max())
    assert torch.equal(outs[1], outs[2]), float((outs[1] - outs[2]).abs().max())


@pytest.mark.gpu
def test_realtime_quanta(hip, ref):
    pc.case_realtime_quanta(hip, ref)
    pc.case_realtime_quanta(hip, ref, cfg=D48, quanta=120)  # 10.7 hops: past the 5760-sample latency, where there is output to compare


@pytest.mark.gpu
def test_feed_scan_close_to_serial(hip, monkeypatch):
    """The feed recurrences (smoothing, peaks, map, formant envelope) run in scan form; SMST_FEED_SERIAL=1 evaluates them
    bin by bin in the reference's order.  Only the carries entering a chunk round differently: the outputs agree to the
    level a 1e-6 input perturbation moves them (measured 5e-8 .. 4e-6 relative RMS on 0.5 s)."""
    pc.case_feed_scan_close_to_serial(hip, monkeypatch, D48, 6, 24000, 2e-4,
                                      setup=lambda b: (b.setTransposeSemitones(4, 8000/48000), b.setFormantFactor(1.2, True)))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(pc.FEED_SCAN_SHAPES))
def test_feed_scan_close_to_serial_shapes(hip, monkeypatch, shape):
    """The same at the smallest shapes that reach each form of the feed kernels (threads without a bin, one bin per thread, the
    <24> instantiations, the LDS form with the bisection): pitch map, formants with an estimated and with a given base."""
    geometry, n, bound = pc.feed_scan_shape(shape)
    pc.case_feed_scan_close_to_serial(hip, monkeypatch, geometry, 3, n, bound)


@pytest.mark.gpu
def test_mapped_path_chunking_and_determinism(hip):
    """Pitch map + formants (scan-form feed, gathering record producers): the same call twice is bit-identical, and
    hop-aligned chunks are bit-identical to one call, as on the plain path."""
    import torch
    pkg = package()
    S, C, sr = 8, 2, 48000
    x = torch.from_numpy(np.stack([synth_input(s, C, 28800, sr) for s in range(S)])).cuda()

    def make():
        b = pkg.StretchBatch(S, C, preset="default", sample_rate=sr, lib=hip)
        b.setTransposeSemitones(5, 8000/48000)
        b.setFormantFactor(0.9, True)
        b.setFormantBase(150/48000)
        return b
    b = make()
    whole = b.process(x, 36000)
    b.synchronize()  # results are ordered on the batch's own stream, not on torch's
    whole = whole.clone()
    b.reset()
    again = b.process(x, 36000)
    b.synchronize()
    again = again.clone()
    b.reset()
    parts = [b.process(x[:, :, 5760*k:5760*(k + 1)].contiguous(), 7200) for k in range(5)]
    b.synchronize()
    chunked = torch.cat(parts, dim=2)
    b.close()
    assert float(whole.abs().max()) > 0.05
    assert torch.equal(whole, again)
    assert torch.equal(whole, chunked), float((whole - chunked).abs().max())


@pytest.mark.gpu
def test_eight_channel_identity_at_scale(hip):
    """BASELINE config-5 geometry (8 channels, 96 kHz, presetCheaper, split computation) through the un-fused recurrence
    (kPredictB + kChain): 1.0x / 0 st reproduces every input delayed by inputLatency + outputLatency."""
    import torch
    pkg = package()
    S, C, sr, n = 48, 8, 96000, 96000
    x = torch.from_numpy(np.stack([synth_input(s, C, n, sr) for s in range(12)])).repeat(4, 1, 1)[:S].contiguous().cuda()
    b = pkg.StretchBatch(S, C, preset="cheaper", sample_rate=sr, lib=hip)
    lag = b.inputLatency() + b.outputLatency()
    y = b.process(x, n)
    b.synchronize()
    b.close()
    err = torch.sqrt(((y[:, :, lag:] - x[:, :, :-lag])**2).mean(dim=(1, 2))/(x[:, :, :-lag]**2).mean(dim=(1, 2)))
    assert float(err.max()) < 4e-6, float(err.max())


def _inputs_cuda(S, C, n, sr):
    import torch
    base = torch.from_numpy(np.stack([synth_input(s, C, n, sr) for s in range(12)]))
    return base.repeat((S + 11)//12, 1, 1)[:S].contiguous().cuda()


@pytest.mark.gpu
def test_full_size_config3_and_4(hip):
    """BASELINE configs 3 and 4b at their full per-GPU stream counts (1024 resp. 512 stereo streams; 2 s instead of 10 s):
    size-independent properties on the mapped path -- every output finite and of input-like level, the same call twice
    bit-identical, and streams inside the big batch bit-identical to the same streams in a batch of their own."""
    import torch
    pkg = package()
    sr, C, n = 48000, 2, 96000

    def cfg3(b):
        b.setTransposeSemitones(12, 8000/48000)

    def cfg4b(b):
        b.setTransposeSemitones(4, 8000/48000)
        b.setFormantFactor(1, True)
        b.setFormantBase(200/48000)
    for S, stretch, setup in ((1024, 1.0, cfg3), (512, 0.75, cfg4b)):
        x = _inputs_cuda(S, C, n, sr)
        n_out = int(n*stretch)
        b = pkg.StretchBatch(S, C, preset="default", sample_rate=sr, lib=hip)
        setup(b)
        y = b.process(x, n_out)
        b.synchronize()
        y = y.clone()
        b.reset()
        y2 = b.process(x, n_out)
        b.synchronize()
        assert torch.equal(y, y2)
        b.close()
        assert bool(torch.isfinite(y).all())
        rms_in, rms_out = x.pow(2).mean(dim=(1, 2)).sqrt(), y[:, :, n_out//4:].pow(2).mean(dim=(1, 2)).sqrt()
        ratio = rms_out/rms_in
        # (the chirp streams lose most of their energy above the fold when shifted up an octave: 0.09)
        assert 0.02 < float(ratio.min()) and float(ratio.max()) < 3.0, (float(ratio.min()), float(ratio.max()))
        picks = [0, S//2 + 1, S - 1]
        small = pkg.StretchBatch(len(picks), C, preset="default", sample_rate=sr, lib=hip)
        setup(small)
        ys = small.process(x[picks].contiguous(), n_out)
        small.synchronize()
        assert torch.equal(ys, y[picks])
        small.close()


@pytest.mark.gpu
def test_full_size_config5_identity(hip):
    """BASELINE config 5 at its full per-GPU size (1024 streams x 8 channels, 96 kHz, presetCheaper / split, 2 s):
    1.0x / 0 st is the identity with the documented delay."""
    import torch
    pkg = package()
    S, C, sr, n = 1024, 8, 96000, 192000
    x = _inputs_cuda(S, C, n, sr)
    b = pkg.StretchBatch(S, C, preset="cheaper", sample_rate=sr, lib=hip)
    lag = b.inputLatency() + b.outputLatency()
    y = b.process(x, n)
    b.synchronize()
    b.close()
    err = torch.sqrt(((y[:, :, lag:] - x[:, :, :-lag])**2).mean(dim=(1, 2))/(x[:, :, :-lag]**2).mean(dim=(1, 2)))
    assert float(err.max()) < 4e-6, float(err.max())


# ---- chaos-free instruments (SURVEY App. D.2 i, iv, v) -------------------------------------------------------------
CHEAPER96 = dict(preset="cheaper", sample_rate=96000.0)


def _cfg3(o):
    o.setTransposeSemitones(12, 8000/48000)


def _cfg4b(o):
    o.setTransposeSemitones(4, 8000/48000)
    o.setFormantFactor(1, True)
    o.setFormantBase(200/48000)


def _report(name, figures):
    """One line per measurement into gpurun_out/ (copied to profiles/ as evidence)."""
    import json
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    os.makedirs(os.path.join(root, "gpurun_out"), exist_ok=True)
    with open(os.path.join(root, "gpurun_out", "parity_instruments.jsonl"), "a") as f:
        def plain(v):
            if isinstance(v, (list, tuple)):
                return [plain(u) for u in v]
            try:
                return float(v)
            except (TypeError, ValueError):
                return str(v)
        f.write(json.dumps(dict(test=name, **{str(k): plain(v) for k, v in figures.items()})) + "\n")


@pytest.mark.parametrize("gain_offsets", [False, True], ids=["equal-gains", "gain-offsets"])
@pytest.mark.parametrize("label,cfg,C,stretch,setup", [
    ("config2", D48, 2, 1.5, None),
    ("config3", D48, 2, 1.0, _cfg3),
    ("config4b", D48, 2, 0.75, _cfg4b),
    ("config5-8ch-cheaper", CHEAPER96, 8, 1.2, lambda o: o.setTransposeSemitones(-5, 0)),
])
def test_teacher_forced(hip, ref, label, cfg, C, stretch, setup, gain_offsets):
    """D.2 (i): product state := checker state, one hop, Band.output and the emitted interval; for the sine / chirp / noise streams of
    the bench (0, 1, 2).  Every hop is bounded (parity_cases.case_teacher_forced): a FIXED ceiling on Band.output outside the
    arg-max near-tie regions (per bin, decided from the checker's data), 1e-4 on |Band.output| inside them, the smooth
    5 x self-sensitivity bound on the hops without any discrete event.  Twice: with the bench's equal-amplitude channels (near-ties
    endemic) and with channel gains 1 - 0.07 c, where at most one hop in ten may have an excused bin at all.  Also the committed
    measurement behind PERTURBATION: the analysis spectra of the two implementations differ by `analysis` rel-RMS, which an input
    perturbation of sqrt(3)*analysis would produce."""
    formant = label == "config4b"
    cap = pc.CAP_FORMANT if formant else pc.CAP_TONAL
    w = pc.case_teacher_forced(hip, ref, cfg, C, stretch, "forced " + label, setup=setup, warm_hops=10, forced_hops=8, cap=cap, trim=0.01 if formant else 0.0,
                               gains=[1 - 0.07*c for c in range(C)] if gain_offsets else None, cap_well_conditioned=pc.CAP_TONAL)
    w["equivalent_perturbation"] = 3**0.5*w["analysis"]
    _report("teacher_forced/" + label + ("/gain-offsets" if gain_offsets else ""), w)
    assert w["spectrum_outside_ties"] <= cap and w["magnitude_inside_ties"] <= pc.TOL_EXCUSED_MAGNITUDE, w  # (asserted per hop inside the case as well)
    # Round 6: the two legs that assert something whatever the scenario's conditioning.  (i) Band.output over the bins the CHECKER itself holds to
    # 1e-3 under an input perturbation of 1e-6, wherever they carry a quarter of the hop's energy: within 5e-3 on every such hop (asserted inside
    # the case; with formant processing that is 16-17 of 24 hops, measured 4.5e-3 / 4.1e-4 -- the whole-spectrum figure there is dominated by
    # near-silent bins that the envelope ratio scales up and whose PHASE the checker does not hold to 1e-1, which is why its ceiling is 5e-2).
    # (ii) |Band.output| over EVERY bin -- the formant ratio, the map and the energy interpolation without the phase: within 2e-4 or five times
    # the checker's own (measured 2e-7 config 2, 5e-5 config 3, 4e-5 config 4b against the checker's own 1.2e-4, 9e-5 config 5).
    assert w.get("well_conditioned_hops", 0) >= w["hops"]//2, w
    assert w["magnitude_all_bins"] <= max(2e-4, pc.SELF_FACTOR*w["magnitude_all_bins_self"]), w
    if gain_offsets:
        # near-ties are rare once the channels differ in level: less than 1 % of the spectra's energy lies in an excused region (most excused bins
        # are at the noise floor), and -- for the stereo configurations -- at most one hop in ten has a region that carries energy at all.
        # (8 channels of independent noise keep two to three near-tie bins per hop whatever the gains: half of that stream's hops, none of
        # the sine and chirp streams')
        assert w["excused_energy_fraction"] <= 0.01, w
        assert w["excused_hops"] <= (0.1 if C == 2 else 0.25)*w["hops"], w
        assert w["clean_hops"] >= (0.75 if C == 2 else 0.5)*w["hops"], w  # the sample-domain legs really cover most hops
    assert w["equivalent_perturbation"] <= pc.PERTURBATION, w
    assert w["equivalent_perturbation"] >= pc.PERTURBATION/8, w  # ... and PERTURBATION is not much larger than it needs to be


def test_hop_magnitudes_noise_full_length(hip, ref):
    """D.2 (iv) on the noise streams of config 2 over the bench's full 10 s (500 hops): the sample-domain comparison is
    meaningless there after ~100 hops, |output_c[b]| per hop is not."""
    r = pc.case_hop_magnitudes(hip, ref, D48, 2, 1.5, "magnitudes config2 noise", hops=500, streams=(2, 5))
    _report("hop_magnitudes/config2-noise-10s", r)


def test_hop_magnitudes_config2_subset_full_length(hip, ref):
    """The same instrument on ALL eight streams of the config-2 parity subset (sine, chirp and noise, streams 0..7) over the
    bench's full 10 s: every hop's |output_c[b]| within 1e-4 of the checker's."""
    r = pc.case_hop_magnitudes(hip, ref, D48, 2, 1.5, "magnitudes config2 subset", hops=500, streams=tuple(range(8)))
    _report("hop_magnitudes/config2-subset-8x10s", r)


def test_hop_decisions_full_length(hip, ref):
    """Configs 3 and 4b at the bench's own length (10 s: 333 and 250 hops) on six streams each (two of every signal type):
    per-hop magnitudes, arg-max channel and output map."""
    # tolerance 2e-4 (1e-4 on the plain path): with a frequency map |output|^2 is an interpolation of the input energies at
    # map.inputBin, whose fp32 resolution near the top of the spectrum is 2.4e-4 bins; the chirp streams end there (19 kHz after
    # 10 s), and one ulp of inputBin moves the interpolated energy of their peak bins by more than 1e-4 (measured worst hop:
    # 1.07e-4, chirp stream, hop 322 of 333, maps agreeing within 2e-3 bins everywhere)
    r = pc.case_hop_magnitudes(hip, ref, D48, 2, 1.0, "decisions config3 full", setup=_cfg3, hops=333, streams=tuple(range(6)), tol=2e-4)
    _report("hop_decisions/config3-6x10s", r)
    r = pc.case_hop_magnitudes(hip, ref, D48, 2, 0.75, "decisions config4b full", setup=_cfg4b, hops=250, streams=tuple(range(6)), tol=2e-4)
    _report("hop_decisions/config4b-6x10s", r)


def test_random_time_factor_seeds(hip, ref):
    """> 2x stretch at presetDefault / 48 kHz on eight streams: level within 2 % of the checker, same-seed determinism across
    instances and across batch / single-stream objects."""
    r = pc.case_random_time_factor_seeds(hip, ref, streams=8, stretch=2.5, seconds=1.5)
    _report("random_time_factor/d48-8streams-2.5x", r)


def test_hop_decisions(hip, ref):
    """D.2 (v): arg-max channel (stretch.h:729-737) and output map / peak list (:859-917) agreement, per hop, on the
    mapped configs (sine, chirp and noise streams)."""
    r = pc.case_hop_magnitudes(hip, ref, D48, 2, 1.0, "decisions config3", setup=_cfg3, hops=80, streams=(0, 1, 2))
    _report("hop_decisions/config3", r)
    r = pc.case_hop_magnitudes(hip, ref, D48, 2, 0.75, "decisions config4b", setup=_cfg4b, hops=80, streams=(0, 1, 2))
    _report("hop_decisions/config4b", r)
    r = pc.case_hop_magnitudes(hip, ref, CHEAPER96, 8, 1.2, "decisions 8ch", setup=lambda o: o.setTransposeSemitones(-5, 0), hops=40, streams=(0, 2))
    _report("hop_decisions/config5-8ch", r)


def test_hop_decisions_config5_as_named(hip, ref):
    """BASELINE config 5 as it names itself: 8-channel streams at 96 kHz, presetCheaper (split computation), PER-STREAM random stretch
    0.75-1.5x and +-12 st drawn as bench.py --config 5 draws them (PCG64(5)), six streams (two of every signal type) x 2 s: per-hop
    |output|, arg-max channel and output map, free running."""
    g = np.random.Generator(np.random.PCG64(5))
    stretches, semis = g.uniform(0.75, 1.5, 8192)[:6], g.uniform(-12, 12, 8192)[:6]
    hops = int(2.0*96000*float(stretches.min())/3840)  # 2 s of input at the smallest stretch factor (interval 3840)
    r = pc.case_hop_magnitudes(hip, ref, CHEAPER96, 8, stretches, "decisions config5 as named", hops=hops, streams=tuple(range(6)), tol=2e-4, semitones=semis)
    _report("hop_decisions/config5-as-named-6x2s", r)


def test_process_does_not_allocate_in_steady_state_gpu(hip):
    from test_abi import _steady_state_allocations
    _steady_state_allocations(hip, dict(preset="default", sample_rate=48000.0), S=16, C=2, calls=4)


def test_feed_fusion_equals_separate(hip, monkeypatch):
    pc.case_feed_fusion_equals_separate(hip, monkeypatch, channel_counts=(1, 2, 3, 8))
    pc.case_feed_fusion_equals_separate(hip, monkeypatch, channel_counts=(2,), geometry=dict(preset="default", sample_rate=48000.0), n=40000)
    pc.case_feed_fusion_equals_separate(hip, monkeypatch, channel_counts=(1, 2, 8), formants=True)
    pc.case_feed_fusion_equals_separate(hip, monkeypatch, channel_counts=(2,), geometry=dict(preset="default", sample_rate=48000.0), n=40000, formants=True)
    pc.case_feed_fusion_equals_separate(hip, monkeypatch, channel_counts=(1, 2, 8), formants=True, bases_given=True)  # every base frequency given: the feed stage is ONE kernel
    pc.case_feed_fusion_equals_separate(hip, monkeypatch, channel_counts=(2,), geometry=dict(preset="default", sample_rate=48000.0), n=40000, formants=True, bases_given=True)
    # 20 bins per thread (kFeedScanA<24, true>, <24, false, true>, kFeedScanC<24, true>; every 96 kHz preset), three intervals
    g24 = dict(block=10240, interval=2560, split=False)
    pc.case_feed_fusion_equals_separate(hip, monkeypatch, channel_counts=(2,), geometry=g24, n=3*2560 + 2560)
    pc.case_feed_fusion_equals_separate(hip, monkeypatch, channel_counts=(2,), geometry=g24, n=3*2560 + 2560, formants=True)
    pc.case_feed_fusion_equals_separate(hip, monkeypatch, channel_counts=(2,), geometry=g24, n=3*2560 + 2560, formants=True, bases_given=True)
    # 32 bins per thread: the LDS forms have no one-pass variant (the case asserts that the counter does not grow)
    pc.case_feed_fusion_equals_separate(hip, monkeypatch, channel_counts=(2,), geometry=dict(block=15360, interval=3840, split=False), n=3*3840 + 3840, formants=True,
                                        bases_given=True, one_pass=False)


def test_gather_pass_shapes(hip, monkeypatch):
    """mono / stereo tiles with a frequency map: the gathering producers' two pass shapes give the same records."""
    # (vertical steps 4 and 5, then 2 and 3; the presets' own geometries last)
    pc.case_gather_pass_shapes(hip, monkeypatch, extra_geometries=(dict(block=512, interval=256, split=False), dict(block=512, interval=170, split=False),
                                                                  dict(preset="default", sample_rate=48000.0), dict(preset="cheaper", sample_rate=48000.0)), n=30000)


def test_vocn_writer_forms(hip, monkeypatch):
    """3-8 channels: the writer wave's whole lines / half lines / sectors are the same values."""
    pc.case_vocn_writer_forms(hip, monkeypatch, channel_counts=(3, 4, 5, 6, 7, 8), n=30000,
                              extra_geometries=(dict(block=512, interval=256, split=False), dict(block=512, interval=170, split=False), dict(preset="cheaper", sample_rate=96000.0)))


def test_fused_equals_unfused(hip, monkeypatch):
    """3-8 channels: kVocoderN (records in LDS) is bit-identical to kPredictB + kChain (records through HBM)."""
    pc.case_fused_equals_unfused(hip, monkeypatch, channel_counts=(1, 2, 3, 4, 5, 6, 7, 8))
    pc.case_fused_equals_unfused(hip, monkeypatch, channel_counts=(8,), geometry=dict(preset="cheaper", sample_rate=96000.0), n=96000)


def test_single_hop_chunks(hip):
    """kVocoderOne (single-hop tiles, the real-time pattern) is bit-identical to the skewed-wavefront kernels."""
    pc.case_single_hop_chunks(hip, channel_counts=(1, 2, 3, 8))
    pc.case_single_hop_chunks(hip, geometry=dict(preset="default", sample_rate=48000.0), channel_counts=(2,), hops=10)
    pc.case_single_hop_chunks(hip, geometry=dict(preset="default", sample_rate=48000.0), channel_counts=(2,), hops=10,
                              setup=lambda b: (b.setTransposeSemitones(4, 8000/48000), b.setFormantFactor(1, True), b.setFormantBase(200/48000)))
    pc.case_single_hop_chunks(hip, geometry=dict(preset="cheaper", sample_rate=96000.0), channel_counts=(8,), hops=5)


def test_half_state(hip, ref):
    """BASELINE config 5 "fp16 internal": carried state in fp16 against the fp32 checker, magnitude domain."""
    r = pc.case_half_state(hip, ref, D48, 2, 1.5, "half config2")
    _report("half_state/config2", r)
    r = pc.case_half_state(hip, ref, CHEAPER96, 8, 1.2, "half config5-8ch", setup=lambda o: o.setTransposeSemitones(-5, 0), hops=20, streams=(0, 2))
    _report("half_state/config5-8ch", r)
    # the bulk path (64 hops per tile: the state is narrowed once per tile) against the fp32 product itself
    import torch
    pkg = package()
    S, C, sr, n = 8, 8, 96000, 192000
    x = torch.from_numpy(np.stack([synth_input(s, C, n, sr) for s in range(S)])).cuda()
    outs = []
    for half in (False, True):
        b = pkg.StretchBatch(S, C, preset="cheaper", sample_rate=sr, lib=hip, half_state=half)
        b.setTransposeSemitones(3.0, 0.0)
        y = b.process(x, int(n*1.2))
        b.synchronize()
        outs.append(y.clone())
        b.close()
    lvl = float((outs[1].pow(2).mean().sqrt()/outs[0].pow(2).mean().sqrt() - 1).abs())
    assert lvl < 0.01, lvl
    assert bool(torch.isfinite(outs[1]).all())


def test_stream_ordering_without_host_sync(hip):
    """smst_batch_wait_for_stream / _signal_stream (the Python wrapper's `ordered=True`): the input is produced by a torch kernel
    on a side stream that is still running when process() is called, and the output is consumed by torch right after the
    call -- no host synchronisation anywhere; the result must equal the fully synchronised run."""
    import torch
    pkg = package()
    S, C, sr, n = 4, 2, 48000, 48000
    base = torch.from_numpy(np.stack([synth_input(s, C, n, sr) for s in range(S)])).cuda()
    b = pkg.StretchBatch(S, C, preset="default", sample_rate=sr, lib=hip)
    ref_out = b.process(base, 60000).clone()
    b.synchronize()
    side = torch.cuda.Stream()
    for trial in range(3):
        b.reset()
        big = torch.randn(4096, 4096, device="cuda")
        with torch.cuda.stream(side):
            for _ in range(4):
                big = big @ big*1e-4           # keeps the side stream busy for a while
            x = base*2.0                       # the producer of the input, behind that work
            x = x*0.5
            y = b.process(x, 60000)            # ordered after `side`'s current work by an event
            total = (y - ref_out).abs().max()  # consumer on the same torch stream, ordered after the batch's kernels
        assert float(total) == 0.0, (trial, float(total))
    b.close()


def test_packed_complex_helpers(hip):
    """csrc/smst_complex.h is inline assembly (v_pk_mul_f32 / v_pk_fma_f32 with op_sel / neg modifiers): operand selects,
    negations and the documented roundings, bit for bit, on the device."""
    pc.case_complex_helpers(hip)


def test_fast_fft_every_preset_geometry(hip, monkeypatch):
    """kAnalyseFast / kSynthFast<R3> for R3 = 10, 12, 20, 24 against the generic FFT ladder and the identity."""
    print(pc.case_fast_fft_close_to_generic(hip, monkeypatch))


def test_clone(hip):
    pc.case_clone(hip)


def test_map_table_lengths(hip):
    pc.case_map_table_lengths(hip)


def test_debug_map_is_of_the_last_call(hip):
    pc.case_debug_map_is_of_the_last_call(hip)


def test_split_mid_interval_flush(hip, ref):
    _report("split_mid_interval_flush", pc.case_split_mid_interval_flush(hip, ref))


@pytest.mark.parametrize("variant", ["L6", "L7", "L8", "L6_3ch", "no_single_hop", "no_single_hop_3ch"])
def test_split_mid_interval_flush_wide(hip, ref, monkeypatch, variant):
    """HopDesc.startBin in every recurrence form, not only kVocoderOne"""
    _report("split_mid_interval_flush_wide/" + variant, _split_flush_wide(hip, ref, monkeypatch, variant))


def _split_flush_wide(lib, ref, monkeypatch, variant):
    if variant.startswith("no_single_hop"):
        monkeypatch.setenv("SMST_NO_SINGLE_HOP", "1")
        return pc.case_split_mid_interval_flush_wide(lib, ref, channels=3 if variant.endswith("3ch") else 2, block=512)
    block = {"L6": 768, "L7": 896, "L8": 1024}[variant[:2]]
    return pc.case_split_mid_interval_flush_wide(lib, ref, channels=3 if variant.endswith("3ch") else 2, block=block)


@pytest.mark.parametrize("geometry", scenarios.split_event_geometries())
def test_split_events_golden(hip, ref, geometry):
    """the reference's shipped WASM build on flush / parameter change / reset / seek between interval boundaries (split computation)"""
    _report("split_events_golden/" + geometry, pc.case_split_events_golden(hip, ref, geometry))


def test_split_events_vs_checker(hip, ref):
    _report("split_events_vs_checker", pc.case_split_events_vs_checker(hip, ref))
    _report("split_events_vs_checker/cheaper48k", pc.case_split_events_vs_checker(hip, ref, channels=2, cfg=dict(preset="cheaper", sample_rate=48000.0)))


def test_carried_emit_equals_copy(hip, monkeypatch):
    pc.case_carried_emit_equals_copy(hip, monkeypatch, streams=37)
    pc.case_carried_emit_equals_copy(hip, monkeypatch, streams=5, splits=(True,), half_state=True)


def test_across_equals_single_hop(hip, monkeypatch):
    pc.case_across_equals_single_hop(hip, monkeypatch, streams=300)
    pc.case_across_equals_single_hop(hip, monkeypatch, streams=5, channel_counts=(2,), setup=lambda b: b.setTransposeSemitones(5, 0.2))


def test_random_call_sequences(hip, ref):
    """API fuzz against the checker: seeded random walks over process / parameter setters / seek / flush / reset."""
    pc.case_random_call_sequences(hip, ref, seeds=range(12))
    # split computation: the same walks -- parameter changes, flushes, seeks and resets between interval boundaries included (round 5)
    _report("random_call_sequences_split", pc.case_random_call_sequences(hip, ref, seeds=range(100, 112), cfg=pc.SMALL_SPLIT))


def test_random_time_factor_parity(hip, ref):
    """Stretch beyond 2x, output without input, long flushes: the product replicates the checker's std::default_random_engine, so
    samples are compared, not just levels."""
    r = pc.case_random_time_factor_parity(hip, ref, geometries=(pc.SMALL, dict(preset="default", sample_rate=48000.0)), seeds=(0, 12345))
    _report("random_time_factor_parity", {k.replace("/", "_"): (v if isinstance(v, float) else v.get("spectrum")) for k, v in r.items()})


def test_reconfigure_keeps_random_engine(hip, ref):
    pc.case_reconfigure_keeps_random_engine(hip, ref)


def test_synth_emit_equals_two_kernels(hip, monkeypatch):
    """kSynthEmitTeams against kSynthTeams + kEmit: output and carry bit-identical."""
    pc.case_synth_emit_equals_two_kernels(hip, monkeypatch, presets=(("cheaper", 48000), ("default", 48000), ("default", 44100), ("cheaper", 44100)), streams=5)
    pc.case_synth_emit_equals_two_kernels(hip, monkeypatch, presets=(("default", 48000),), streams=3, channels=1)
    pc.case_synth_emit_equals_two_kernels(hip, monkeypatch, presets=(("default", 48000),), streams=2, channels=2, splits=(False,), half_state=True)
    pc.case_synth_emit_equals_two_kernels(hip, monkeypatch, presets=(("cheaper", 48000),), streams=3, channels=5, splits=(True,))


def test_oracle_parity_through_one_kernel_synthesis(hip, ref, monkeypatch):
    """The oracle-parity cases that the launcher's thresholds would route through kSynthTeams + kEmit (few streams), forced through
    kSynthEmitTeams: the API walk at presetDefault @ 48 kHz (process / flush / reset / seek / parameter changes between calls: every
    way the carry is handed over) and the first streams of config 2 at the benchmark's own length."""
    pkg = pc.package()
    monkeypatch.setenv("SMST_FFT_TEAMS", "2")
    monkeypatch.setenv("SMST_SYNTH_EMIT", "2")
    before = pkg.launch_count("synth_emit", hip)
    pc.case_api_surface(hip, ref, cfg=D48, scale=12)
    _batch_vs_ref(hip, ref, 4, 2, 48000, 480000, 720000, D48, "default", "config2-one-kernel")
    assert pkg.launch_count("synth_emit", hip) > before


def test_fft_teams_equals_per_frame(hip, monkeypatch):
    """kAnalyseTeams (SMST_FFT_TEAMS=1) against kAnalyseFast: bit-identical."""
    pc.case_fft_teams_equals_per_frame(hip, monkeypatch, presets=(("cheaper", 48000), ("default", 48000), ("default", 44100)), streams=5)
    pc.case_fft_teams_equals_per_frame(hip, monkeypatch, presets=(("default", 48000),), streams=2, channels=1)


def test_split_batch_events(hip, monkeypatch):
    """split computation in a batch: streams at different offsets of their intervals, per-stream setters and flushes == every stream alone"""
    pc.case_split_batch_events(hip, monkeypatch)


def test_split_dropped_block_random_engine(hip, ref):
    print(pc.case_split_dropped_block_random_engine(hip, ref))


def test_api_surface_and_realtime_quanta_split(hip, ref):
    """seek / ragged chunks / flush / outputSeek / exact and the AudioWorklet calling patterns in split-computation mode"""
    pc.case_api_surface(hip, ref, cfg=pc.SMALL_SPLIT)
    pc.case_realtime_quanta(hip, ref, cfg=pc.SMALL_SPLIT)


def test_split_freq_map_mid_interval(hip, ref):
    """ADVICE round 5 / review item 8: the frequency-map TABLE is latched with the step that read it"""
    _report("split_freq_map_mid_interval", pc.case_split_freq_map_mid_interval(hip, ref))


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["small", "default48", "default96_mono", "pattern_NCC", "pattern_NCCN", "pattern_NNNCC"])
def test_continuous_equals_tiled(hip, monkeypatch, variant):
    """kVocoderCont (one wavefront through the tiles of a call) against kVocoder tile by tile: bit-identical outputs and carried state;
    the launch counters prove which ran.  On the device this is also the test of the kernel's own load tracking (smst_async.h) and of
    row 0 reading back, through memory, what the same workgroup's writer wave stored a few hundred blocks earlier."""
    if variant.startswith("pattern_"):  # the tile patterns that reach the end-of-segment joins (tests/test_stream_order_emu.py)
        _report("continuous_equals_tiled/" + variant, pc.case_continuous_equals_tiled(hip, monkeypatch, channel_counts=(1, 2), pattern=variant[8:]))
    elif variant == "small":
        _report("continuous_equals_tiled/small", pc.case_continuous_equals_tiled(hip, monkeypatch))
    elif variant == "default48":
        _report("continuous_equals_tiled/default48", pc.case_continuous_equals_tiled(hip, monkeypatch, geometry=dict(preset="default", interval=1440), channel_counts=(2,), streams=9))
    else:
        monkeypatch.setenv("SMST_ALIGN_ALL", "1")
        _report("continuous_equals_tiled/default96_mono", pc.case_continuous_equals_tiled(hip, monkeypatch, geometry=dict(preset="default", interval=2880, sr=96000), channel_counts=(1,), ratios=(1.5,)))


def test_formant_stages(hip, ref, monkeypatch):
    """the formant stage itself -- envelope, pitch estimate, energy ratio per hop against oracle/_ref's private members,
    bound 1e-4 -- at presetDefault / 48 kHz on two streams of every signal type, for config 4b's parameters, an estimated base frequency
    and a formant shift."""
    _report("formant_stages/D48", pc.case_formant_stages(hip, ref, monkeypatch, D48, hops=30, streams=tuple(range(6))))


@pytest.mark.parametrize("preset", ["default", "cheaper"])
def test_presets_at_192k(hip, ref, preset):
    """signalsmith-stretch.h:63-68 at 192 kHz: 12288 / 10240 bins -- two FFT buffers do not fit a CU's LDS, the generic kernels keep the second
    one in memory (kAnalyse<true> / kSynth<true>).  Three stereo streams (sine, chirp, noise), 0.5 s, 1.25x, against the checker with the
    horizon-aware bound; the WASM fixtures of the same geometries run in test_golden."""
    n = 96000
    _batch_vs_ref(hip, ref, 3, 2, 192000, n, int(n*1.25), dict(preset=preset, sample_rate=192000.0), preset, "%s @ 192 kHz" % preset)


# ---------------------------------------------------------------------------------------------------------------
# Every accepted geometry (tests/geometry_cases.py): every band count, every vertical-step form, the (channels, bands, step) boundary grid
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,block", [(m, blk) for m in gc.band_counts() for blk in gc.blocks_for(m)])
def test_spectra_and_identity_every_band_count(hip, ref, M, block):
    """Band.input / .prevInput of every stream and channel against a float64 DFT (rel-RMS <= 1e-6, max bin <= 1e-5), and the 1.0x identity
    (<= 2e-6), at all 39 band counts, with block = fftSamples and with the shortest block above the previous band count."""
    print(gc.case_spectra_and_identity(hip, ref, M, block))


@pytest.mark.parametrize("M", gc.FAST_SIZES)
def test_fft_forms_spectra(hip, ref, monkeypatch, M):
    print(gc.case_fft_forms_spectra(hip, ref, monkeypatch, M))


@pytest.mark.parametrize("M", gc.FAST_SIZES)
def test_lean_tables_spectra(hip, ref, monkeypatch, M):
    """SMST_FFT_TABLES=lean at every register-blocked size (5120 / 6144: the 4 x 5 and 8 x 3 last stages, outputs prepared in four rounds)."""
    print(gc.case_lean_tables_spectra(hip, ref, monkeypatch, M))


@pytest.mark.parametrize("C,L", [(c, l) for l in sorted(gc.STEP_GEOMETRIES) for c in gc.SWEEP_CHANNELS if l <= gc.expected_limit(c)])
def test_vertical_step(hip, ref, C, L):
    print(gc.case_vertical_step(hip, ref, C, L))


@pytest.mark.parametrize("C,L", [(2, 5), (2, 6), (3, 5), (3, 6), (8, 5), (1, 9)])
def test_vertical_step_split(hip, ref, C, L):
    """split computation: one hop per call, the single-hop and across forms up to their edge (L = 5) and the forms past it"""
    print(gc.case_vertical_step(hip, ref, C, L, split=True, legs=("forced", "free")))


@pytest.mark.parametrize("C,L", [(2, 5), (2, 6), (3, 5), (3, 6), (1, 9)])
def test_vertical_step_realtime_quanta(hip, ref, C, L):
    gc.case_realtime_quanta_step(hip, ref, C, L)


def test_accepted_geometries_run(hip, monkeypatch):
    """(channels, bands, vertical step) boundary grid under SMST_CHECK_LAUNCHES=1: refused with the documented limit, or runs."""
    ran, refused = gc.case_accepted_geometries_run(hip, monkeypatch, range(1, 17), (2, 40, 2048, 16384), (1, 2, 5, 6, 7, 8, 14, 15, 30, 31, 59, 62, 63))
    assert (5, 2048, 59) in refused and (4, 16384, 62) in ran and (9, 2048, 30) in ran and (16, 16384, 14) in ran
