"""Cases over the whole range of geometries the constructor accepts (include/smst.h "Limits"), shared by the CPU-emulated run
(test_parity_emu.py, a subset) and the real gfx950 run (test_parity_gpu.py, the full grid).

Which kernels run depends on the band count M = fftSamples/2 and the vertical step L = round(fftSamples/interval):
  * FFT: the register-blocked kernels at M = 2560 / 3072 / 5120 / 6144, the generic radix-4/2/3/5 ladder everywhere else, with
    the second ping-pong buffer in memory above 9600 bands;
  * recurrence: kVocoder (1-2 channels, L = 2..7), kVocoderN and the single-hop / across forms (3-8 channels, L = 2..5), and
    kPredictB + kChain for every other combination, whose LDS ring has 4 / 8 / 16 / 32 / 64 slots depending on L.
The cases here compare the analysis spectra with a float64 DFT at every band count, pin the identity at every band count, sweep the
vertical step against the checker, and walk the (channels, bands, step) boundary grid."""
import numpy as np

import parity_cases as pc
from conftest import package, rel_rms, synth_input

TOL_SPECTRUM_RMS = 1e-6  # rel-RMS of one hop's spectrum (per channel) against the float64 DFT of the same float32 samples and window
TOL_SPECTRUM_MAX = 1e-5  # largest bin error, relative to the hop's largest |X|
MAX_BANDS = 16384        # the largest band count {1,2,3,4,5,6,8}*2^k reaches below the LDS limit of 19200 (include/smst.h)
FAST_SIZES = (2560, 3072, 5120, 6144)  # the register-blocked FFT's band counts (smst_fft.hip)


def band_counts(hi=MAX_BANDS):
    """Every band count a block of at least 4 samples can produce: {2,3,4,5,6,8}*2^k up to `hi` (39 sizes up to 16384)."""
    return sorted({m << k for m in (2, 3, 4, 5, 6, 8) for k in range(15) if 2 <= (m << k) <= hi})


def blocks_for(M):
    """Two blocks with M bands: block = fftSamples, and the shortest block above the previous band count (an odd block whose window
    covers only part of the FFT: the zero-padding branches of the analysis)."""
    sizes = band_counts(1 << 20)
    i = sizes.index(M)
    return (2*M,) if i == 0 else (2*M, 2*sizes[i - 1] + 1)


def expected_limit(channels):
    """The longest vertical step the constructor accepts for `channels` (include/smst.h): kChain's ring of a power of two >= L + 2 slots
    per channel and lane, plus a 128-bin stage per channel, has to fit 160 KiB of LDS; the fused kernels' skew stops at 62."""
    for L in range(62, 0, -1):
        ring = 4
        while ring < L + 2:
            ring *= 2
        if (channels*ring*64 + channels*128)*8 <= 160*1024:
            return L
    return 0


def vertical_step(block, interval):
    M = _bands_of_block(block)
    return max(1, int(np.round(np.float32(2*M)/np.float32(interval))))


def _bands_of_block(block):
    """fftSamples/2 for a block (smst_engine.cpp fastSizeAbove, signalsmith-stretch.h's choice of fast sizes)."""
    size = (block + 1)//2
    power2 = 1
    while power2*8 < size:
        power2 *= 2
    multiple = (size + power2 - 1)//power2
    if multiple == 7:
        multiple += 1
    return multiple*power2


def dft_spectrum(block, window, N):
    """X[k] = sum_n x[n] w[n] exp(-2 pi i (k + 1/2) n / N), n centred on block//2, unnormalised (test_modified_spectrum_definition), in
    float64: the samples and the window are taken as the exact float32 values both implementations start from."""
    B = block.shape[-1]
    n = np.arange(B) - B//2
    v = np.asarray(block, np.float64)*np.asarray(window, np.float64)*np.exp(-1j*np.pi*n/N)
    buf = np.zeros(block.shape[:-1] + (N,), np.complex128)
    buf[..., n % N] = v
    return np.fft.fft(buf, axis=-1)[..., :N//2]


def _block_ending(x, end, B):
    """The B input samples before `end` (zero before the stream's start): [C, B]."""
    out = np.zeros((x.shape[0], B), np.float32)
    lo = max(0, end - B)
    if end > lo:
        out[:, B - (end - lo):] = x[:, lo:end]
    return out


def _spectrum_errors(got, want):
    """Per channel: (rel-RMS, max bin error / max|X|) of one hop."""
    got, want = np.asarray(got, np.complex128), np.asarray(want, np.complex128)
    res = []
    for g, w in zip(got, want):
        scale = float(np.abs(w).max())
        res.append((float(np.sqrt(np.mean(np.abs(g - w)**2)/max(np.mean(np.abs(w)**2), 1e-300))), float(np.abs(g - w).max())/max(scale, 1e-300)))
    return res


def _assert_spectrum(got, want, label):
    worst = (0.0, 0.0)
    for c, (e_rms, e_max) in enumerate(_spectrum_errors(got, want)):
        assert e_rms <= TOL_SPECTRUM_RMS and e_max <= TOL_SPECTRUM_MAX, "%s, channel %d: spectrum vs float64 DFT rel-RMS %.3e (<= %.0e), max bin %.3e (<= %.0e)" % (
            label, c, e_rms, TOL_SPECTRUM_RMS, e_max, TOL_SPECTRUM_MAX)
        worst = (max(worst[0], e_rms), max(worst[1], e_max))
    return worst


def case_spectra_and_identity(lib, ref, M, block, channels=2, streams=3, hops=None, label=""):
    """Items 1 and 2 at one geometry, 1.0x / 0 st, hop-aligned calls (one interval in, one out):
      * after every call, Band.input and Band.prevInput of every stream and channel against the float64 DFT of the block the reference
        analyses: at a hop-aligned call the new block starts at output index 0, so inputOffset = 0 and the analysed block ends where the
        previous call's input ended (signalsmith-stretch.h:281-295); at the end of the hop prevInput holds the same spectrum (the next
        hop's previous input), so both are compared with the same DFT.  The checker's own
        Band.input must meet the same bound at the same offset (that pins the offset, and shows the bound is tight);
      * the concatenated output against the input delayed by inputLatency + outputLatency, past the first two blocks.
    Returns the worst figures."""
    pkg = package()
    interval = max(1, block//4)
    b = pkg.StretchBatch(streams, channels, block=block, interval=interval, lib=lib)
    assert b.bands() == M, (block, b.bands(), M)
    B, I, N = b.blockSamples(), b.intervalSamples(), b.fftSamples()
    lat = b.inputLatency() + b.outputLatency()
    if hops is None:
        hops = -(-(lat + 2*B + 4*I)//I) + 1
    sr = 48000
    xs = np.stack([synth_input(s, channels, hops*I, sr) for s in range(streams)])
    r = ref.RefStretch(0)
    r.configure(channels, B, I)
    w = r.window()
    assert w.shape == (B,) and r.fftSamples() == N
    worst = dict(product=(0.0, 0.0), checker=(0.0, 0.0))
    ys = []
    for k in range(hops):
        ys.append(np.array(b.process(np.ascontiguousarray(xs[:, :, k*I:(k + 1)*I]), I), copy=True))
        r.process(xs[0][:, k*I:(k + 1)*I], I)
        if k == 0:
            continue  # nothing but zeros before the first call
        for s in range(streams):
            want = dft_spectrum(_block_ending(xs[s], k*I, B), w, N)
            for which in (0, 1):
                tag = "%s M=%d block=%d interval=%d stream %d hop %d %s" % (label, M, B, I, s, k, ("Band.input", "Band.prevInput")[which])
                e = _assert_spectrum(b.debug_state(s, which), want, tag)
                worst["product"] = tuple(max(a, c) for a, c in zip(worst["product"], e))
                if s == 0:
                    e = _assert_spectrum(r.bands_complex(which), want, tag + " (checker)")
                    worst["checker"] = tuple(max(a, c) for a, c in zip(worst["checker"], e))
    b.close()
    y = np.concatenate(ys, axis=2)
    n = hops*I
    skip = 2*B
    assert n - lat - skip >= 4*I, (M, block, n, lat)
    worst["identity"] = rel_rms(y[:, :, lat + skip:n], xs[:, :, skip:n - lat])
    assert worst["identity"] <= pc.TOL_EXACT, "%s M=%d block=%d: identity rel-RMS %.3e > %.0e" % (label, M, B, worst["identity"], pc.TOL_EXACT)
    return worst


def _one_long_call(lib, ref, M, block, channels, streams, label):
    """One long call: hops at output indices 0, I, 2I, ... (samplesSinceLast starts past the interval), the last one at K*I, its frame
    inside the call's own input: both spectra of every stream against the float64 DFT, and the identity.  Returns (worst spectrum, identity)."""
    pkg = package()
    b = pkg.StretchBatch(streams, channels, block=block, interval=block//4, lib=lib)
    B, I, N = b.blockSamples(), b.intervalSamples(), b.fftSamples()
    assert N == 2*M
    K = 12
    n = K*I + 1
    xs = np.stack([synth_input(s, channels, n, 48000) for s in range(streams)])
    y = np.asarray(b.process(xs, n))
    r = ref.RefStretch(0)
    r.configure(channels, B, I)
    r.process(xs[0], n)
    w = r.window()
    long_worst = (0.0, 0.0)
    for s in range(streams):
        want = dft_spectrum(_block_ending(xs[s], K*I, B), w, N)
        for which in (0, 1):
            e = _assert_spectrum(b.debug_state(s, which), want, "%s M=%d one call, stream %d state %d" % (label, M, s, which))
            long_worst = tuple(max(a, c) for a, c in zip(long_worst, e))
            if s == 0:
                _assert_spectrum(r.bands_complex(which), want, "%s M=%d one call (checker) state %d" % (label, M, which))
    lat = b.inputLatency() + b.outputLatency()
    ident = rel_rms(y[:, :, lat + 2*B:n], xs[:, :, 2*B:n - lat])
    assert ident <= pc.TOL_EXACT, (label, M, ident)
    b.close()
    return long_worst, ident


def case_fft_forms_spectra(lib, ref, monkeypatch, M, channels=2, streams=3):
    """At a register-blocked size: per-frame (SMST_FFT_TEAMS=0), team (=2) and generic (SMST_NO_FAST_FFT=1) kernels, each against the
    float64 DFT, at the preset's block (15/8 of the bands: the window leaves the padding the team kernels' element slots need) --
    hop-aligned calls (case_spectra_and_identity: those frames reach into the carried history) and one long call whose last hop's frame
    lies inside the call's own input (where the team kernels take it: only at 2560 / 3072 bands).  Launch counts prove which form ran.
    Returns the worst figures per form."""
    pkg = package()
    block = 15*M//8
    teams_size = M in (2560, 3072)
    forms = (("per_frame", dict(SMST_FFT_TEAMS="0")), ("teams", dict(SMST_FFT_TEAMS="2")), ("generic", dict(SMST_NO_FAST_FFT="1")))
    names = ("analyse_fast", "analyse_teams", "analyse_generic", "synth_fast", "synth_teams", "synth_generic", "synth_emit")
    results = {}
    for form, env in forms:
        for key in ("SMST_FFT_TEAMS", "SMST_NO_FAST_FFT"):
            monkeypatch.delenv(key, raising=False)
        for key, v in env.items():
            monkeypatch.setenv(key, v)
        before = {k: pkg.launch_count(k, lib) for k in names}
        worst = case_spectra_and_identity(lib, ref, M, block, channels, streams, label=form)
        long_worst, ident = _one_long_call(lib, ref, M, block, channels, streams, form)
        grew = {k: pkg.launch_count(k, lib) - before[k] for k in names}
        if form == "generic":
            ok = grew["analyse_generic"] > 0 and grew["synth_generic"] > 0 and all(grew[k] == 0 for k in names if not k.endswith("generic"))
        elif form == "teams" and teams_size:
            ok = grew["analyse_teams"] > 0 and (grew["synth_teams"] > 0 or grew["synth_emit"] > 0) and grew["analyse_generic"] == 0
        else:  # per-frame (and SMST_FFT_TEAMS=2 at 5120 / 6144 bands, which have no team kernels)
            ok = grew["analyse_fast"] > 0 and grew["synth_fast"] > 0 and all(grew[k] == 0 for k in ("analyse_teams", "synth_teams", "synth_emit", "analyse_generic", "synth_generic"))
        assert ok, (form, M, "unexpected FFT kernel forms", grew)
        worst["one_call"] = long_worst
        worst["one_call_identity"] = ident
        results[form] = worst
    for key in ("SMST_FFT_TEAMS", "SMST_NO_FAST_FFT"):
        monkeypatch.delenv(key, raising=False)
    return results


def case_lean_tables_spectra(lib, ref, monkeypatch, M, channels=2, streams=3):
    """SMST_FFT_TABLES=lean at a register-blocked size, the preset's block, under the same bounds as the full tables: hop-aligned calls
    (case_spectra_and_identity: every frame reaches into the carried history, the kernels' general path) and one long call (the frames
    inside the call's input take the usual-case path).  SMST_FFT_TEAMS=2 asks for the team kernels wherever they are allowed, so the
    launch counts -- the per-frame kernels ran, no team and no generic kernel did -- hold only because the lean tables are in force.
    Returns the worst figures."""
    pkg = package()
    names = ("analyse_fast", "analyse_teams", "analyse_generic", "synth_fast", "synth_teams", "synth_generic", "synth_emit")
    monkeypatch.setenv("SMST_FFT_TABLES", "lean")
    monkeypatch.setenv("SMST_FFT_TEAMS", "2")
    before = {k: pkg.launch_count(k, lib) for k in names}
    worst = case_spectra_and_identity(lib, ref, M, 15*M//8, channels, streams, label="lean")
    worst["one_call"], worst["one_call_identity"] = _one_long_call(lib, ref, M, 15*M//8, channels, streams, "lean")
    grew = {k: pkg.launch_count(k, lib) - before[k] for k in names}
    monkeypatch.delenv("SMST_FFT_TABLES")
    monkeypatch.delenv("SMST_FFT_TEAMS")
    assert grew["analyse_fast"] > 0 and grew["synth_fast"] > 0 and all(grew[k] == 0 for k in names if not k.endswith("_fast")), (M, "lean tables: unexpected FFT kernel forms", grew)
    return worst


# ---------------------------------------------------------------------------------------------------------------
# Vertical-step sweep (item 3) and the boundary grid (item 4)
# ---------------------------------------------------------------------------------------------------------------
# (block, interval) with fftSamples 1024 (2048 for 62: no interval gives round(1024/interval) = 62; for 1 an interval below the block, so
# that the overlap-add ring still holds a frame's tail after the hop) for every vertical step the sweep visits:
# every ring boundary (L + 2 = 4 | 8 | 16 | 32 | 64 slots) and every template edge of the fused kernels (2..7 for 1-2 channels, 2..5 for 3-8)
STEP_GEOMETRIES = {1: (1024, 800), 2: (1024, 512), 3: (1024, 341), 4: (1024, 256), 5: (1024, 205), 6: (1024, 171), 7: (1024, 146),
                   8: (1024, 128), 9: (1024, 114), 14: (1024, 73), 15: (1024, 68), 30: (1024, 34), 31: (1024, 33), 62: (2048, 33)}
SWEEP_CHANNELS = (1, 2, 3, 5, 8, 9, 16)
FUSED_COUNTERS = ("vocoder_aligned", "vocoder_staged", "vocoder_gather", "vocoder_n", "vocoder_one", "vocoder_across", "vocoder_continuous")


def fused_expected(C, L):
    """smst_vocoder.hip fusedSupported(): the records stay in LDS (kVocoder / kVocoderN / single-hop / across); otherwise kPredictB + kChain."""
    return C <= 8 and 2 <= L <= (7 if C <= 2 else 5)


def _recurrence_form(lib, before):
    pkg = package()
    grew = {k: pkg.launch_count(k, lib) - v for k, v in before.items()}
    return grew


def _counters(lib):
    pkg = package()
    return {k: pkg.launch_count(k, lib) for k in FUSED_COUNTERS + ("chain_unfused",)}


def _assert_form(C, L, grew, label):
    if fused_expected(C, L):
        assert grew["chain_unfused"] == 0 and sum(grew[k] for k in FUSED_COUNTERS) > 0, (label, "expected a fused recurrence", grew)
    else:
        assert grew["chain_unfused"] > 0 and sum(grew[k] for k in FUSED_COUNTERS) == 0, (label, "expected kPredictB + kChain", grew)


def case_vertical_step(lib, ref, C, L, split=False, legs=("forced", "magnitudes", "free"), stretch=1.3, semitones=2.0):
    """One point of the sweep: channels C, vertical step L, 1.3x, channel energies that differ (as case_channels):
      * teacher-forced single hops (fixed one-hop bounds: the strong leg);
      * phase-free per-hop magnitudes, free running, at +2 st as well;
      * the free-running sample-domain comparison (check_scenario's bounds).  Mono at L = 1 has no informative first horizon (every
        output bin is its own maximum channel and the phase follows the b-1 tap alone): there the teacher-forced leg carries the point.
    The two legs with fixed bounds run without a frequency map: at 1024 bins a +2 st map's peak runs are decided by near-ties in two to
    five of nine forced hops on the MI355X (at every step, in the long-tested kVocoder forms too -- _flip_margin explains every one), and
    a flipped run moves whole groups of bins.  The vertical step lives in the recurrence's b-1 / b-L taps, which plain stretching drives
    just as hard; the pitch-mapped path is the magnitude leg's, whose bound admits explained flips.
    Launch counts prove the recurrence form.  Returns the figures."""
    block, interval = STEP_GEOMETRIES[L]
    assert vertical_step(block, interval) == L, (block, interval, vertical_step(block, interval), L)
    cfg = dict(preset="configure", block=block, interval=interval, split=split)
    label = "C=%d L=%d%s" % (C, L, " split" if split else "")
    setup = (lambda o: o.setTransposeSemitones(semitones, 0.2)) if semitones else None
    gains = [1 - 0.05*c for c in range(C)]
    out = {}
    if "forced" in legs:
        before = _counters(lib)
        f = pc.case_teacher_forced(lib, ref, cfg, C, stretch, label + " forced", gains=gains)
        _assert_form(C, L, _recurrence_form(lib, before), label + " forced")
        # the teacher-forced ratio: the worst hop's spectrum distance over its bound max(TOL_FORCED_SPECTRUM, SELF_FACTOR x the checker's own)
        out["forced_ratio"] = f["spectrum_outside_all_ties"]/max(pc.TOL_FORCED_SPECTRUM, pc.SELF_FACTOR*f["spectrum_self_outside_all_ties"])
        out["forced_spectrum"] = f["spectrum_outside_all_ties"]
    if "magnitudes" in legs:
        before = _counters(lib)
        m = pc.case_hop_magnitudes(lib, ref, cfg, C, stretch, label + " magnitudes", setup=setup, hops=20)
        _assert_form(C, L, _recurrence_form(lib, before), label + " magnitudes")
        out["magnitude"] = m["magnitude"]
    if "free" in legs:
        n = 6*block
        x = synth_input(3, C, n, 48000)*(1 + 0.3*np.arange(C))[:, None].astype(np.float32)
        nout = int(n*stretch)
        play = lambda o, xx: o.process(xx, nout)  # noqa: E731
        before = _counters(lib)
        g = pc.make("product", lib, ref, C, cfg)
        y = play(g, x)
        _assert_form(C, L, _recurrence_form(lib, before), label + " free")
        o = play(pc.make("ref", lib, ref, C, cfg), x)
        o2 = [play(pc.make("ref", lib, ref, C, cfg), pc.perturbed(x, seed)) for seed in pc.SELF_SEEDS]
        out["free_hops"] = pc.assert_parity(y, o, o2, interval, label + " free", require_informative=not (C == 1 and L == 1))
        out["free"] = rel_rms(y, o)
    return out


def case_realtime_quanta_step(lib, ref, C, L):
    """The AudioWorklet pattern (128-sample quanta, one hop or none per call: the single-hop and across forms where they apply) at
    vertical step L against the checker."""
    block, interval = STEP_GEOMETRIES[L]
    cfg = dict(preset="configure", block=block, interval=interval, split=False)
    before = _counters(lib)
    x = synth_input(0, C, 128*60, 48000)*(1 + 0.3*np.arange(C))[:, None].astype(np.float32)

    def play(o, xx):
        return np.concatenate([o.process(np.ascontiguousarray(xx[:, q*128:(q + 1)*128]), 128) for q in range(xx.shape[1]//128)], axis=1)
    pc.check_scenario(lib, ref, cfg, x, play, "C=%d L=%d quanta" % (C, L))
    _assert_form(C, L, _recurrence_form(lib, before), "C=%d L=%d quanta" % (C, L))


def case_accepted_geometries_run(lib, monkeypatch, channel_counts, bands, steps, hops=3):
    """Every (channels, bands, vertical step) point is either refused at construction (SMST_ERR_INVALID, the limit in smst_last_error())
    or runs `hops` hops under SMST_CHECK_LAUNCHES=1 -- and which of the two happens is the documented limit (expected_limit)."""
    pkg = package()
    monkeypatch.setenv("SMST_CHECK_LAUNCHES", "1")
    ran, refused = [], []
    for M in bands:
        N = 2*M
        for L in steps:
            interval = None
            for I in range(max(1, N//(L + 1)), N//max(L - 1, 1) + 2):
                if 1 <= I <= N and max(1, int(np.round(np.float32(N)/np.float32(I)))) == L:
                    interval = I
                    break
            if interval is None:
                continue  # no interval gives this step at this size
            for C in channel_counts:
                label = "C=%d M=%d L=%d (block %d, interval %d)" % (C, M, L, N, interval)
                ok = L <= 62 and L <= expected_limit(C)
                try:
                    b = pkg.StretchBatch(1, C, block=N, interval=interval, lib=lib)
                except pkg.StretchError as e:
                    msg = str(e)
                    assert not ok, "%s: refused, but the documented limit accepts it: %s" % (label, msg)
                    assert msg.startswith("smst error -1:"), (label, msg)
                    assert ("vertical step" in msg and str(expected_limit(C)) in msg) or "interval too small" in msg, (label, msg)
                    refused.append((C, M, L))
                    continue
                assert ok, "%s: accepted beyond the documented limit" % label
                try:
                    assert b.bands() == M
                    n = N + hops*interval
                    x = np.ascontiguousarray(synth_input(0, C, n, 48000)[None])
                    y = np.asarray(b.process(x, n))
                    b.synchronize()
                finally:
                    b.close()
                assert np.isfinite(y).all() and np.abs(y).max() > 0, (label, "no output")
                ran.append((C, M, L))
    monkeypatch.delenv("SMST_CHECK_LAUNCHES", raising=False)
    return ran, refused
