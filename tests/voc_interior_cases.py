"""The interior form of the line-aligned producers' block (kVocoder ALIGNED: vocoderProduceAligned, the blocks of a producer wave between its rows'
edges) against SMST_VOC_INTERIOR=0 (the general form, with its clamps, zero selects and lane masks, in every block): shared by the CPU stand-in
and the GPU test.

A case is ONE small batch run twice over the same two calls, the second ragged (tests/analyse_pairs_cases.py: plan) -- the default form and
SMST_VOC_INTERIOR=0 -- and asserts that each call's output, the carried sums and window products after each call and the carried per-bin state at
the end are byte-identical, and by the launch counters which form ran in which call.  Neither run is the authority: the general form is the code the
other suites pin against the checker and against the other producer forms.

What the counters must say is derived from the rule (smst_vocoder.hip), not from a run:
  * the silence gate passes a stream through, and it fires no hop, once 2*block samples of silence lie behind it: the first call (13 hops at
    stretch 1.5: more than 8 intervals of input, and a block is 4 intervals, 2.5 in presetCheaper) makes the all-zero stream such a one for the second;
  * the first hop of a fresh stream draws its time factors at random, so the first tile of a batch's first call goes to the gathering producers; the
    second call carries the cases (and, where the first call has more than 64 hops, its second tile);
  * a tile of a call goes to kVocoder ALIGNED when the batch qualifies (mono / stereo, fp32 state, no frequency map, L = 4 -- or L <= 4 under
    SMST_ALIGN_ALL -- and a band count that is a multiple of 16) and some stream has more than one hop in it: `vocoder_aligned` counts those tiles;
  * such a tile is twisted, unless SMST_VOC_TWIST=0, where the analysis teams exist for the band count (256*R3): `vocoder_twisted`;
  * wave `it` of a stream's producers owns hops 8*it .. 8*it + 7 and runs interior blocks when all eight are hops of the tile and the pair range
    8 <= mw, mw + 1 <= M/8 - 5 is not empty (M >= 112): `vocoder_interior` counts the aligned tiles in which some stream has 8 hops or more, and
    nothing with SMST_VOC_INTERIOR=0."""
import numpy as np

from conftest import package, synth_input
from analyse_pairs_cases import plan

SWITCHES = ("SMST_FFT_TEAMS", "SMST_VOC_TWIST", "SMST_ALIGN_ALL", "SMST_VOC_INTERIOR")
COUNTERS = ("vocoder_interior", "vocoder_aligned", "vocoder_twisted")
TEAM_BANDS = (2560, 3072, 5120, 6144)

DEFAULTS = dict(preset="default", sample_rate=48000, block=None, interval=None, split=None, channels=2, streams=4, stretch=1.5, hops1=13, hops2=(8, 0, 9, 12), in2=None,
                env={}, half_state=False, transpose=None, silent=3,
                bands=3072,    # what the geometry must come to (asserted): the rule's M
                aligned=True)  # the batch qualifies for kVocoder ALIGNED
RAW = {"SMST_VOC_TWIST": "0"}
CASES = {
    # presetDefault at 48 kHz (M = 3072, L = 4, the twisted form), stereo: stream 1 has no hop, stream 3 is silent (the gate passes it through).
    # 8 hops: the first producer alone is whole; 9: a whole wave beside a partial one; 7: no whole wave -- the general form everywhere
    "stereo_8_9": dict(),
    "stereo_7_17": dict(hops2=(7, 0, 17, 12)),
    "stereo_15_16": dict(hops2=(15, 0, 16, 12)),
    "stereo_7_only": dict(hops2=(7, 0, 5, 12)),
    "stereo_64": dict(hops2=(64, 0, 33, 12)),  # all eight waves
    # a whole tile and a short second one (64 + 9), in both calls
    "stereo_64_and_9": dict(hops1=73, hops2=(73, 0, 66, 12)),
    # the same raggedness without a silent stream, mono
    "mono_8_9_17": dict(channels=1, hops2=(8, 9, 17, 0), silent=None),
    "mono_15_16": dict(channels=1, hops2=(15, 0, 16, 12)),
    # SMST_VOC_TWIST=0 in both runs: the raw aligned form (rotation factors requested, the twist per record)
    "raw_stereo_8_9_17": dict(hops2=(8, 9, 17, 0), silent=None, env=RAW),
    "raw_mono_7_16": dict(channels=1, hops2=(7, 0, 16, 12), env=RAW),
    "raw_stereo_64_and_9": dict(hops1=73, hops2=(73, 0, 66, 12), env=RAW),
    # the run-time geometry at 3072 bins; R3 = 10 (M = 2560: another interior length)
    "runtime_geometry_3072": dict(block=5700, interval=1440, hops2=(9, 0, 17, 12)),
    "r3_10": dict(block=4800, interval=1280, bands=2560, hops2=(8, 0, 17, 12)),
    "r3_10_mono_raw": dict(block=4800, interval=1280, bands=2560, channels=1, hops2=(15, 0, 9, 12), env=RAW),
    # L = 3 through the line-aligned producers: the edge conditions depend on L
    "cheaper_align_all": dict(preset="cheaper", split=False, bands=2560, env={"SMST_ALIGN_ALL": "1"}, hops2=(8, 9, 17, 0), silent=None),
    "cheaper_align_all_mono_raw": dict(preset="cheaper", split=False, bands=2560, channels=1, env={"SMST_ALIGN_ALL": "1", "SMST_VOC_TWIST": "0"}, hops2=(16, 0, 9, 12)),
    # the smallest geometries: four intervals per block, band counts that are multiples of 16.  256 bands: interior pairs mw = 8 .. 26, ten of the
    # 39 blocks a wave is active in; 96 bands: 96/8 - 5 < 9, no interior pair -- the counter must not grow
    "small_256": dict(block=512, interval=128, bands=256, hops2=(8, 9, 17, 0), silent=None),
    "small_256_mono_two_tiles": dict(block=512, interval=128, bands=256, channels=1, hops1=73, hops2=(73, 0, 66, 12)),
    "small_96_empty": dict(block=192, interval=48, bands=96, hops2=(8, 9, 17, 0), silent=None),
    # ---- tiles that do not take the aligned kernel: both runs equal, the counter stays 0
    "frequency_map": dict(transpose=1.25, hops2=(9, 0, 17, 12), aligned=False),
    "three_channels": dict(channels=3, hops2=(9, 0, 17, 12), aligned=False),
    "fp16_state": dict(half_state=True, hops2=(9, 0, 17, 12), aligned=False),
}
# the CPU stand-in runs a kernel lane by lane: the index logic of the block range, of both producer kinds, of each L, and the host's rule
EMU_CASES = ("stereo_8_9", "mono_8_9_17", "small_256", "small_96_empty", "cheaper_align_all_mono_raw", "fp16_state")


def expected_counters(case, interior):
    """-> [{counter: growth} per call], from the rule in the module's docstring"""
    M = case["bands"]
    silent = case["silent"]  # all zeros: counts hops in the first call, gated in the second (run_form asserts that it is)
    per_call = []
    for call, hops in enumerate((case["hops1"], None)):
        S = case["streams"]
        if call == 0:
            counts = [hops for s in range(S)]
        else:
            counts = [0 if s == silent else case["hops2"][s % len(case["hops2"])] for s in range(S)]
        most = max(counts)
        want = dict.fromkeys(COUNTERS, 0)
        for tile in range((most + 63)//64):
            tile_hops = min(64, most - 64*tile)
            if not case["aligned"] or tile_hops < 2 or (call == 0 and tile == 0):
                continue
            want["vocoder_aligned"] += 1
            if case["env"].get("SMST_VOC_TWIST") != "0" and M in TEAM_BANDS:
                want["vocoder_twisted"] += 1
            if interior and tile_hops >= 8 and 8 + 1 <= M//8 - 5:
                want["vocoder_interior"] += 1
        per_call.append(want)
    return per_call


def run_form(lib, env, case, interior):
    """-> ({what: bytes}, [counter growth per call]) of one run; env: pytest's monkeypatch"""
    pkg = package()
    for k in SWITCHES:
        env.delenv(k, raising=False)
    env.setenv("SMST_FFT_TEAMS", "2")
    for k, val in case["env"].items():
        env.setenv(k, val)
    if not interior:
        env.setenv("SMST_VOC_INTERIOR", "0")
    S, C, sr = case["streams"], case["channels"], case["sample_rate"]
    if case["block"]:
        b = pkg.StretchBatch(S, C, block=case["block"], interval=case["interval"], split=bool(case["split"]), lib=lib, half_state=case["half_state"])
    else:
        b = pkg.StretchBatch(S, C, preset=case["preset"], sample_rate=sr, split=case["split"], lib=lib, half_state=case["half_state"])
    assert b.bands() == case["bands"], (b.bands(), case["bands"])
    if case["transpose"]:
        b.setTransposeFactor(case["transpose"])
    calls = plan(case, b.intervalSamples())
    if case["silent"] is not None:  # the gate's rule: 2*block samples of silence before the second call
        assert calls[0][0][case["silent"]] >= 2*b.blockSamples(), (calls[0][0], b.blockSamples())
    n_total = int(sum(n_in.max() for n_in, _ in calls))
    x = np.stack([synth_input(s, C, n_total, sr) for s in range(S)])
    if case["silent"] is not None:
        x[case["silent"]] = 0.0
    got, grew = {}, []
    pos = np.zeros(S, np.int64)
    for call, (n_in, n_out) in enumerate(calls):
        before = {k: pkg.launch_count(k, lib) for k in COUNTERS}
        xin = np.zeros((S, C, int(n_in.max())), np.float32)
        for s in range(S):
            xin[s, :, :n_in[s]] = x[s, :, pos[s]:pos[s] + n_in[s]]
        pos += n_in
        y = np.array(b.process(xin, n_out.astype(np.int32), in_samples=n_in.astype(np.int32)), copy=True)
        if call == 0:
            assert float(np.abs(y).max()) > 0.05
        got["output %d" % call] = np.concatenate([y[s, :, :n_out[s]].ravel() for s in range(S)]).tobytes()
        carry = [b.debug_carry(s) for s in range(S)]
        got["carried sums %d" % call] = np.concatenate([c[0].ravel() for c in carry]).tobytes()
        got["carried products %d" % call] = np.concatenate([c[1].ravel() for c in carry]).tobytes()
        grew.append({k: pkg.launch_count(k, lib) - before[k] for k in COUNTERS})
    for which, what in enumerate(("input", "previous input", "output", "energy")):
        got["state: " + what] = np.concatenate([np.asarray(b.debug_state(s, which)).ravel() for s in range(S)]).tobytes()
    b.close()
    for k in SWITCHES:
        env.delenv(k, raising=False)
    return got, grew


def case_voc_interior(lib, monkeypatch, name):
    case = dict(DEFAULTS, **CASES[name])
    assert 2 <= case["streams"] <= 4
    inner, grew_i = run_form(lib, monkeypatch, case, True)
    general, grew_g = run_form(lib, monkeypatch, case, False)
    print(name, "default:", grew_i, "SMST_VOC_INTERIOR=0:", grew_g)
    assert grew_i == expected_counters(case, True), (name, grew_i, expected_counters(case, True))
    assert grew_g == expected_counters(case, False), (name, grew_g, expected_counters(case, False))
    assert sorted(inner) == sorted(general)
    differing = [k for k in sorted(inner) if inner[k] != general[k]]
    assert not differing, (name, differing)
