"""Twisted tiles (the previous-hop twist formed once per bin by the analysis pass and kept in the Xprev rows: kAnalyseTeamPairs<TWIST>, kTwistRows,
kVocoder ALIGNED TWISTED) against SMST_VOC_TWIST=0 (Band.prevInput in Xprev, the twist formed per record): shared by the CPU stand-in and the
GPU test.

A case is ONE batch geometry run twice over the same two calls, the second ragged (tests/analyse_pairs_cases.py: plan) -- the default form and
SMST_VOC_TWIST=0 -- and asserts that each call's output, the carried sums and window products after each call and the carried per-bin state
at the end are byte-identical, and by the launch counters which form ran in which call.  SMST_FFT_TEAMS=2 lets the small tiles of these batches
take the team kernels, as in the pair tests.

What the counters must say is derived from the rule, not from a run:
  * a call's tile is twisted when the batch takes kVocoder ALIGNED (mono / stereo, fp32 state, L = 4 -- or L <= 4 under SMST_ALIGN_ALL), the tile has
    more than one hop (a one-hop tile goes to the single-hop kernels), every hop of it re-analyses its previous window (not at stretch 1.0),
    no hop is mapped or pre-analysed (split computation: the block in flight), and the teams apply;
  * the first hop of a fresh stream has no input interval behind it: its time factor is clamped and drawn at random (HOP_RANDOM_TF), so the first
    tile of a batch's first call goes to the gathering producers -- raw.  The second call carries the cases;
  * the second call's first hop begins half an interval into it.  At stretch 1.5 and a block of 4 intervals (2.5: presetCheaper) its hop k has its window
    in the call from k = 6 on (4) and its previous window from k = 7 on (5): a stream with 9 or 12 hops has rows that the pair kernel turns
    (analyse_twist) and first rows that kTwistRows turns (twist_rows); with at most 3 hops no window lies in the call, no team kernel is launched
    and kTwistRows turns every row;
  * whoever turns them, a twisted call has analyse_twist + twist_rows > 0, and a raw call has neither."""
import numpy as np

from conftest import package, synth_input
from analyse_pairs_cases import plan

SWITCHES = ("SMST_FFT_TEAMS", "SMST_VOC_TWIST", "SMST_ALIGN_ALL")
COUNTERS = ("vocoder_twisted", "vocoder_aligned", "analyse_twist", "twist_rows", "analyse_pairs", "analyse_fast")

RAGGED = (7, 0, 9, 12)
DEFAULTS = dict(preset="default", sample_rate=48000, block=None, interval=None, split=None, channels=2, streams=4, stretch=1.5, hops1=9, hops2=RAGGED, in2=None,
                env={}, half_state=False, transpose=None, silent=None,
                twisted=(False, True), # which calls run the twisted form (with the default switches)
                pairs2=True)           # the second call has rows with both windows in the call, and rows without (None: not derived)
CASES = {
    # EXACT R3 = 12 (presetDefault at 48 kHz, M = 3072, L = 4), stereo and mono; a tile of 9 hops, then ragged tiles of up to 12
    "default_48k_stereo": dict(),
    "default_48k_mono": dict(channels=1),
    # tiles of 1 (the single-hop kernels: raw), 2 and 3 hops whose windows lie in the call
    "tile_of_1": dict(hops2=(1, 1, 0, 1), in2=12.0, twisted=(False, False)),
    "tile_of_2": dict(hops2=(2, 1, 0, 2), in2=9.0, pairs2=None),
    "tile_of_3": dict(hops2=(3, 2, 0, 3), in2=6.0, channels=1, pairs2=None),
    # a whole tile and the ramp behind it: 64 + 9 hops in the second call (the first call's second tile, nine hops with every window in the call, is twisted too)
    "whole_tile_and_9": dict(hops1=73, hops2=(73, 0, 66), streams=3, twisted=(True, True)),
    # every hop of the second call reaches into the history: kTwistRows alone
    "all_rows_late": dict(hops2=(2, 0, 3, 1), pairs2=False),
    # the run-time geometry (a block that is not 15/16 of the transform) at M = 3072, L = 4; R3 = 10 with L = 4, EXACT and run-time
    "runtime_geometry_3072": dict(block=5700, interval=1440),
    "r3_10_exact": dict(block=4800, interval=1280, channels=1),
    "r3_10_runtime": dict(block=4760, interval=1280),
    # L = 3 through the line-aligned producers
    "cheaper_align_all": dict(preset="cheaper", split=False, env={"SMST_ALIGN_ALL": "1"}),  # (the preset's own default is split computation)
    # a stream of zeros (the silence gate passes it through: it fires no hop)
    "one_stream_silent": dict(silent=1),
    # ---- tiles that do not qualify: both runs are raw, and equal
    "stretch_1": dict(stretch=1.0, twisted=(False, False)),
    "frequency_map": dict(transpose=1.25, twisted=(False, False)),
    "three_channels": dict(channels=3, twisted=(False, False)),
    "fp16_state": dict(half_state=True, twisted=(False, False)),
    "cheaper_l3": dict(preset="cheaper", split=False, twisted=(False, False)),
    # split computation: the block in flight at the end of the first call is the second call's pre-analysed row
    "split_preanalysed": dict(split=True, twisted=(False, False)),
}
# the CPU stand-in runs a kernel lane by lane: the index logic of the pass shape, of the late rows, of each geometry, and the host's rule
EMU_CASES = ("default_48k_stereo", "tile_of_1", "tile_of_3", "all_rows_late", "r3_10_runtime", "cheaper_align_all", "stretch_1", "split_preanalysed")


def run_form(lib, env, case, twist):
    """-> ({what: bytes}, [counter growth per call]) of one run; env: pytest's monkeypatch"""
    pkg = package()
    for k in SWITCHES:
        env.delenv(k, raising=False)
    env.setenv("SMST_FFT_TEAMS", "2")
    for k, val in case["env"].items():
        env.setenv(k, val)
    if not twist:
        env.setenv("SMST_VOC_TWIST", "0")
    S, C, sr = case["streams"], case["channels"], case["sample_rate"]
    if case["block"]:
        b = pkg.StretchBatch(S, C, block=case["block"], interval=case["interval"], split=bool(case["split"]), lib=lib, half_state=case["half_state"])
    else:
        b = pkg.StretchBatch(S, C, preset=case["preset"], sample_rate=sr, split=case["split"], lib=lib, half_state=case["half_state"])
    if case["transpose"]:
        b.setTransposeFactor(case["transpose"])
    calls = plan(case, b.intervalSamples())
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


def case_voc_twist(lib, monkeypatch, name):
    case = dict(DEFAULTS, **CASES[name])
    assert 2 <= case["streams"] <= 4
    twisted, grew_t = run_form(lib, monkeypatch, case, True)
    raw, grew_r = run_form(lib, monkeypatch, case, False)
    print(name, "default:", grew_t, "SMST_VOC_TWIST=0:", grew_r)
    for call in range(2):
        g = grew_t[call]
        if case["twisted"][call]:
            assert g["vocoder_twisted"] > 0 and g["vocoder_twisted"] == g["vocoder_aligned"], (name, call, g)
            assert g["analyse_twist"] + g["twist_rows"] > 0, (name, call, g)
        else:
            assert g["vocoder_twisted"] == 0 and g["analyse_twist"] == 0 and g["twist_rows"] == 0, (name, call, g)
        g = grew_r[call]
        assert g["vocoder_twisted"] == 0 and g["analyse_twist"] == 0 and g["twist_rows"] == 0, (name, call, g)
    if case["twisted"][1] and case["pairs2"] is not None:
        g = grew_t[1]
        assert g["twist_rows"] > 0 and g["analyse_fast"] > 0, (name, g)  # the first hops of the call reach into the history
        assert (g["analyse_twist"] > 0) == case["pairs2"], (name, g)
    if name == "whole_tile_and_9":  # first call: the second tile alone, no late row; second call: both tiles, late rows in the first
        assert [grew_t[0][k] for k in ("vocoder_twisted", "analyse_twist", "twist_rows")] == [1, 1, 0], (name, grew_t[0])
        assert [grew_t[1][k] for k in ("vocoder_twisted", "analyse_twist", "twist_rows")] == [2, 2, 1], (name, grew_t[1])
    assert sorted(twisted) == sorted(raw)
    differing = [k for k in sorted(twisted) if twisted[k] != raw[k]]
    assert not differing, (name, differing)
