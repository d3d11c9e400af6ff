"""Which form of the bin recurrence a tile takes (csrc/smst_recurrence_form.h: recurrenceForm), pinned against the commit before that function
existed: shared by the CPU stand-in and the GPU test.

Until then the decision was spread over the engine's tile loop and three levels of launchers.  A scenario is ONE small batch, two calls (the
second ragged: tests/analyse_pairs_cases.py, plan) and a set of switches, and asserts
  * the growth of every recurrence launch counter over each call -- the decision itself, tile by tile;
  * SHA-256 digests of each call's output, of the carried sums and window products after each call and of the carried per-bin state at the end;
  * `shows`: the counters that must have grown for the scenario to have reached the branch of the decision it is here for (from the rule, not
    from a run: DESIGN.md section 3).
The first two are compared with what the parent commit gave, kept under tests/golden/ (recurrence_forms_parent_gpu.json: recorded on an MI355X;
recurrence_forms_parent_emu.json: from the CPU stand-in).  The counters are decided on the host, so the two files must agree on them.

The `flush` scenarios drive one stream object instead: a split-computation block that a flush() interrupts inside its main prediction
(tests/parity_cases.py: case_split_mid_interval_flush) runs with HopDesc.startBin > 0 -- never lanes-across-streams, never bounded producers.

`python tests/recurrence_form_cases.py record gpu|emu <file> [scenario ...]` writes the digests and counters of the library it runs on."""
import hashlib
import json
import os

import numpy as np

from conftest import ROOT, package, synth_input
from analyse_pairs_cases import plan

GOLDEN = {kind: os.path.join(ROOT, "tests", "golden", "recurrence_forms_parent_%s.json" % kind) for kind in ("gpu", "emu")}
SWITCHES = ("SMST_FFT_TEAMS", "SMST_VOC_TWIST", "SMST_VOC_INTERIOR", "SMST_NO_ALIGN", "SMST_NO_STAGE", "SMST_ALIGN_ALL", "SMST_NO_ACROSS", "SMST_NO_SINGLE_HOP",
            "SMST_NO_FUSE", "SMST_CONTINUOUS")
COUNTERS = ("vocoder_aligned", "vocoder_twisted", "vocoder_interior", "vocoder_staged", "vocoder_gather", "vocoder_n", "vocoder_one", "vocoder_across",
            "vocoder_continuous", "chain_unfused", "analyse_twist", "twist_rows")

DEFAULTS = dict(kind="calls", preset=None, sample_rate=48000, block=512, interval=128, split=False, channels=2, streams=3, stretch=1.5, hops1=9, hops2=(9, 0, 17), in2=None,
                env={}, half_state=False, transpose=None, bands=256, shows=(), never=())
DEFAULT_48K = dict(preset="default", block=None, interval=None, split=None, bands=3072, hops2=(7, 0, 9))
CHEAPER = dict(preset="cheaper", block=None, interval=None, split=False, bands=2560)
ONE_HOP = dict(hops1=1, hops2=(1, 1, 0), in2=3.0)
STEP_6 = dict(block=768, interval=128, bands=384)
FLUSH = dict(kind="flush", split=True, streams=1, lead_hops=16)
CONTINUOUS = dict(block=1920, interval=480, bands=1024, streams=2, hops1=150, hops2=(9, 20), env={"SMST_CONTINUOUS": "1"})
SCENARIOS = {
    # a fresh stream's first hop draws its time factors at random: the gathering producers; the second call's tile is bounded
    "fresh_stereo": dict(shows=("vocoder_gather", "vocoder_aligned"), never=("vocoder_staged", "vocoder_twisted")),
    # presetDefault at 48 kHz: L = 4, the analysis teams exist -- aligned, twisted, interior (hop counts 7 / 9: one whole producer wave)
    "default_48k": dict(DEFAULT_48K, shows=("vocoder_aligned", "vocoder_twisted", "vocoder_interior", "analyse_twist")),
    "default_48k_no_twist": dict(DEFAULT_48K, env={"SMST_VOC_TWIST": "0"}, shows=("vocoder_aligned", "vocoder_interior"), never=("vocoder_twisted", "analyse_twist")),
    "default_48k_no_interior": dict(DEFAULT_48K, env={"SMST_VOC_INTERIOR": "0"}, shows=("vocoder_aligned", "vocoder_twisted"), never=("vocoder_interior",)),
    "default_48k_no_align": dict(DEFAULT_48K, env={"SMST_NO_ALIGN": "1"}, shows=("vocoder_staged",), never=("vocoder_aligned", "vocoder_twisted", "analyse_twist")),
    "default_48k_no_stage": dict(DEFAULT_48K, env={"SMST_NO_STAGE": "1"}, shows=("vocoder_gather",), never=("vocoder_aligned", "vocoder_staged", "vocoder_twisted")),
    # aligned, but no analysis teams for 256 bands: never twisted
    "small_mono": dict(channels=1, shows=("vocoder_aligned", "vocoder_interior"), never=("vocoder_twisted", "analyse_twist")),
    # presetCheaper: L = 3 stays on the staged producers unless SMST_ALIGN_ALL
    "cheaper": dict(CHEAPER, shows=("vocoder_staged",), never=("vocoder_aligned",)),
    "cheaper_align_all": dict(CHEAPER, env={"SMST_ALIGN_ALL": "1"}, shows=("vocoder_aligned",), never=("vocoder_staged",)),
    "fp16_state": dict(half_state=True, shows=("vocoder_staged",), never=("vocoder_aligned",)),
    "fp16_state_mono": dict(half_state=True, channels=1, shows=("vocoder_staged",), never=("vocoder_aligned",)),
    # a frequency map: gathering producers, the hop rotation table beside the rings where the CU's LDS holds both -- stereo: up to 3640 bands
    "transposed_256": dict(transpose=1.25, shows=("vocoder_gather",), never=("vocoder_aligned", "vocoder_staged")),
    "transposed_4096": dict(transpose=1.25, block=8192, interval=2048, bands=4096, hops2=(3, 0, 5), shows=("vocoder_gather",), never=("vocoder_aligned", "vocoder_staged")),
    # one hop per call: lanes across streams; one chain per stream; the wavefront kernel
    "one_hop_mono": dict(ONE_HOP, channels=1, shows=("vocoder_across",), never=("vocoder_one", "vocoder_gather", "vocoder_aligned")),
    "one_hop_stereo": dict(ONE_HOP, shows=("vocoder_across",), never=("vocoder_one", "vocoder_gather", "vocoder_aligned")),
    "one_hop_no_across": dict(ONE_HOP, env={"SMST_NO_ACROSS": "1"}, shows=("vocoder_one",), never=("vocoder_across",)),
    "one_hop_no_across_mono": dict(ONE_HOP, channels=1, env={"SMST_NO_ACROSS": "1"}, shows=("vocoder_one",), never=("vocoder_across",)),
    "one_hop_no_single_hop": dict(ONE_HOP, env={"SMST_NO_SINGLE_HOP": "1"}, never=("vocoder_across", "vocoder_one")),
    # 3-8 channels: kVocoderN, kVocoderOne; more, or SMST_NO_FUSE: records through memory
    "three_channels": dict(channels=3, shows=("vocoder_n",), never=("chain_unfused", "vocoder_gather")),
    "three_channels_one_hop": dict(ONE_HOP, channels=3, shows=("vocoder_one",), never=("vocoder_n", "vocoder_across")),
    "eight_channels_one_hop": dict(ONE_HOP, channels=8, streams=2, hops2=(1, 1), shows=("vocoder_one",), never=("vocoder_n",)),
    "eight_channels": dict(channels=8, streams=2, hops2=(9, 3), shows=("vocoder_n",), never=("chain_unfused",)),
    "nine_channels": dict(channels=9, streams=2, hops2=(9, 3), shows=("chain_unfused",), never=("vocoder_n",)),
    "sixteen_channels": dict(channels=16, streams=2, hops2=(9, 3), shows=("chain_unfused",), never=("vocoder_n",)),
    "three_channels_no_fuse": dict(channels=3, env={"SMST_NO_FUSE": "1"}, shows=("chain_unfused",), never=("vocoder_n",)),
    "mono_no_fuse_one_hop": dict(ONE_HOP, channels=1, env={"SMST_NO_FUSE": "1"}, shows=("chain_unfused",), never=("vocoder_across", "vocoder_one")),
    # a vertical step of 6: fused for mono / stereo (gathering producers only), un-fused from three channels on
    "step_6_mono": dict(STEP_6, channels=1, shows=("vocoder_gather",), never=("vocoder_staged", "vocoder_aligned", "chain_unfused")),
    "step_6_three_channels": dict(STEP_6, channels=3, shows=("chain_unfused",), never=("vocoder_n",)),
    "step_6_mono_one_hop": dict(STEP_6, **ONE_HOP, channels=1, shows=("vocoder_gather",), never=("vocoder_across", "vocoder_one")),
    # a flush() between two chunks of a split block's main prediction (offset 104 of the interval): startBin > 0
    "flush_start_bin": dict(FLUSH, offset=104, shows=("vocoder_one",), never=("vocoder_across",)),
    "flush_start_bin_no_single_hop": dict(FLUSH, offset=104, env={"SMST_NO_SINGLE_HOP": "1"}, shows=("vocoder_gather",), never=("vocoder_across", "vocoder_one")),
    "flush_behind_prediction": dict(FLUSH, offset=121, shows=("vocoder_across",), never=("vocoder_one",)),  # (the prediction is complete: startBin = 0)
    # SMST_CONTINUOUS: the first call's tiles are N C C (the first hop after the reset draws its time factors), the second call's a lone tile
    "continuous": dict(CONTINUOUS, shows=("vocoder_continuous", "vocoder_gather", "vocoder_aligned"), never=("vocoder_twisted",)),
    "continuous_mono": dict(CONTINUOUS, channels=1, shows=("vocoder_continuous", "vocoder_gather", "vocoder_aligned"), never=("vocoder_twisted",)),
    "continuous_off": dict(CONTINUOUS, env={}, shows=("vocoder_gather", "vocoder_aligned"), never=("vocoder_continuous",)),
}
# the CPU stand-in runs a kernel lane by lane: the scenarios with 1024 bands at most, and one of presetDefault
EMU_SCENARIOS = tuple(n for n, s in SCENARIOS.items() if dict(DEFAULTS, **s)["bands"] <= 1024) + ("default_48k",)

# Every recurrence kernel at the smallest and at the largest channel count it is built for: {counter of the kernel: (scenario, scenario)}.  The
# CPU stand-in checks after every launch that the kernel wrote nothing behind the LDS its launcher asked for (tests/emu/hip_emu.cpp), so these
# scenarios pin each kernel's layout type against its carving at both ends.  (kPredictB runs in front of every kChain.)
CHANNEL_LIMITS = {
    "vocoder_gather": ("step_6_mono", "transposed_256"), "vocoder_staged": ("fp16_state_mono", "fp16_state"), "vocoder_aligned": ("small_mono", "fresh_stereo"),
    "vocoder_across": ("one_hop_mono", "one_hop_stereo"), "vocoder_continuous": ("continuous_mono", "continuous"),
    "vocoder_n": ("three_channels", "eight_channels"), "vocoder_one": ("one_hop_no_across_mono", "eight_channels_one_hop"),
    "chain_unfused": ("mono_no_fuse_one_hop", "sixteen_channels"),
}
CHANNEL_RANGE = {"vocoder_gather": (1, 2), "vocoder_staged": (1, 2), "vocoder_aligned": (1, 2), "vocoder_across": (1, 2), "vocoder_continuous": (1, 2),
                 "vocoder_n": (3, 8), "vocoder_one": (1, 8), "chain_unfused": (1, 16)}


def case_channel_limits_are_covered(names):
    """every kernel's two scenarios are among `names`, have the channel counts, and are there to show that kernel"""
    for counter, pair in CHANNEL_LIMITS.items():
        for name, channels in zip(pair, CHANNEL_RANGE[counter]):
            sc = dict(DEFAULTS, **SCENARIOS[name])
            assert name in names and sc["channels"] == channels and counter in sc["shows"], (counter, name)


def _digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _counts(pkg, lib):
    return {k: pkg.launch_count(k, lib) for k in COUNTERS}


def _run_calls(pkg, lib, sc):
    S, C, sr = sc["streams"], sc["channels"], sc["sample_rate"]
    if sc["preset"]:
        b = pkg.StretchBatch(S, C, preset=sc["preset"], sample_rate=sr, split=sc["split"], lib=lib, half_state=sc["half_state"])
    else:
        b = pkg.StretchBatch(S, C, block=sc["block"], interval=sc["interval"], split=bool(sc["split"]), lib=lib, half_state=sc["half_state"])
    assert b.bands() == sc["bands"], (b.bands(), sc["bands"])
    if sc["transpose"]:
        b.setTransposeFactor(sc["transpose"])
    calls = plan(sc, b.intervalSamples())
    n_total = int(sum(n_in.max() for n_in, _ in calls))
    x = np.stack([synth_input(s, C, n_total, sr) for s in range(S)])
    digests, grew = {}, []
    pos = np.zeros(S, np.int64)
    for call, (n_in, n_out) in enumerate(calls):
        before = _counts(pkg, lib)
        xin = np.zeros((S, C, int(n_in.max())), np.float32)
        for s in range(S):
            xin[s, :, :n_in[s]] = x[s, :, pos[s]:pos[s] + n_in[s]]
        pos += n_in
        y = np.array(b.process(xin, n_out.astype(np.int32), in_samples=n_in.astype(np.int32)), copy=True)
        if call == 0 and sc["hops1"] > 4:
            assert float(np.abs(y).max()) > 0.05
        digests["output %d" % call] = _digest(np.concatenate([y[s, :, :n_out[s]].ravel() for s in range(S)]))
        carry = [b.debug_carry(s) for s in range(S)]
        digests["carried sums %d" % call] = _digest(np.concatenate([c[0].ravel() for c in carry]))
        digests["carried products %d" % call] = _digest(np.concatenate([c[1].ravel() for c in carry]))
        after = _counts(pkg, lib)
        grew.append({k: after[k] - before[k] for k in COUNTERS})
    for which, what in enumerate(("input", "previous input", "output", "energy")):
        digests["state: " + what] = _digest(np.concatenate([np.asarray(b.debug_state(s, which)).ravel() for s in range(S)]))
    b.close()
    return digests, grew


def _run_flush(pkg, lib, sc):
    C, I = sc["channels"], sc["interval"]
    x = synth_input(0, C, 12000, sc["sample_rate"])
    g = pkg.SignalsmithStretch(lib=lib)
    g.configure(C, sc["block"], I, split=True)
    n_out = sc["lead_hops"]*I + sc["offset"]
    n_in = int(n_out/1.19)
    digests, grew = {}, []
    steps = (("process", lambda: g.process(x[:, :n_in], n_out)), ("flush", lambda: g.flush(I)), ("process after", lambda: g.process(x[:, 6000:6700], 700)))
    for what, step in steps:
        before = _counts(pkg, lib)
        y = np.array(step(), copy=True)
        digests[what] = _digest(y)
        after = _counts(pkg, lib)
        grew.append({k: after[k] - before[k] for k in COUNTERS})
    assert float(np.abs(y).max()) > 0.05
    g.close()
    return digests, grew


def run_scenario(lib, env, name):
    """-> {"digests": {what: digest}, "counters": [growth per call]} of one scenario; env: anything with setenv / delenv (pytest's monkeypatch)"""
    sc = dict(DEFAULTS, **SCENARIOS[name])
    assert 1 <= sc["streams"] <= 4
    pkg = package()
    for k in SWITCHES:
        env.delenv(k, raising=False)
    env.setenv("SMST_FFT_TEAMS", "2")  # the team kernels even for these small tiles: what a twisted tile's analysis is built on
    for k, val in sc["env"].items():
        env.setenv(k, val)
    try:
        digests, grew = (_run_flush if sc["kind"] == "flush" else _run_calls)(pkg, lib, sc)
    finally:
        for k in SWITCHES:
            env.delenv(k, raising=False)
    total = {k: sum(g[k] for g in grew) for k in COUNTERS}
    print(name, [{k: v for k, v in g.items() if v} for g in grew])
    assert all(total[k] > 0 for k in sc["shows"]) and all(total[k] == 0 for k in sc["never"]), (name, total)
    return {"digests": digests, "counters": grew}


def case_recurrence_form(lib, monkeypatch, name, kind):
    want = json.load(open(GOLDEN[kind]))["scenarios"][name]
    got = run_scenario(lib, monkeypatch, name)
    assert got["counters"] == want["counters"], (name, got["counters"], want["counters"])
    assert sorted(got["digests"]) == sorted(want["digests"])
    differing = [k for k in sorted(got["digests"]) if got["digests"][k] != want["digests"][k]]
    assert not differing, (name, differing)


def case_golden_files_agree_on_the_counters():
    """the decision is the host's: the stand-in's record and the MI355X's hold the same counters for every scenario both ran"""
    gpu, emu = (json.load(open(GOLDEN[kind]))["scenarios"] for kind in ("gpu", "emu"))
    assert sorted(gpu) == sorted(SCENARIOS) and sorted(emu) == sorted(EMU_SCENARIOS)
    for name in emu:
        assert emu[name]["counters"] == gpu[name]["counters"], name


class _Environ:
    def setenv(self, k, v):
        os.environ[k] = v

    def delenv(self, k, raising=False):
        os.environ.pop(k, None)


def record(kind, names, commit):
    import ctypes
    import time
    pkg = package()
    lib = pkg.load_library() if kind == "gpu" else pkg.bind(ctypes.CDLL(os.environ.get("SMST_EMU_LIBRARY") or os.path.join(ROOT, "tests", "emu", "libsmst_emu.so")))
    doc = {"recorded_from": "the commit before csrc/smst_recurrence_form.h (%s), %s" % (commit, "MI355X" if kind == "gpu" else "CPU stand-in"), "scenarios": {}}
    for name in names:
        t0 = time.time()
        doc["scenarios"][name] = run_scenario(lib, _Environ(), name)
        print(name, "recorded, %.1f s" % (time.time() - t0), flush=True)
    return doc


if __name__ == "__main__":
    import sys
    kind, dest = sys.argv[2], sys.argv[3]
    doc = record(kind, sys.argv[4:] or list(SCENARIOS if kind == "gpu" else EMU_SCENARIOS), os.environ.get("SMST_RECORDED_COMMIT", "e96c4fb"))
    with open(dest, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
