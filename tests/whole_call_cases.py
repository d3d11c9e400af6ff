"""The whole-call stages of the engine -- seek, flush, outputSeek, the resets under them and exact(), which chains all of them -- pinned against
the commit before their per-stream tables moved into rotating pinned sets (csrc/smst_staging.h): shared by the CPU stand-in and the GPU test.

A scenario is ONE small batch (5 streams, stereo, block 512 / interval 128, with and without split computation) driven through SEQUENCE:
  1. seek with ragged lengths, one of them 0;
  2. process, ragged;
  3. two seeks back to back with different lengths, then process;
  4. flush with a count above the interval (a block runs through the zeros), two at most the interval, a 0 and a negative one (left out);
  5. outputSeek with input lengths on both sides of the input latency (the pre-roll process runs once per group), then process;
  6. three exact() calls back to back, nothing read and nothing synchronised between them: ragged lengths and rates, one stream too short for
     its outputSeekLength, one left out by a negative count -- planar fp32, int16 frames with a stream in LEVEL_PROTECT, planar fp32;
with setters between the calls.  After every step: SHA-256 digests of the step's output, of debug_carry and of debug_state 0..3 of every
stream (the three exact calls are one step).  The digests are compared, for equality, with what the parent commit gave, kept under
tests/golden/ (whole_call_parent_gpu.json: recorded on an MI355X on device memory; whole_call_parent_emu.json: from the CPU stand-in on host
memory).

The calls go through a small adapter (ApiCalls: the public Python API), so that tests/test_stream_order_emu.py can drive the same sequence
through the C ABI on device memory under the deferred schedules.

`python tests/whole_call_cases.py record gpu|emu <file>` writes the digests of the library it runs on."""
import hashlib
import json
import os

import numpy as np

from conftest import ROOT, package, synth_input

GOLDEN = {kind: os.path.join(ROOT, "tests", "golden", "whole_call_parent_%s.json" % kind) for kind in ("gpu", "emu")}
S, CHANNELS, INTERVAL = 5, 2, 128
GEOMETRY = dict(block=512, interval=INTERVAL)
SCENARIOS = {"plain": False, "split": True}

# (what, argument ...): positions are offsets into inputs(); every count list is per stream
SEQUENCE = (
    ("set", "setTransposeSemitones", (3, 0), dict(stream=1)),
    ("seek", 0, [640, 333, 0, 500, 129], [1.0, 0.8, 1.25, 1.0, 0.5]),
    ("process", 640, [900, 700, 0, 1024, 513], [1100, 640, 300, 1024, 400]),                        # (position, in, out)
    ("set", "setFormantFactor", (1.3, True), dict(stream=2)),                                        # split: between the steps of blocks in flight
    ("seek", 2000, [640, 200, 640, 0, 640], [1.25, 1.0, 1.0, 1.0, 0.8]),
    ("seek", 3000, [500, 640, 64, 300, 0], [0.8, 1.1, 1.0, 2.0, 1.0]),
    ("process", 3640, [700, 650, 300, 129, 1000], [700, 600, 350, 128, 900]),
    ("flush", [300, 100, 0, -1, INTERVAL], [1.0, 0.8, 0.0, 0.0, 1.25]),
    ("set", "setFormantBase", (200/48000,), dict(stream=2)),
    ("outputSeek", 5000, [2000, 200, 2000, 1500, 200]),                                             # input latency 256: seeks of 256 and of 200 samples
    ("process", 7000, [800, 640, 512, 900, 100], [800, 700, 500, 1000, 128]),
    ("set", "set_pcm_level", (1, 1.5, 0.9), dict(stream=0)),                                         # 1: LEVEL_PROTECT -- the clip's peak decides the gain
    ("exact", ((8000, [3000, 4000, 200, 2500, 3500], [3600, 3000, 300, -1, 2800], False),            # (position, in, out, frames)
               (9000, [2500, 3000, 3100, 150, 2000], [2000, 3300, -1, 200, 2600], True),
               (10000, [2000, 2200, 2400, 2600, 100], [2600, -1, 2000, 2400, 150], False)),
              ([True, True, False, False, True], [True, True, False, False, True], [True, False, True, True, False])),   # which streams run
)
N_INPUT = 14000


def inputs():
    """[S, C, N_INPUT] float32"""
    return np.stack([synth_input(s, CHANNELS, N_INPUT, 48000) + 0.3*synth_input(s + 4, CHANNELS, N_INPUT, 48000) for s in range(S)]).astype(np.float32)


def frames_s16(planar):
    """[S, C, n] float32 -> int16 frames [S, n, C]"""
    return np.ascontiguousarray(np.clip(np.round(np.transpose(planar, (0, 2, 1))*32768.0), -32768, 32767).astype(np.int16))


def _digest(parts):
    h = hashlib.sha256()
    for a in parts:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


class ApiCalls:
    """The calls of SEQUENCE through StretchBatch.  to_memory / to_host move a numpy array into the memory under test and back (the default:
    host memory; torch tensors: device memory, and then nothing between two calls waits for the device)."""

    def __init__(self, batch, to_memory=lambda a: a, to_host=lambda a: np.array(a, copy=True)):
        self.b, self.to_memory, self.host = batch, to_memory, to_host
        self.like = to_memory(np.zeros(1, np.float32))

    def seek(self, x, counts, rates):
        self.b.seek(self.to_memory(x), rates, in_samples=counts)

    def process(self, x, nin, nout):
        return self.b.process(self.to_memory(x), nout, in_samples=nin)

    def flush(self, counts, rates):
        return self.b.flush(counts, rates, like=self.like)

    def output_seek(self, x, lengths):
        self.b.outputSeek(self.to_memory(x), lengths)

    def exact(self, x, nin, nout, frames):
        """-> (out, ok): out is read with host() once every call of the step has been issued"""
        return (self.b.exactFrames if frames else self.b.exact)(self.to_memory(x), nout, in_samples=nin)


def run_sequence(batch, calls, x=None, rounds=1, between=None):
    """SEQUENCE on `batch` through `calls` -> {"NN what: output | carry | state": digest} of the LAST round; between(what): called around
    every call of a step (the stream-order test's counters)"""
    x = inputs() if x is None else x
    cut = lambda pos, counts: np.ascontiguousarray(x[:, :, pos:pos + max(max(counts), 1)])
    digests = {}
    for _ in range(rounds):
        digests = {}
        for k, step in enumerate(SEQUENCE):
            what, out = step[0], []
            if what == "set":
                getattr(batch, step[1])(*step[2], **step[3])
                continue
            if what == "seek":
                calls.seek(cut(step[1], step[2]), step[2], step[3])
            elif what == "process":
                y = calls.host(calls.process(cut(step[1], step[2]), step[2], step[3]))
                out = [y[s, :, :n] for s, n in enumerate(step[3])]
            elif what == "flush":
                y = calls.host(calls.flush(step[1], step[2]))
                out = [y[s, :, :max(n, 0)] for s, n in enumerate(step[1])]
            elif what == "outputSeek":
                calls.output_seek(cut(step[1], step[2]), step[2])
            elif what == "exact":
                issued = []
                for pos, nin, nout, frames in step[1]:                       # back to back: nothing is read before the last one is issued
                    clip = cut(pos, nin)
                    issued.append(calls.exact(frames_s16(clip) if frames else clip, nin, nout, frames))
                for (pos, nin, nout, frames), runs, (y, ok) in zip(step[1], step[2], issued):
                    y = calls.host(y)
                    assert np.asarray(ok).tolist() == runs, (pos, np.asarray(ok).tolist(), runs)
                    for s, n in enumerate(nout):
                        if n >= 0:
                            assert bool(np.any(y[s, :n] if frames else y[s, :, :n])) == runs[s], (pos, s)   # zeros for the short one, sound for the others
                            out.append(y[s, :n] if frames else y[s, :, :n])
                out += list(batch.take_pcm_peaks())
            name = "%02d %s: " % (k, what)
            if out:
                digests[name + "output"] = _digest(out)
            carry = [batch.debug_carry(s) for s in range(S)]
            digests[name + "carry"] = _digest([a for c in carry for a in c])
            digests[name + "state"] = _digest([batch.debug_state(s, which) for s in range(S) for which in range(4)])
    return digests


def new_batch(lib, split):
    return package().StretchBatch(S, CHANNELS, split=split, seed=7, lib=lib, **GEOMETRY)


def run_scenario(lib, name, **memory):
    b = new_batch(lib, SCENARIOS[name])
    digests = run_sequence(b, ApiCalls(b, **memory))
    b.close()
    return digests


def case_whole_call(lib, name, kind, **memory):
    want = json.load(open(GOLDEN[kind]))["scenarios"][name]
    got = run_scenario(lib, name, **memory)
    assert sorted(got) == sorted(want)
    differing = [k for k in sorted(got) if got[k] != want[k]]
    assert not differing, (name, differing)


def case_steady_state(lib, name, **memory):
    """the whole sequence a second and a third time moves neither allocation_events() nor workspaceBytes()"""
    b = new_batch(lib, SCENARIOS[name])
    calls, x = ApiCalls(b, **memory), inputs()
    run_sequence(b, calls, x)
    events, workspace = b.allocation_events(), b.workspaceBytes()
    run_sequence(b, calls, x, rounds=2)
    assert (b.allocation_events(), b.workspaceBytes()) == (events, workspace)
    b.close()


def record(kind, commit):
    import ctypes
    pkg = package()
    memory = {}
    if kind == "gpu":
        import torch
        lib = pkg.load_library()
        memory = dict(to_memory=lambda a: torch.from_numpy(a).cuda(), to_host=lambda t: t.cpu().numpy())
    else:
        lib = pkg.bind(ctypes.CDLL(os.environ.get("SMST_EMU_LIBRARY") or os.path.join(ROOT, "tests", "emu", "libsmst_emu.so")))
    where = "MI355X, device memory" if kind == "gpu" else "CPU stand-in, host memory"
    doc = {"recorded_from": "the commit before csrc/smst_staging.h (%s), %s" % (commit, where), "scenarios": {}}
    for name in SCENARIOS:
        doc["scenarios"][name] = run_scenario(lib, name, **memory)
        print(name, "recorded", flush=True)
    return doc


if __name__ == "__main__":
    import sys
    doc = record(sys.argv[2], os.environ.get("SMST_RECORDED_COMMIT", "8c99aaa"))
    with open(sys.argv[3], "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
