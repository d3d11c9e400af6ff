"""The per-call table of the _pcm calls -- [in counts][out counts][dither entries][level entries][loudness entries][channel weights]
(csrc/smst_pcm_tables.h) -- pinned against the commit before the table got its one definition: shared by the CPU stand-in and the GPU test.

Which sections a call uploads is decided by three things: whether it dithers, whether the batch is levelled, whether a stream is in the
loudness mode (and whether the output counts ride in front).  ONE small batch (3 streams, stereo, block 256 / interval 64) walks COMBOS:
  plain               no dither, not levelled: only the counts travel;
  dither              TPDF on stream 0, TPDF_HP on stream 2, none on 1;
  fixed+dither        LEVEL_FIXED gains on every stream (the batch is a levelled one from here on), the dither as before;
  fixed               ... and the dither off again: the entries still travel, `dither` is null;
  protect/normalise   PROTECT on stream 0, NORMALISE on stream 2, FIXED on 1, the dither on again;
  loudness            LOUDNESS on stream 1 (sample rate 2560: its 100-ms step is the 256 frames of SMST_LOUDNESS_CHUNK, the smallest the
                      library accepts, so a 400-ms block is 1024 frames), FIXED on the others, channel weights 1 and 0.7.
Every combination runs in int16, packed int24 and float32 frames (float32 has no step to dither: the entries travel, `dither` is null).  The
streaming combinations go through process then flush (one stream with a count of 0, one left out of the flush by a negative count); every
combination through two exact calls back to back, nothing read between them, so both table sets are in use: ragged clips of 1500-3000
frames, one stream too short for its outputSeekLength, one left out by a negative count.

After every step: SHA-256 digests of the output bytes, of take_pcm_overs, take_pcm_peaks, take_pcm_loudness and of pcm_dither()'s frame
counters.  They are compared, for equality, with what the parent commit gave, kept under tests/golden/ (pcm_tables_parent_gpu.json: recorded
on an MI355X, host and device memory; pcm_tables_parent_emu.json: from the CPU stand-in on host memory).  Two recordings of the GPU file at
the parent were identical in every quantity -- the loudness passes sum in one fixed order and use no floating-point atomic -- so nothing is
compared within a tolerance.

The calls go through a small adapter (ApiCalls: the public Python API), so that tests/test_stream_order_emu.py can drive the same sequence
through the C ABI on device memory under the deferred schedules.

`python tests/pcm_tables_cases.py record gpu|emu <file>` writes the digests of the library it runs on."""
import hashlib
import json
import os

import numpy as np

from conftest import ROOT, package, synth_input

GOLDEN = {kind: os.path.join(ROOT, "tests", "golden", "pcm_tables_parent_%s.json" % kind) for kind in ("gpu", "emu")}
S, CHANNELS = 3, 2
GEOMETRY = dict(block=256, interval=64)
LOUDNESS_RATE = 2560.0
FORMATS = ("s16", "s24", "f32")
N_INPUT = 12000

# (name, setters before the combination's calls, whether the streaming calls run).  Modes as include/smst.h numbers them: dither 0 none,
# 1 TPDF, 2 TPDF_HP; level 0 FIXED, 1 PROTECT, 2 NORMALISE
COMBOS = (
    ("plain", (), True),
    ("dither", (("setPcmDither", (1, 11), dict(stream=0)), ("setPcmDither", (2, 12), dict(stream=2))), True),
    ("fixed+dither", (("set_pcm_level", (0, 2.5, 1.0), dict(stream=0)), ("set_pcm_level", (0, 0.5, 1.0), dict(stream=1)),
                      ("set_pcm_level", (0, 1.0, 1.0), dict(stream=2))), True),
    ("fixed", (("setPcmDither", (0,), dict()),), True),
    ("protect/normalise", (("setPcmDither", (1, 21), dict(stream=0)), ("setPcmDither", (2, 22), dict(stream=2)),
                           ("set_pcm_level", (1, 3.0, 0.8), dict(stream=0)), ("set_pcm_level", (2, 1.0, 0.5), dict(stream=2))), False),
    ("loudness", (("set_pcm_level", (0, 1.5, 1.0), dict(stream=0)), ("set_pcm_level", (0, 0.75, 1.0), dict(stream=2)),
                  ("set_pcm_loudness", (-20.0, 0.9, LOUDNESS_RATE), dict(stream=1)), ("set_pcm_loudness_weights", ([1.0, 0.7],), dict())), False),
)
PROCESS = ([700, 0, 513], [640, 300, 450])                                  # (in, out)
FLUSH = ([200, -1, 64], [1.0, 0.0, 1.25])                                   # (counts, rates)
EXACT = (([2500, 3000, 1800], [3000, 2400, 2000]),                          # (in, out): every stream runs
         ([100, 2800, 2000], [150, 1500, -1]))                              # stream 0 too short, stream 2 left out
EXACT_RUNS = ([True, True, True], [False, True, False])


def inputs():
    """[S, C, N_INPUT] float32"""
    return np.stack([synth_input(s, CHANNELS, N_INPUT, 48000) + 0.3*synth_input(s + 4, CHANNELS, N_INPUT, 48000) for s in range(S)]).astype(np.float32)


def frames_of(planar, fmt):
    """[S, C, n] float32 -> frames [S, n, C] of the format (packed int24: uint8 [S, n, C, 3], little-endian)"""
    v = np.ascontiguousarray(np.transpose(planar, (0, 2, 1)))
    if fmt == "f32":
        return v
    if fmt == "s16":
        return np.clip(np.round(v*32768.0), -32768, 32767).astype(np.int16)
    codes = np.clip(np.round(v.astype(np.float64)*8388608.0), -8388608, 8388607).astype("<i4")
    return np.ascontiguousarray(codes.view(np.uint8).reshape(codes.shape + (4,))[..., :3])


def _digest(parts):
    h = hashlib.sha256()
    for a in parts:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


class ApiCalls:
    """The frame calls through StretchBatch.  to_memory / to_host move a numpy array into the memory under test and back (the default: host
    memory; torch tensors: device memory)."""

    def __init__(self, batch, to_memory=lambda a: a, to_host=lambda a: np.array(a, copy=True)):
        self.b, self.to_memory, self.host = batch, to_memory, to_host
        self.like = to_memory(np.zeros(1, np.float32))

    def process(self, x, nin, nout):
        return self.b.processFrames(self.to_memory(x), nout, in_samples=nin)

    def flush(self, counts, rates, fmt):
        return self.b.flushFrames(counts, rates, like=self.like, dtype={"s16": np.int16, "s24": "s24", "f32": np.float32}[fmt])

    def exact(self, x, nin, nout):
        """-> (out, ok): out is read with host() once both calls of the step have been issued"""
        return self.b.exactFrames(self.to_memory(x), nout, in_samples=nin)


def _meters(batch):
    """what the takes and the getters give after a step, as digests"""
    lufs, blocks, gated = batch.take_pcm_loudness()
    return {"overs": _digest(batch.takePcmOvers()), "peaks": _digest(batch.take_pcm_peaks()), "loudness": _digest([lufs, blocks, gated]),
            "dither frames": _digest([np.asarray([batch.pcmDither(s)[2] for s in range(S)], np.int64)])}


def run_sequence(batch, calls, x=None):
    """COMBOS on `batch` through `calls` -> {"combination format step: quantity": digest}"""
    x = inputs() if x is None else x
    digests, pos = {}, 0

    def cut(counts, fmt):
        nonlocal pos
        clip = frames_of(x[:, :, pos:pos + max(max(counts), 1)], fmt)
        pos = (pos + 997) % (N_INPUT - 3000)
        return clip

    def note(name, out):
        digests[name + ": output"] = _digest(out)
        for what, d in _meters(batch).items():
            digests[name + ": " + what] = d

    for combo, setters, streaming in COMBOS:
        for setter, args, kwargs in setters:
            getattr(batch, setter)(*args, **kwargs)
        for fmt in FORMATS:
            name = "%s %s " % (combo, fmt)
            if streaming:
                y = calls.host(calls.process(cut(PROCESS[0], fmt), *PROCESS))
                note(name + "process", [y[s, :n] for s, n in enumerate(PROCESS[1])])
                y = calls.host(calls.flush(FLUSH[0], FLUSH[1], fmt))
                note(name + "flush", [y[s, :max(n, 0)] for s, n in enumerate(FLUSH[0])])
            issued = [calls.exact(cut(nin, fmt), nin, nout) for nin, nout in EXACT]            # back to back: nothing is read in between
            out = []
            for (nin, nout), runs, (y, ok) in zip(EXACT, EXACT_RUNS, issued):
                y = calls.host(y)
                assert np.asarray(ok).tolist() == runs, (name, np.asarray(ok).tolist(), runs)
                for s, n in enumerate(nout):
                    if n >= 0:
                        assert (nin[s] >= batch.outputSeekLength(nin[s]/n)) == runs[s], (name, s)
                        assert bool(np.any(y[s, :n])) == runs[s], (name, s)                     # zeros for the short one, sound for the others
                        out.append(y[s, :n])
            note(name + "exact", out)
    return digests


def new_batch(lib):
    return package().StretchBatch(S, CHANNELS, seed=7, lib=lib, **GEOMETRY)


def run_memory(lib, **memory):
    b = new_batch(lib)
    digests = run_sequence(b, ApiCalls(b, **memory))
    b.close()
    return digests


def case_pcm_tables(lib, kind, where, **memory):
    want = json.load(open(GOLDEN[kind]))["memory"][where]
    got = run_memory(lib, **memory)
    assert sorted(got) == sorted(want)
    differing = [k for k in sorted(got) if got[k] != want[k]]
    assert not differing, (where, differing)


def device_memory():
    import torch
    return dict(to_memory=lambda a: torch.from_numpy(a).cuda(), to_host=lambda t: t.cpu().numpy())


def record(kind, commit):
    import ctypes
    pkg = package()
    if kind == "gpu":
        lib = pkg.load_library()
        memories = {"host": {}, "device": device_memory()}
    else:
        lib = pkg.bind(ctypes.CDLL(os.environ.get("SMST_EMU_LIBRARY") or os.path.join(ROOT, "tests", "emu", "libsmst_emu.so")))
        memories = {"host": {}}
    where = "MI355X" if kind == "gpu" else "CPU stand-in"
    doc = {"recorded_from": "the commit before csrc/smst_pcm_tables.h (%s), %s" % (commit, where), "memory": {}}
    for name, memory in memories.items():
        doc["memory"][name] = run_memory(lib, **memory)
        print(name, "recorded", flush=True)
    return doc


if __name__ == "__main__":
    import sys
    doc = record(sys.argv[2], os.environ.get("SMST_RECORDED_COMMIT", "8078ab3"))
    with open(sys.argv[3], "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
