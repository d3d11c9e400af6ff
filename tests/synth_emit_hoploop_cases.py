"""kSynthEmitTeams' hop loop against kSynthTeams + kEmit (SMST_SYNTH_EMIT=0), at the edges of a tile: shared by the CPU stand-in and the GPU test.

The fused kernel's hop loop carries only what every hop needs; what only the edges of a tile need (a stream without hops, the samples in
front of a tile's first hop, the call's last interval, split computation's trailing interval, the carry write) runs in front of the loop
and behind it, and the presets' geometries are compile-time facts of their instantiations.  A case therefore runs ONE batch of streams
whose hop counts within a tile are 0, 1, 2, NI - 1, NI, NI + 1, 9 and 64 (NI = ceil(block/interval) + 1 intervals of ring: the first NI
intervals of a tile take their window products from memory), through both forms, and asserts that every call's output and the carried
sums and window products after every call are byte-identical -- and, by the launch counters, that the first run really went through
the fused kernel and the second did not.

The batch is 64 (stream, channel) pairs, the launcher's own threshold (SMST_SYNTH_EMIT stays at its default): one team per pair.

Calls (hop counts are driven by the per-stream output lengths; a stream with no output and no input sits a call out):
  1  the first call after a reset: every stream's first hop begins at sample 0.  The longest stream fires 70 hops: tile 1 (6 hops, below the
     launcher's 8: two kernels) starts from the carry the fused kernel wrote for tile 0
  2  every stream that has fired begins its first hop INSIDE the call (samples in front of the tile's first hop; a stream without a hop emits
     carried samples only); the longest stream fires 73 hops, so tile 1 (9 hops) is a fused tile that starts from a fused tile's carry
  3  as 2 with 9 hops at the most, the hop counts dealt to other streams
  then flush().
The streams come in four groups that differ in where a call's output ends relative to its last hop's interval: exactly at its end; one
sample in front of it; one sample behind its BEGINNING (without split computation: one final sample in the last interval; with it: the
tile ends one sample behind its last complete interval, so the trailing interval is a single sample); somewhere inside."""
import numpy as np

from conftest import package, synth_input

GROUPS = 4


def hop_pattern(NI, longest):
    return (0, 1, 2, NI - 1, NI, NI + 1, 9, longest)


class _Schedule:
    """the reference's block scheduler, as far as the output positions of the hops go (signalsmith-stretch.h:280-319)"""

    def __init__(self, streams, interval):
        self.I = interval
        self.since = [None]*streams  # samples since the stream's last hop began; None: it has not fired since the reset

    def first(self, s):
        return 0 if self.since[s] is None or self.since[s] >= self.I else self.I - self.since[s]

    def call(self, s, n_out):
        first, I = self.first(s), self.I
        hops = (n_out - first + I - 1)//I if n_out > first else 0
        if hops:
            self.since[s] = n_out - (first + (hops - 1)*I)
        elif self.since[s] is not None:
            self.since[s] += n_out
        return hops


def plan_calls(streams, interval, NI):
    """-> [(n_out[streams], hops[streams])] for the three calls"""
    sched = _Schedule(streams, interval)
    I = interval
    calls = []
    for call, longest in enumerate((70, 73, 9)):
        pattern = hop_pattern(NI, longest)
        n_out, hops = np.zeros(streams, np.int64), np.zeros(streams, np.int64)
        for s in range(streams):
            group = s//8 % GROUPS
            # the full pattern in ONE group per call (another one each call); in the other groups the two longest streams fire 1 and 2 hops
            h = pattern[(s + 3*call) % 8]
            if group != call % GROUPS and h in (9, longest):
                h = 1 if h == 9 else 2
            first = sched.first(s)
            if h == 0:
                n = min(first, 37)  # carried samples only -- none where the stream's next hop is due at once
            else:
                end = first + h*I  # where the last hop's interval ends
                n = (end, end - 1, end - I + 1, end - I//2 + 3)[group]
            n_out[s] = n
            hops[s] = sched.call(s, n)
            assert hops[s] == h, (call, s, h, int(hops[s]))
        calls.append((n_out, hops))
    return calls


def case_hoploop(lib, monkeypatch, streams=32, channels=2, preset="default", sample_rate=48000, split=False, half_state=False):
    pkg = package()
    names = ("synth_emit", "synth_teams", "synth_fast")
    runs = []
    for fused in (True, False):
        if fused:
            monkeypatch.delenv("SMST_SYNTH_EMIT", raising=False)
        else:
            monkeypatch.setenv("SMST_SYNTH_EMIT", "0")
        before = [pkg.launch_count(k, lib) for k in names]
        b = pkg.StretchBatch(streams, channels, preset=preset, sample_rate=sample_rate, split=split, lib=lib, half_state=half_state)
        B, I = b.blockSamples(), b.intervalSamples()
        NI = -(-B//I) + 1
        calls = plan_calls(streams, I, NI)
        if fused:
            assert sorted(set(int(h) for h in calls[0][1])) == sorted(set(hop_pattern(NI, 70)))
            assert max(calls[1][1]) == 73 and max(calls[2][1]) == 9
        n_max = max(int(n.max()) for n, _ in calls)
        x = np.stack([synth_input(s, channels, n_max, 48000) for s in range(streams)])
        got = []
        pos = np.zeros(streams, np.int64)
        for n_out, _ in calls:
            n_in = np.where(n_out > 0, np.maximum(n_out*4//5, 1), 0).astype(np.int32)  # 1.25x
            xin = np.zeros((streams, channels, max(int(n_in.max()), 1)), np.float32)
            for s in range(streams):
                seg = x[s, :, pos[s] % n_max:][:, :n_in[s]]
                xin[s, :, :seg.shape[1]] = seg
            pos += n_in
            y = np.array(b.process(xin, n_out.astype(np.int32), in_samples=n_in), copy=True)
            got.append([y[s, :, :n_out[s]].copy() for s in range(streams)])
            got.append([b.debug_carry(s) for s in range(streams)])
        got.append(np.array(b.flush(b.outputLatency() + 100), copy=True))
        b.close()
        grew = [pkg.launch_count(k, lib) - c for k, c in zip(names, before)]
        # fused: tile 0 of every call and tile 1 of call 2 (tile 1 of call 1 takes two kernels in this run too); with split computation a call's
        # first tile begins with the block in flight from the call before and takes two kernels: tile 0 of call 1 and tile 1 of call 2 are left
        if fused:
            assert grew[0] >= (2 if split else 4), grew
        else:
            assert grew[0] == 0 and grew[1] + grew[2] > 0, (fused, grew)
        runs.append(got)
    monkeypatch.delenv("SMST_SYNTH_EMIT", raising=False)
    a, r = runs
    assert max(float(np.abs(y).max()) for y in a[0] if y.size) > 0.05
    for step in range(0, 6, 2):
        for s in range(streams):
            assert a[step][s].tobytes() == r[step][s].tobytes(), ("output", step//2, s)
            for which in (0, 1):
                assert a[step + 1][s][which].tobytes() == r[step + 1][s][which].tobytes(), ("carried sums" if which == 0 else "carried products", step//2, s)
    assert a[6].tobytes() == r[6].tobytes(), "flush"


# (name, arguments): every instantiation of the fused kernel with a compile-time geometry, the one that reads the geometry from the batch,
# mono, the fp16 carry, split computation
CASES = {
    "default_48k": dict(preset="default", sample_rate=48000),
    "default_44k1": dict(preset="default", sample_rate=44100),
    "cheaper_48k": dict(preset="cheaper", sample_rate=48000),
    "cheaper_44k1": dict(preset="cheaper", sample_rate=44100),
    "runtime_geometry": dict(preset="default", sample_rate=46000),   # block 5520, interval 1380: 3072 bands as at 48 kHz, no instantiation of its own
    "mono_64": dict(preset="default", sample_rate=48000, streams=64, channels=1),
    "half_state": dict(preset="cheaper", sample_rate=44100, half_state=True),
    "split": dict(preset="default", sample_rate=48000, split=True),
}
# the CPU stand-in runs a kernel lane by lane (half a minute per case): the index logic of a full-slot geometry, of one whose last slot is
# partial and whose frames end inside an interval (with the fp16 carry), of the run-time geometry, and of split computation
EMU_CASES = ("default_48k", "half_state", "runtime_geometry", "split")
