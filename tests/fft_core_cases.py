"""The FFT kernels' transform core (csrc/smst_fft_complex.h): shared by the CPU stand-in and the GPU tests.

1. case_fft_complex_helpers: every helper of the header on 4096 operand tuples against its documented formula in float32.

2. case_bit_identity: the change that introduced the header moved no rounding, so every path through the transforms computes what the
   commit before it computed, byte for byte.  That commit's helpers are gone, so its results are kept as SHA-256 digests under
   tests/golden/ (fft_core_parent_gpu.json: recorded on an MI355X; fft_core_parent_emu.json: from the CPU stand-in) -- of each call's output,
   of the carried sums and window products after each call, and of the carried per-bin state at the end.  A case is one batch, a first
   call of 9 hops per stream and a second, ragged call (another length per stream, some streams without a hop); the switches of the case
   select the kernels, and the launch counters say that the intended ones ran.

   `python tests/fft_core_cases.py record gpu|emu` writes the digests of the library it runs on (the commit whose results are to be kept)."""
import hashlib
import json
import os

import numpy as np

from conftest import ROOT, package, synth_input

GOLDEN = {kind: os.path.join(ROOT, "tests", "golden", "fft_core_parent_%s.json" % kind) for kind in ("gpu", "emu")}


# ------------------------------------------------------------------------------------------------------
# helper formulas
# ------------------------------------------------------------------------------------------------------
def fft_complex_operands():
    g = np.random.Generator(np.random.PCG64(77))
    v = g.standard_normal((4096, 4)).astype(np.float32)
    v[:16] = 0.0
    return v


def fft_complex_expectation(v, fused):
    """The roundings csrc/smst_fft_complex.h documents, in float32.  fused: the device's single-rounded multiply-adds (float64 products of
    float32 operands are exact, one rounding on the way back); not fused: every product rounded, as the CPU stand-in's twin computes."""
    f32, f64 = np.float32, np.float64
    ax, ay, bx, by = (v[:, i].astype(f32) for i in range(4))

    def mul(x, y):
        return (x.astype(f64)*y.astype(f64)).astype(f32)

    def fma(x, y, z):
        if not fused:
            return (mul(x, y) + z).astype(f32)
        return (x.astype(f64)*y.astype(f64) + z.astype(f64)).astype(f32)
    out = np.zeros((v.shape[0], 20), f32)
    out[:, 0], out[:, 1] = fma(ax, bx, -mul(ay, by)), fma(ax, by, mul(ay, bx))      # fmul<false>(a, b)   = a*b
    out[:, 2], out[:, 3] = fma(ax, bx, mul(ay, by)), fma(ax, -by, mul(ay, bx))      # fmul<true>(a, b)    = a*conj(b)
    out[:, 4], out[:, 5] = fma(bx, ax, mul(by, ay)), fma(bx, ay, -mul(by, ax))      # fmulc(a, b)         = a*conj(b), b's terms first
    out[:, 6], out[:, 7] = ax - by, ay + bx                                        # faddI(a, b)         = a + i b
    out[:, 8], out[:, 9] = ax + by, ay - bx                                        # fsubI(a, b)         = a - i b
    out[:, 10], out[:, 11] = ax + bx, ay + by                                      # fadd
    out[:, 12], out[:, 13] = ax - bx, ay - by                                      # fsub
    out[:, 14], out[:, 15] = ax, -ay                                               # fconjStore(a, true)
    out[:, 16], out[:, 17] = ax, -ay                                               # fconjLoad(a, true)
    out[:, 18], out[:, 19] = ax, ay                                                # fconjLoad / fconjStore(a, false)
    return out


def fft_complex_exact(v):
    """the fused formulas with every fused multiply-add rounded ONCE, from exact rational arithmetic (slow: the CPU check of the expectation)"""
    from fractions import Fraction
    f32 = np.float32

    def rnd(q):  # a rational to the nearest float32, ties to even: through an integer quotient, not through float64
        if q == 0:
            return f32(0.0)
        sign, q = (-1 if q < 0 else 1), abs(q)
        e = q.numerator.bit_length() - q.denominator.bit_length()
        if Fraction(2)**e > q:
            e -= 1
        e = max(e, -126)                       # subnormals share the smallest exponent
        scaled = q/Fraction(2)**(e - 23)       # the significand as a rational in [2^23, 2^24)
        n = scaled.numerator//scaled.denominator
        rest = scaled - n
        if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and n % 2):
            n += 1
        return f32(sign*float(n)*2.0**(e - 23))
    want = fft_complex_expectation(v, True).copy()
    F = [[Fraction(float(x)) for x in row] for row in v]
    for i, (ax, ay, bx, by) in enumerate(F):
        yy, yx = Fraction(float(rnd(ay*by))), Fraction(float(rnd(ay*bx)))
        want[i, 0], want[i, 1] = rnd(ax*bx - yy), rnd(ax*by + yx)
        want[i, 2], want[i, 3] = rnd(ax*bx + yy), rnd(-ax*by + yx)
        want[i, 4], want[i, 5] = rnd(bx*ax + yy), rnd(bx*ay - Fraction(float(rnd(by*ax))))
    return want


def case_fft_complex_helpers(lib, fused):
    v = fft_complex_operands()
    got = package().fft_complex_selftest(v, lib=lib)
    want = fft_complex_expectation(v, fused)
    # the float64 emulation of a float32 fma double-rounds in rare cases: an ulp there, exact agreement on the rest
    close = np.abs(got - want) <= np.spacing(np.abs(want).astype(np.float32))
    assert close.all(), (got[~close][:4], want[~close][:4])
    assert (got == want).mean() >= 0.999, float((got == want).mean())
    assert np.array_equal(np.signbit(got[:16]), np.signbit(want[:16])), "signs of zero"


# ------------------------------------------------------------------------------------------------------
# bit-identity against the commit before the header
# ------------------------------------------------------------------------------------------------------
TEAMS_EMIT = dict(env={"SMST_FFT_TEAMS": "2"}, ran=("analyse_teams", "synth_emit"), idle=("synth_fast", "analyse_generic", "synth_generic"))  # (the ragged call's tile is below the fused kernel's 8 hops: kSynthTeams + kEmit)
TEAMS_TWO = dict(env={"SMST_FFT_TEAMS": "2", "SMST_SYNTH_EMIT": "0"}, ran=("analyse_teams", "synth_teams"), idle=("synth_emit", "synth_fast", "analyse_generic", "synth_generic"))
FAST = dict(env={"SMST_FFT_TEAMS": "0"}, ran=("analyse_fast", "synth_fast"), idle=("analyse_teams", "synth_teams", "synth_emit", "analyse_generic", "synth_generic"))
GENERIC = dict(env={"SMST_NO_FAST_FFT": "1"}, ran=("analyse_generic", "synth_generic"), idle=("analyse_teams", "analyse_fast", "synth_teams", "synth_fast", "synth_emit"))
CASES = {
    "teams_emit_default_48k": dict(TEAMS_EMIT, preset="default", sample_rate=48000, streams=32),
    "teams_emit_cheaper_48k": dict(TEAMS_EMIT, preset="cheaper", sample_rate=48000, streams=32),
    "teams_default_48k": dict(TEAMS_TWO, preset="default", sample_rate=48000, streams=32),
    "teams_cheaper_48k": dict(TEAMS_TWO, preset="cheaper", sample_rate=48000, streams=32),
    "fast_default_48k": dict(FAST, preset="default", sample_rate=48000, streams=32),
    "fast_cheaper_48k": dict(FAST, preset="cheaper", sample_rate=48000, streams=32),
    "fast_default_96k": dict(FAST, preset="default", sample_rate=96000, streams=2),   # R3 = 24
    "fast_cheaper_96k": dict(FAST, preset="cheaper", sample_rate=96000, streams=2),   # R3 = 20
    "generic_default_48k": dict(GENERIC, preset="default", sample_rate=48000, streams=2),
}
SWITCHES = ("SMST_FFT_TEAMS", "SMST_SYNTH_EMIT", "SMST_NO_FAST_FFT")
COUNTERS = ("analyse_teams", "analyse_fast", "analyse_generic", "synth_teams", "synth_fast", "synth_generic", "synth_emit")


def _digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def run_case(lib, env, name):
    """-> {what: digest} of one case; env: anything with setenv / delenv (pytest's monkeypatch)"""
    case = CASES[name]
    pkg = package()
    for k in SWITCHES:
        env.delenv(k, raising=False)
    for k, val in case["env"].items():
        env.setenv(k, val)
    S, C, sr = case["streams"], 2, case["sample_rate"]
    before = {k: pkg.launch_count(k, lib) for k in COUNTERS}
    b = pkg.StretchBatch(S, C, preset=case["preset"], sample_rate=sr, lib=lib)
    I = b.intervalSamples()
    # call 1: 9 hops for every stream (the first at sample 0); call 2: ragged -- 0 to 4 hops, another length per stream
    n1 = np.full(S, 9*I, np.int64)
    n2 = np.array([(s % 5)*I + 13*s + 1 for s in range(S)], np.int64)
    n_max = int(n1.max() + n2.max())
    x = np.stack([synth_input(s, C, n_max, sr) for s in range(S)])
    got = {}
    pos = np.zeros(S, np.int64)
    for call, n_out in enumerate((n1, n2)):
        n_in = np.maximum(n_out*4//5, 1).astype(np.int32)  # 1.25x
        xin = np.zeros((S, C, int(n_in.max())), np.float32)
        for s in range(S):
            xin[s, :, :n_in[s]] = x[s, :, pos[s]:pos[s] + n_in[s]]
        pos += n_in
        y = np.array(b.process(xin, n_out.astype(np.int32), in_samples=n_in), copy=True)
        if call == 0:
            assert float(np.abs(y).max()) > 0.05
        got["output %d" % call] = _digest(np.concatenate([y[s, :, :n_out[s]].ravel() for s in range(S)]))
        carry = [b.debug_carry(s) for s in range(S)]
        got["carried sums %d" % call] = _digest(np.concatenate([c[0].ravel() for c in carry]))
        got["carried products %d" % call] = _digest(np.concatenate([c[1].ravel() for c in carry]))
    for which, what in enumerate(("input", "previous input", "output", "energy")):
        got["state: " + what] = _digest(np.concatenate([np.asarray(b.debug_state(s, which)).ravel() for s in range(S)]))
    b.close()
    for k in SWITCHES:
        env.delenv(k, raising=False)
    grew = {k: pkg.launch_count(k, lib) - before[k] for k in COUNTERS}
    assert all(grew[k] > 0 for k in case["ran"]) and all(grew[k] == 0 for k in case["idle"]), (name, grew)
    return got


def case_bit_identity(lib, monkeypatch, name, kind):
    want = json.load(open(GOLDEN[kind]))["cases"][name]
    got = run_case(lib, monkeypatch, name)
    assert sorted(got) == sorted(want)
    differing = [k for k in sorted(got) if got[k] != want[k]]
    assert not differing, (name, differing)


class _Environ:
    def setenv(self, k, v):
        os.environ[k] = v

    def delenv(self, k, raising=False):
        os.environ.pop(k, None)


def record(kind, names):
    import ctypes
    pkg = package()
    lib = pkg.load_library() if kind == "gpu" else pkg.bind(ctypes.CDLL(os.environ.get("SMST_EMU_LIBRARY") or os.path.join(ROOT, "tests", "emu", "libsmst_emu.so")))
    doc = {"recorded_from": "the commit before csrc/smst_fft_complex.h (91889fb), %s" % ("MI355X" if kind == "gpu" else "CPU stand-in"), "cases": {}}
    for name in names:
        doc["cases"][name] = run_case(lib, _Environ(), name)
        print(name, "recorded", flush=True)
    return doc


if __name__ == "__main__":
    import sys
    kind, dest = sys.argv[2], sys.argv[3]
    doc = record(kind, sys.argv[4:] or list(CASES))
    with open(dest, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
