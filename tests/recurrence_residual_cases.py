"""The bin recurrence (csrc/smst_recurrence.h: computeRecord, recordChannelFields, recurrenceOutputs, makeOutput* and the channel lock, in every
form recurrenceForm chooses among) against a plain numpy mirror of the reference's steps (signalsmith-stretch.h:642-660 the hop rotation,
:697-719 the preliminary prediction, :722-803 the main prediction and the lock), BIN BY BIN: shared by the CPU stand-in and the GPU test.

THE INSTRUMENT.  Within a hop out[b] feeds out[b+1] and out[b+L], and the next hop reads it too: compared after a free run, a rounding at
one bin is everywhere a few bins later, which is why the checker comparisons carry bounds built for chaos.  Here nothing is propagated.
After a hop everything that went into one bin of it is still readable or known: the own-hop taps out[b-1] and out[b-L] are final outputs
of the same hop, so the mirror takes, for bin b, the PRODUCT'S OWN float32 out[.][b-1] and out[.][b-L] of that hop, the previous hop's
out[.][b+1] and out[.][b+L], both spectra, the map and the energies, evaluates in float64 what the reference says out[.][b] is, and
compares that with the product's out[.][b].  An error at one bin shows at that bin and nowhere else; the maximum channel is decided on the
very floats the product decided on.

PARTNER STREAMS.  Only the state after a call can be read (debug_state, debug_map), so a checked hop is the LAST hop of a stream B that fires
h + 1 hops in the measured call; its partner A -- the same signal, parameters and warm-up, in the same batch -- fires h hops.  A's Band.output,
Band.input and Prediction.energy after the call are hop h's previous output, previous input and previous energy; B's Band.input, Band.output,
Prediction.energy and map are hop h's own.  (h = 0: the stream's own state after the warm-up call.)  The premise -- a hop's result does not
depend on how many hops follow it in the call -- is asserted on the checker (case_partner_premise); a product that violates it fails the
residual, and that is a finding.  A stream that fires k hops is B for h = k - 1 and A for h = k.

TIERS.  A: the input advances by the interval, one sample less or one more per hop, so no hop re-analyses its previous input (:303) and
every operand is read back; the time factors are 1, I/(I-1), I/(I+1), the taps at map - tf and map - L tf fractional.  B: 1.6x, 0.8x and
2.5x (the input advance rounded to whole samples, so that partner streams share their hops exactly; beyond 2x every bin draws its two
time factors: the engine is restated here, engine_draws -- and partners must share the engine's state too, which only streams 0 and 1 of a
batch do: layout).  The previous input of such a hop exists only inside the call: the mirror forms it as
the float64 DFT (geometry_cases.dft_spectrum, the checker's window) of the block one interval before the hop's input offset (:288-303), and
the bound of a bin is widened by the linearised effect of TOL_SPECTRUM_MAX of the hop's largest bin -- what the product's float32 spectrum
may differ from that DFT by -- on out[b].  TIER B IS A NET FOR GROSS ERRORS BY DESIGN: a staging window that does not reach b - L tf at
tf = 1.6, a wrong draw index, a wrong row for SRC_REANALYSED.

TOLERANCES.  Compared: |out_product - out_mirror| / sqrt(E[c][b]) per bin and channel over the bin's condition number
kappa[b] = (sum of the four terms' magnitudes)/|phi| (1 where makeOutput falls back to the input; locked channels inherit the maximum
channel's).  The yardstick is the same local formula in float32 in the reference's operation order (numpy float32: IEEE division and
square root, no contraction) against its float64 evaluation on operands that no product code has touched (the checker's, driven through
the cases' own calls: measure_yardstick), worst kappa-normalised figure per (bands, channels, tier): YARDSTICK.  The product must stay within
MARGIN = 4 times that -- what FMA contraction and re-association, the three 1-ulp hardware operations (rcp, rsq, sqrt) and the lock
normalised by E_m |T|^2 instead of |out_m T|^2 have to fit into.  EXPERIMENTS.md has the product's own worst figures next to the yardsticks.
  * a bin with E = 0 in a channel must be exactly zero there;
  * the maximum channel: the mirror decides on the read-back energies, first maximum wins; only where the two largest differ by less than
    4 float32 ulps (a plain tile forms |in|^2 in the kernel, contracted or not) is the bin accepted under either choice;
  * makeOutput's fallback (:598-601): where |phase|^2 lies within (1 +- 10 bound kappa) of 1e-15 either branch is accepted;
  * at most CAP_EXCUSED of a case's bins may be excused (asserted on the mirror alone: test_inputs_stay_within_caps), and in Tier B at most
    CAP_ALLOWANCE_SHARE of the bins with energy may have an allowance above 1e-2.

NOT HERE.  Bins below a hop's start bin (split computation).  half_state: the read-back output is fp16-rounded while the in-tile taps are
not, so the residual would measure the quantisation."""
import ctypes
import ctypes.util

import numpy as np

import feed_stage_cases as fs
import geometry_cases as gc
import recurrence_form_cases as rf
from conftest import package, synth_input

MARGIN = 4.0
NOISE_FLOOR = np.float32(1e-15)
CAP_EXCUSED = 0.01
CAP_ALLOWANCE_SHARE = 0.10
ALLOWANCE_LARGE = 1e-2
WARMUP_HOPS = 3
SAMPLE_RATE = 48000
NOISE_STREAM = 8  # conftest.synth_input: stream type = s mod 3, 2 = noise
QUIET, QUIET_TILT_DB = 45.0, 40.0  # the quiet stream: scaled by QUIET/fftSamples, its level falling by QUIET_TILT_DB from 0 to the Nyquist frequency

# The reference's own float32 rounding of the local formula, kappa-normalised: measure_yardstick() on the checker's operands over the cases'
# calls (test_recurrence_residual_emu.py::test_inputs_stay_within_caps prints them; EXPERIMENTS.md).  (bands, channels, tier)
YARDSTICK = {
    (256, 1, "A"): 8.72e-06, (256, 1, "B"): 1.57e-05, (256, 2, "A"): 1.01e-05, (256, 2, "B"): 1.75e-05,
    (256, 3, "A"): 3.39e-06, (256, 3, "B"): 1.68e-05, (256, 8, "A"): 2.13e-06, (256, 8, "B"): 1.71e-05,
    (256, 9, "A"): 2.12e-06, (256, 9, "B"): 1.70e-05, (256, 16, "A"): 2.07e-06, (256, 16, "B"): 1.70e-05,
    (384, 1, "A"): 3.78e-05, (384, 3, "A"): 5.83e-06, (1024, 2, "A"): 6.75e-05, (2560, 2, "A"): 7.52e-04,
    (2560, 2, "B"): 4.67e-04, (3072, 2, "A"): 1.38e-03, (3072, 2, "B"): 3.00e-04, (4096, 2, "A"): 4.84e-05,
}


def bound(M, channels, tier):
    return MARGIN*YARDSTICK[(M, channels, tier)]


# ---------------------------------------------------------------------------------------------------------------------------------
# Geometry, time factors, signals
# ---------------------------------------------------------------------------------------------------------------------------------
def _libm():
    path = ctypes.util.find_library("m")
    lib = ctypes.CDLL(path) if path else None
    if lib is not None:
        for f in (lib.cosf, lib.sinf):
            f.restype, f.argtypes = ctypes.c_float, (ctypes.c_float,)
    return lib


def rotation_table(M, N, I):
    """The hop rotation as the reference accumulates it (:647-656; smst_engine.cpp uploadConstantTables does the same): a float32 running
    product from std::polar of two float32 angles.  A definition, not a rounding: the float64 mirror uses these float32 values."""
    f32 = np.float32
    f0, f1 = f32(0.5)/f32(N), f32(1.5)/f32(N)
    a0, a1 = f0*f32(I)*f32(2*np.pi), (f1 - f0)*f32(I)*f32(2*np.pi)
    m = _libm()
    polar = (lambda a: (f32(m.cosf(float(a))), f32(m.sinf(float(a))))) if m is not None else (lambda a: (f32(np.cos(float(a))), f32(np.sin(float(a)))))
    (r, i), (sr, si) = polar(a0), polar(a1)
    rot = np.zeros(M, np.complex64)
    for b in range(M):
        rot[b] = complex(r, i)
        r, i = r*sr - i*si, r*si + i*sr
    return rot


class Geometry:
    def __init__(self, obj, channels):
        """obj: a StretchBatch or a checker instance"""
        self.C, self.M, self.N, self.I, self.B = channels, obj.bands(), obj.fftSamples(), obj.intervalSamples(), obj.blockSamples()
        self.L = int(np.round(np.float32(self.N)/np.float32(self.I)))  # :637
        self.rot = rotation_table(self.M, self.N, self.I)


# name: (tier, the input advance per hop from the interval)
TIME_FACTORS = {
    "1": ("A", lambda I: I), "I/(I-1)": ("A", lambda I: I - 1), "I/(I+1)": ("A", lambda I: I + 1),
    "1.6x": ("B", lambda I: int(round(I/1.6))), "0.8x": ("B", lambda I: int(round(I/0.8))), "2.5x": ("B", lambda I: int(round(I/2.5))),
}
TIER_A = tuple(k for k, v in TIME_FACTORS.items() if v[0] == "A")
TIER_B = tuple(k for k, v in TIME_FACTORS.items() if v[0] == "B")
LCG_MODULUS, LCG_MULTIPLIER = 2147483647, 16807


def engine_draws(seed, hops_before, M, tf):
    """The 2M - 2 time factors of a randomised hop (smst_kernels_common.h engineDraw; libstdc++'s minstd_rand0 behind
    uniform_real_distribution<float>(4 - tf, tf), :640): bin b's upward steps take draw 2b - 1 (b > 0), its downward steps draw 2b (b < M - 1);
    every randomised hop before it advanced the engine by 2M - 2.  -> (tf_up[M], tf_down[M]) float32."""
    f32 = np.float32
    state = seed % LCG_MODULUS or 1
    state = state*pow(LCG_MULTIPLIER, (2*M - 2)*hops_before, LCG_MODULUS) % LCG_MODULUS
    x = np.zeros(2*M, np.int64)
    for j in range(2*M - 2):
        state = state*LCG_MULTIPLIER % LCG_MODULUS
        x[j] = state
    u = np.minimum((x - 1).astype(f32)*f32(2.0**-31), np.nextafter(f32(1), f32(0)))
    tf = f32(tf)
    lo = f32(4) - tf
    draws = u*(tf - lo) + lo
    up, down = np.full(M, tf, f32), np.full(M, tf, f32)
    b = np.arange(M)
    up[1:] = draws[2*b[1:] - 1]
    down[:M - 1] = draws[2*b[:M - 1]]
    return up, down


def time_factors(g, advance, seed, random_hops_before):
    """(tf_up, tf_down, random) of a hop whose input advanced by `advance` samples (:312, :638-640)."""
    tf = max(np.float32(g.I)/max(np.float32(1), np.float32(advance)), np.float32(0.5))
    if tf > 2:
        return engine_draws(seed, random_hops_before, g.M, tf) + (True,)
    return np.full(g.M, tf, np.float32), np.full(g.M, tf, np.float32), False


def signal(kind, channels, n, fft_samples):
    """A sine pair over noise 12 dB below it (conftest.synth_input, streams 0 and 2), a different level per channel (1 - 0.07 c), independent
    noise per channel -- so every bin has energy and the maximum channel changes from bin to bin.  "quiet": the same, scaled down and its
    level falling with frequency: |phase|^2 goes with the cube of the energy, so makeOutput's fallback takes the upper bins and leaves the
    lower ones at every shape and time factor; "silent": channel 1 digitally silent."""
    x = 0.6*synth_input(0, channels, n, SAMPLE_RATE) + 0.5*synth_input(NOISE_STREAM, channels, n, SAMPLE_RATE)
    x *= (1 - 0.07*np.arange(channels))[:, None]
    if kind == "quiet":
        spectrum = np.fft.rfft(x.astype(np.float64), axis=-1)
        tilt = 10.0**(-QUIET_TILT_DB/20*np.arange(spectrum.shape[-1])/max(spectrum.shape[-1] - 1, 1))
        x = np.fft.irfft(spectrum*tilt, n, axis=-1)*(QUIET/fft_samples)
    if kind == "silent" and channels > 1:
        x[1] = 0
    return np.ascontiguousarray(x, np.float32)


# ---------------------------------------------------------------------------------------------------------------------------------
# The mirror.  Complex values are (re, im) pairs of real arrays, multiplied component by component in the reference's order (_impl::mul).
# ---------------------------------------------------------------------------------------------------------------------------------
def _c(z, T):
    z = np.asarray(z)
    return np.asarray(z.real, T), np.asarray(z.imag, T)


def _mul(a, b):
    return a[0]*b[0] - a[1]*b[1], a[0]*b[1] + a[1]*b[0]


def _mulc(a, b):  # a * conj(b), mul<true>
    return b[0]*a[0] + b[1]*a[1], b[0]*a[1] - b[1]*a[0]


def _add(a, b):
    return a[0] + b[0], a[1] + b[1]


def _norm(a):
    return a[0]*a[0] + a[1]*a[1]


def _mag(a):
    return np.hypot(np.asarray(a[0], np.float64), np.asarray(a[1], np.float64))


def _where(m, a, b):
    return np.where(m, a[0], b[0]), np.where(m, a[1], b[1])


def _lerp(rows, pos, T):
    """getFractional (:553-580) of rows [.., M] at positions pos [M]: nothing outside [0, M)."""
    M = rows[0].shape[-1]
    low = np.floor(pos)
    frac = np.asarray(pos - low, T)
    idx = np.clip(low, -2, M).astype(np.int64)
    out = []
    for r in rows:
        z = np.zeros(r.shape[:-1] + (1,), T)
        pad = np.concatenate((z, r, z), axis=-1)  # bins -1 .. M
        lo, hi = pad[..., np.clip(idx + 1, 0, M + 1)], pad[..., np.clip(idx + 2, 0, M + 1)]
        out.append(lo + (hi - lo)*frac)
    return tuple(out)


def _shift(a, k):
    """a[.., b + k], zero where that is past the last bin (k > 0) or before the first (k < 0)"""
    out = np.zeros_like(a)
    M = a.shape[-1]
    if k > 0:
        out[..., :M - k] = a[..., k:]
    else:
        out[..., -k:] = a[..., :M + k]
    return out


class Hop:
    """The operands of one hop: its own Band.input `cur`, map `ib` (inputBin per bin), Prediction.energy `E` and outputs `out`; the previous
    hop's output `prev_out`, input `prev_in` and energy `Eprev`; the time factors per bin."""

    def __init__(self, g, cur, ib, E, out, prev_out, prev_in, Eprev, tf_up, tf_down, tier="A", prev_in_error=0.0):
        self.g, self.cur, self.E, self.out, self.prev_out, self.prev_in, self.Eprev = g, cur, np.asarray(E, np.float32), out, prev_out, prev_in, np.asarray(Eprev, np.float32)
        self.ib = np.arange(g.M, dtype=np.float32) if ib is None else np.asarray(ib, np.float32)
        self.tf_up, self.tf_down, self.tier, self.prev_in_error = tf_up, tf_down, tier, prev_in_error

    def max_channel(self):
        """(first maximum of the read-back energies, the runner-up where it is within 4 float32 ulps of it else -1)"""
        mc = np.argmax(self.E, axis=0)
        if self.E.shape[0] == 1:
            return mc, np.full(self.g.M, -1)
        top = np.take_along_axis(self.E, mc[None], 0)[0]
        rest = self.E.copy()
        np.put_along_axis(rest, mc[None], -1.0, 0)
        second = np.argmax(rest, axis=0)
        close = (top - np.take_along_axis(rest, second[None], 0)[0] < 4*np.spacing(top)) & (top > 0)
        return mc, np.where(close, second, -1)


def _make_output(phase, inp, energy, T, flip=None):
    """Prediction::makeOutput (:596-603) -> (output, |phase|^2, whether it fell back to the input)"""
    n = _norm(phase)
    weak = n <= T(NOISE_FLOOR)
    if flip is not None:
        weak = weak ^ flip
    ph = _where(weak, inp, phase)
    pn = np.where(weak, _norm(inp) + T(NOISE_FLOOR), n)
    with np.errstate(all="ignore"):
        gain = np.sqrt(energy/pn)
    gain = np.where(pn > 0, gain, T(0))  # (only under a flip: a phase of exactly zero forced through the normal branch)
    return (ph[0]*gain, ph[1]*gain), n, weak


class Prepared:
    """Everything of a hop that does not depend on its own outputs, in T arithmetic."""

    def __init__(self, op, T, mc):
        g = op.g
        M, L = g.M, g.L
        self.op, self.T, self.mc = op, T, mc
        sel = lambda a: np.take_along_axis(a, mc[None], 0)[0]  # noqa: E731
        sel2 = lambda z: (sel(z[0]), sel(z[1]))  # noqa: E731
        cur, rot = _c(op.cur, T), _c(g.rot, T)
        ib = op.ib.astype(T)
        self.E, Eprev = op.E.astype(T), op.Eprev.astype(T)
        self.P = _lerp(cur, ib, T)  # Prediction.input, :710
        # the rotation (:651-656) and the preliminary prediction (:713-716) of every bin and channel
        prev_in, prev_out = _mul(_c(op.prev_in, T), rot), _mul(_c(op.prev_out, T), rot)
        twist = _mulc(self.P, _lerp(prev_in, ib, T))
        phase = _mul(prev_out, twist)
        self.den = np.maximum(Eprev, self.E) + T(NOISE_FLOOR)
        prelim = (phase[0]/self.den, phase[1]/self.den)
        # the four twists of the maximum channel (:748-785)
        tf_up, tf_down = op.tf_up.astype(T), op.tf_down.astype(T)
        b = np.arange(M)
        zero = (np.zeros(M, T), np.zeros(M, T))
        self.Pm, self.Em = sel2(self.P), sel(self.E)
        self.A = _where(b > 0, _mulc(self.Pm, sel2(_lerp(cur, ib - tf_up, T))), zero)
        self.Bc = _where(b >= L, _mulc(self.Pm, sel2(_lerp(cur, ib - T(L)*tf_up, T))), zero)
        P1, PL = sel2((_shift(self.P[0], 1), _shift(self.P[1], 1))), sel2((_shift(self.P[0], L), _shift(self.P[1], L)))
        down1, downL = sel2(_lerp(cur, _shift(ib, 1) - tf_down, T)), sel2(_lerp(cur, _shift(ib, L) - T(L)*tf_down, T))
        up1, upL = sel2((_shift(prelim[0], 1), _shift(prelim[1], 1))), sel2((_shift(prelim[0], L), _shift(prelim[1], L)))
        self.tC = _where(b < M - 1, _mulc(up1, _mulc(P1, down1)), zero)
        self.tD = _where(b < M - L, _mulc(upL, _mulc(PL, downL)), zero)
        # d|previous-hop terms| / d|previous input|: out_prev P conj(Q) / den times the vertical twist (Tier B's allowance)
        po = _mag(_c(op.prev_out, np.float64))
        s1 = sel(_shift(po*_mag(self.P)/np.asarray(self.den, np.float64), 1))*_mag(P1)*_mag(down1)
        sL = sel(_shift(po*_mag(self.P)/np.asarray(self.den, np.float64), L))*_mag(PL)*_mag(downL)
        self.sensitivity = np.where(b < M - 1, s1, 0.0) + np.where(b < M - L, sL, 0.0)

    def phase(self, own, bins=slice(None)):
        """:744-786 at `bins`, the own-hop taps from `own` ((re, im) [C, M])"""
        M, L, mc = self.op.g.M, self.op.g.L, self.mc
        b = np.arange(M)[bins]
        m = mc[bins]
        o1 = (own[0][m, np.maximum(b - 1, 0)], own[1][m, np.maximum(b - 1, 0)])
        oL = (own[0][m, np.maximum(b - L, 0)], own[1][m, np.maximum(b - L, 0)])
        at = lambda z: (z[0][bins], z[1][bins])  # noqa: E731
        tA, tB = _mul(o1, at(self.A)), _mul(oL, at(self.Bc))  # (the coefficients are zero where the reference skips the term)
        phi = _add(_add(_add(tA, tB), at(self.tC)), at(self.tD))
        return phi, _mag(tA) + _mag(tB) + _mag(at(self.tC)) + _mag(at(self.tD))

    def outputs(self, phi, bins=slice(None), flip_m=None, flip_c=None):
        """:788-800 -> (out (re, im) [C, K], |phase|^2 of the maximum channel [K], of the locks [C, K], fallback taken [C, K])"""
        T, C = self.T, self.E.shape[0]
        Pm, Em, m = (self.Pm[0][bins], self.Pm[1][bins]), self.Em[bins], self.mc[bins]
        om, n_m, weak_m = _make_output(phi, Pm, Em, T, flip_m)
        K = len(Em)
        out = (np.zeros((C, K), T), np.zeros((C, K), T))
        n_c, weak = np.zeros((C, K), T), np.zeros((C, K), bool)
        for c in range(C):
            Pc = (self.P[0][c][bins], self.P[1][c][bins])
            oc, n_c[c], weak[c] = _make_output(_mul(om, _mulc(Pc, Pm)), Pc, self.E[c][bins], T, None if flip_c is None else flip_c[c])
            out[0][c], out[1][c] = np.where(m == c, om[0], oc[0]), np.where(m == c, om[1], oc[1])
            weak[c] = np.where(m == c, weak_m, weak[c])
            n_c[c] = np.where(m == c, n_m, n_c[c])
        return out, n_m, n_c, weak


def evaluate(op, T, mc=None, flip_m=None, flip_c=None):
    """The local formula of every bin, the own-hop taps taken from op.out: a dict of out [C, M] complex, kappa [M], the norms and branches."""
    mc = op.max_channel()[0] if mc is None else mc
    p = Prepared(op, T, mc)
    phi, terms = p.phase(_c(op.out, T))
    out, n_m, n_c, weak = p.outputs(phi, flip_m=flip_m, flip_c=flip_c)
    weak_m = np.take_along_axis(weak, mc[None], 0)[0]
    with np.errstate(all="ignore"):
        kappa = np.where(weak_m, 1.0, np.maximum(terms/_mag(phi), 1.0))
        allowance = np.where(weak_m, 0.0, op.prev_in_error*p.sensitivity/_mag(phi))
    return dict(out=np.asarray(out[0], np.float64) + 1j*np.asarray(out[1], np.float64), kappa=np.nan_to_num(kappa, nan=1.0, posinf=1e300), n_m=np.asarray(n_m, np.float64),
                n_c=np.asarray(n_c, np.float64), weak=weak, weak_m=weak_m, mc=mc, allowance=np.nan_to_num(allowance, nan=0.0, posinf=1e300))


def free_run(op, T=np.float32):
    """The hop run free in T arithmetic: every bin from the mirror's OWN outputs, bin after bin (what check_mirror compares with the checker)."""
    p = Prepared(op, T, op.max_channel()[0])
    C, M = p.E.shape
    own = (np.zeros((C, M), T), np.zeros((C, M), T))
    for b in range(M):
        bins = slice(b, b + 1)
        phi, _ = p.phase(own, bins)
        out, _, _, _ = p.outputs(phi, bins)
        own[0][:, b], own[1][:, b] = out[0][:, 0], out[1][:, 0]
    return own[0].astype(np.float64) + 1j*own[1]


def deviations(op, got, limit, T=np.float64):
    """|got - mirror| / sqrt(E) per bin and channel for outputs `got` [C, M] against the float64 mirror of `op`, the decisions a rounding can flip
    (limit: the bound they are cleared with) accepted either way.  -> dict: dev [C, M] (nan where E = 0), kappa, allowance, excused [M],
    nonzero_where_silent (count), r (the mirror's base evaluation)."""
    r = evaluate(op, T)
    mc, runner_up = op.max_channel()
    E = op.E.astype(np.float64)
    clear = 10*limit*r["kappa"]
    near = lambda n: np.abs(n/float(NOISE_FLOOR) - 1) <= clear  # noqa: E731
    amb_m = near(r["n_m"])
    amb_c = near(r["n_c"]) & (np.arange(E.shape[0])[:, None] != mc[None])
    tied = runner_up >= 0
    with np.errstate(all="ignore"):
        dev = np.abs(got - r["out"])/np.sqrt(E)
        variants = []
        for alt in ((False, True) if tied.any() else (False,)):
            mca = np.where(tied, runner_up, mc) if alt else mc
            for fm in ((False, True) if amb_m.any() else (False,)):
                for fc in ((False, True) if amb_c.any() else (False,)):
                    if alt or fm or fc:
                        variants.append(evaluate(op, T, mca, amb_m if fm else None, amb_c if fc else None))
        kappa, allowance = r["kappa"].copy(), r["allowance"].copy()
        for v in variants:
            d = np.abs(got - v["out"])/np.sqrt(E)
            worst_of = lambda dd, vv: np.nanmax(np.where(E > 0, dd/(limit*vv["kappa"] + vv["allowance"])[None], 0.0), axis=0)  # noqa: E731
            col = worst_of(d, v) < worst_of(dev, dict(kappa=kappa, allowance=allowance))
            dev = np.where(col[None], d, dev)
            kappa, allowance = np.where(col, v["kappa"], kappa), np.where(col, v["allowance"], allowance)
    silent = E == 0
    return dict(dev=np.where(silent, np.nan, dev), kappa=kappa, allowance=allowance, excused=tied | amb_m | amb_c.any(axis=0),
                nonzero_where_silent=int(np.count_nonzero(np.asarray(got)[silent])), r=r)


def assert_within(op, got, limit, label, fig, T=np.float64):
    """The check every (hop, stream) has to pass; the worst figures go into `fig`."""
    d = deviations(op, got, limit, T)
    assert d["nonzero_where_silent"] == 0, (label, "a bin without energy must be exactly zero", d["nonzero_where_silent"])
    live = ~np.isnan(d["dev"])
    if not live.any():
        return d
    assert np.isfinite(np.asarray(got)).all(), (label, "non-finite output")
    with np.errstate(all="ignore"):
        allowed = limit*d["kappa"] + d["allowance"]
        ratio = np.where(live, d["dev"]/allowed[None], 0.0)
        normalised = np.where(live, np.maximum(d["dev"] - d["allowance"][None], 0.0)/d["kappa"][None], 0.0)
    c, b = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    fig["normalised"] = max(fig.get("normalised", 0.0), float(normalised.max()))
    fig["of_bound"] = max(fig.get("of_bound", 0.0), float(ratio.max()))
    assert ratio[c, b] <= 1, "%s: bin %d channel %d (maximum channel %d): |out - mirror|/sqrt(E) = %.3e, kappa %.3g, allowance %.3e, bound %.3e" % (
        label, b, c, d["r"]["mc"][b], d["dev"][c, b], d["kappa"][b], d["allowance"][b], limit)
    return d


# ---------------------------------------------------------------------------------------------------------------------------------
# Driving an implementation through a warm-up call and a measured call; states and operands
# ---------------------------------------------------------------------------------------------------------------------------------
def checker_state(r):
    return dict(input=r.bands_complex(0).astype(np.complex64), output=r.bands_complex(2).astype(np.complex64), energy=r.bands_real(4).copy(), map=r.output_map())


def product_state(b, s):
    m = b.debug_map(s)
    return dict(input=b.debug_state(s, 0).astype(np.complex64), output=b.debug_state(s, 2).astype(np.complex64), energy=b.debug_state(s, 3), map=m)


def previous_input_dft(g, window, x, end):
    """Band.prevInput of a hop that re-analyses it (:333-349): the block one interval before the hop's input offset, in float64."""
    return gc.dft_spectrum(gc._block_ending(x, end - g.I, g.B), window, g.N)


def operands(g, a, b, mapped, tf_name, seed, hops_before, x=None, window=None):
    """Hop h's operands from the partner's state `a` (before the hop) and the stream's own `b` (after it); hops_before: the hops of the stream
    before this one, the warm-up's included (what a randomised hop's draws and a re-analysed hop's input offset follow from)."""
    tier, advance = TIME_FACTORS[tf_name]
    adv = advance(g.I)
    tf_up, tf_down, _ = time_factors(g, adv, seed, hops_before)
    prev_in, err = a["input"], 0.0
    if tier == "B":
        prev_in = previous_input_dft(g, window, x, hops_before*adv)
        err = gc.TOL_SPECTRUM_MAX*float(np.abs(prev_in).max())
    ib = b["map"][:, 0] if (mapped and b["map"] is not None) else None
    return Hop(g, b["input"], ib, b["energy"], b["output"], a["output"], prev_in, a["energy"], tf_up, tf_down, tier, err)


def checker_pair(ref, g_of, channels, params, kind, tf_name, h, seed=0, configure=None):
    """Two checker instances through the cases' calls: A fires h hops in the measured call, B h + 1.  -> (geometry, state of A, state of B, x, B)"""
    states = []
    for k in (h, h + 1):
        r = ref.RefStretch(seed)
        configure(r)
        params.apply(r)
        g = g_of(r)
        adv = TIME_FACTORS[tf_name][1](g.I)
        x = signal(kind, channels, (WARMUP_HOPS + h + 1)*adv, g.N)
        r.process(x[:, :WARMUP_HOPS*adv], WARMUP_HOPS*g.I)
        if k:
            r.process(x[:, WARMUP_HOPS*adv:(WARMUP_HOPS + k)*adv], k*g.I)
        states.append(checker_state(r))
    return g, states[0], states[1], x, r


def case_partner_premise(ref, channels=2, block=512, interval=128):
    """A hop's result does not depend on how many hops follow it in the call: the measured call of h + 1 hops in one piece, and as the
    partner's call of h hops followed by one more hop, leave identical private bands."""
    if getattr(ref, "is_port", False):
        return 0
    compared = 0
    for tf_name in ("I/(I-1)", "1.6x", "2.5x"):
        adv = TIME_FACTORS[tf_name][1](interval)
        for h in (1, 2, 9):
            x = signal("normal", channels, (WARMUP_HOPS + h + 1)*adv, 2*gc._bands_of_block(block))
            whole, parts = ref.RefStretch(0), ref.RefStretch(0)
            for r in (whole, parts):
                r.configure(channels, block, interval)
                fs.PARAMS["up12_limit"].apply(r)
                r.process(x[:, :WARMUP_HOPS*adv], WARMUP_HOPS*interval)
            at = WARMUP_HOPS*adv
            whole.process(x[:, at:at + (h + 1)*adv], (h + 1)*interval)
            parts.process(x[:, at:at + h*adv], h*interval)
            parts.process(x[:, at + h*adv:at + (h + 1)*adv], interval)
            for which in (0, 1, 2):
                assert np.array_equal(whole.bands_complex(which), parts.bands_complex(which)), (tf_name, h, which)
            assert np.array_equal(whole.bands_real(4), parts.bands_real(4)) and np.array_equal(whole.output_map(), parts.output_map()), (tf_name, h)
            compared += 1
    return compared


ULPS = 16*2.0**-24  # the float32 mirror and the checker run the same operations in the same order: a few ulp for the compiler's freedom


def check_mirror(ref, channels=2, block=512, interval=128):
    """Pins the mirror before it judges anything: the float32 mirror, fed with the checker's own private bands before a hop, runs the hop free
    -- every bin from its own outputs -- and its Band.output is compared with the checker's to a few ulp kappa; then the bin-local float64
    evaluation on the checker's operands.  The port restates none of the members: there only the mirror's own sanity checks run."""
    g = None
    compared = 0
    if not getattr(ref, "is_port", False):
        for name, tf_name, h in (("none", "I/(I-1)", 2), ("up12_limit", "I/(I+1)", 1), ("table7", "1", 0), ("comp_estimated", "I/(I-1)", 2), ("none", "2.5x", 1), ("none", "1.6x", 2)):
            p = fs.PARAMS[name]
            g, a, b, x, r = checker_pair(ref, lambda r: Geometry(r, channels), channels, p, "normal", tf_name, h, configure=lambda r: r.configure(channels, block, interval))
            op = operands(g, a, b, p.mapped, tf_name, 0, WARMUP_HOPS + h, x, r.window())
            if op.tier == "B":  # (the spectrum the checker re-analysed is gone after the hop: bin-local, with Tier B's allowance)
                fig = {}
                assert_within(op, b["output"], ULPS, "checker %s %s h = %d" % (name, tf_name, h), fig, np.float32)
                print("mirror against the checker, %s, %s, h = %d: %s" % (name, tf_name, h, fig))
                compared += 1
                continue
            got = free_run(op)
            kappa = evaluate(op, np.float64)["kappa"]
            with np.errstate(all="ignore"):
                dev = np.abs(got - b["output"])/np.sqrt(op.E.astype(np.float64))
            dev = np.where(op.E > 0, dev, np.abs(got - b["output"]))
            worst = float(np.max(dev/kappa[None]))
            print("mirror against the checker, %s, %s, h = %d: %.2e" % (name, tf_name, h, worst))
            assert worst <= ULPS, (name, tf_name, h, worst)
            compared += 1
    # (silence gives exactly zero)
    g = g or _PlainGeometry(channels, 256, 512, 128)
    zero = np.zeros((channels, g.M), np.complex64)
    op = Hop(g, zero, None, np.zeros((channels, g.M)), zero, zero, zero, np.zeros((channels, g.M)), np.ones(g.M, np.float32), np.ones(g.M, np.float32))
    assert not evaluate(op, np.float64)["out"].any()
    return compared


class _PlainGeometry(Geometry):
    def __init__(self, channels, M, block, interval):
        self.C, self.M, self.N, self.I, self.B = channels, M, 2*M, interval, block
        self.L = int(np.round(np.float32(self.N)/np.float32(self.I)))
        self.rot = rotation_table(M, self.N, interval)


# ---------------------------------------------------------------------------------------------------------------------------------
# The rows: the smallest shapes that reach each form (geometries and switches from recurrence_form_cases.SCENARIOS)
# ---------------------------------------------------------------------------------------------------------------------------------
FULL = (0, 1, 2, 7, 8, 9, 63)
FULL_256 = FULL + (64,)  # lane 0 of the call's second tile, taken from the first tile's carry
# feed_stage_cases.PARAMS: none | transposed without and with a tonality limit | a 7-knot table | a formant factor with a given base | compensation
# with an estimated base
MAPPED_SETS = ("none", "down12", "up12_limit", "table7", "shift_up3", "comp_estimated")


def _row(scenario, hops, shows, env=None, sets=("none",), tier_b=None):
    sc = dict(rf.DEFAULTS, **rf.SCENARIOS[scenario])
    return dict(scenario=scenario, hops=hops, shows=shows, env=dict(sc["env"], **(env or {})), sets=sets, tier_b=sc["bands"] == 256 if tier_b is None else tier_b, sc=sc)


ROWS = {
    # kVocoder, plain bounded tiles at 256 bands, L = 4: line-aligned producers with interior blocks, staged, gathering; mono and stereo
    "aligned_mono": _row("small_mono", FULL_256, ("vocoder_aligned", "vocoder_interior")),
    "staged_mono": _row("small_mono", FULL_256, ("vocoder_staged",), env={"SMST_NO_ALIGN": "1"}),
    "gather_mono": _row("small_mono", FULL_256, ("vocoder_gather",), env={"SMST_NO_STAGE": "1"}),
    "aligned_stereo": _row("fresh_stereo", FULL_256, ("vocoder_aligned", "vocoder_interior")),
    "staged_stereo": _row("fresh_stereo", FULL_256, ("vocoder_staged",), env={"SMST_NO_ALIGN": "1"}),
    "gather_stereo": _row("fresh_stereo", FULL_256, ("vocoder_gather",), env={"SMST_NO_STAGE": "1"}),
    # presetDefault at 48 kHz (Tier B's tiles re-analyse: twisted), presetCheaper (L = 3: the longest reach at tf = 1.6)
    "default_48k": _row("default_48k", FULL, ("vocoder_aligned", "vocoder_interior"), tier_b=True),
    "default_48k_no_twist": _row("default_48k_no_twist", FULL, ("vocoder_aligned",), tier_b=True),
    "cheaper": _row("cheaper", FULL, ("vocoder_staged",), tier_b=True),
    "cheaper_align_all": _row("cheaper_align_all", FULL, ("vocoder_aligned",)),
    # mapped tiles: every parameter set side by side in one batch; the rotation table in LDS (256 bands) and not (4096)
    "mapped_256": _row("transposed_256", (0, 1, 2), ("vocoder_gather",), sets=MAPPED_SETS),
    "mapped_4096": _row("transposed_4096", (0, 1, 2), ("vocoder_gather",), sets=MAPPED_SETS),
    "step_6_mono": _row("step_6_mono", FULL, ("vocoder_gather",)),
    # one hop in the call: lanes across streams, one chain per stream, records through memory
    "across_mono": _row("one_hop_mono", (0,), ("vocoder_across",)),
    "across_stereo": _row("one_hop_stereo", (0,), ("vocoder_across",)),
    "one_stereo": _row("one_hop_no_across", (0,), ("vocoder_one",)),
    "one_mono": _row("one_hop_no_across_mono", (0,), ("vocoder_one",)),
    "one_three_channels": _row("three_channels_one_hop", (0,), ("vocoder_one",)),
    "one_eight_channels": _row("eight_channels_one_hop", (0,), ("vocoder_one",)),
    "unfused_one_hop_mono": _row("mono_no_fuse_one_hop", (0,), ("chain_unfused",)),
    # 3-8 channels: kVocoderN; more, SMST_NO_FUSE, or L = 6 from three channels on: kPredictB + kChain
    "three_channels": _row("three_channels", FULL_256, ("vocoder_n",)),
    "eight_channels": _row("eight_channels", FULL_256, ("vocoder_n",)),
    "nine_channels": _row("nine_channels", FULL_256, ("chain_unfused",)),
    "sixteen_channels": _row("sixteen_channels", FULL_256, ("chain_unfused",)),
    "three_channels_no_fuse": _row("three_channels_no_fuse", FULL_256, ("chain_unfused",)),
    "step_6_three_channels": _row("step_6_three_channels", FULL, ("chain_unfused",)),
    # kVocoderCont: one wavefront over the call's two tiles -- the last hop of the first tile, and hops behind the boundary
    "continuous": _row("continuous", (63, 66), ("vocoder_continuous",)),
}
EMU_ROWS = tuple(n for n, r in ROWS.items() if r["sc"]["bands"] <= 1024)
SHAPES = sorted({(r["sc"]["bands"], r["sc"]["channels"], tier) for r in ROWS.values() for tier in (("A", "B") if r["tier_b"] else ("A",))})


def layout(row, tf_name="1"):
    """The streams of a row's batch: (signal kind, parameter set, hops fired in the measured call), and the pairs to check: (h, stream of A
    or None for the stream's own state after the warm-up, stream of B).  With drawn time factors (2.5x) partners must share their engine's
    state as well: stream s is seeded with seed + s, and only 0 and 1 seed minstd_rand0 alike (0 becomes 1) -- so streams 0 and 1 are the one
    pair with h = 1, every other stream fires one hop and is checked from its own state after the warm-up (h = 0)."""
    r = ROWS[row]
    streams, pairs = [], []
    drawn = tf_name == "2.5x"

    def stream(kind, name, k):
        key = (kind, name, k)
        if key not in streams:
            streams.append(key)
        return streams.index(key)
    for i, name in enumerate(r["sets"]):
        hops = r["hops"] if i < 4 else r["hops"][:2]
        kinds = ("normal",) if len(r["sets"]) > 1 else (("normal", "quiet", "silent") if r["sc"]["channels"] > 1 else ("normal", "quiet"))
        for kind in kinds:
            for h in (hops if kind == "normal" else hops[:2]):
                if drawn and (h > 1 or (h == 1 and (i, kind) != (0, "normal"))):
                    continue
                pairs.append((h, stream(kind, name, h) if h else None, stream(kind, name, h + 1)))
    assert len(streams) <= 16, (row, len(streams))
    assert not drawn or all(sa is None or (sa, sb) == (0, 1) for _, sa, sb in pairs), row
    return streams, pairs


def _configure(sc, channels):
    if sc["preset"] == "default":
        return lambda r: r.presetDefault(channels, sc["sample_rate"])
    if sc["preset"] == "cheaper":
        return lambda r: r.presetCheaper(channels, sc["sample_rate"], split=False)
    return lambda r: r.configure(channels, sc["block"], sc["interval"])


def measure_yardstick(ref, M, channels, tier, limit=None, hops=(0, 2, 9)):
    """float32 local formula against float64 at one shape on the checker's operands -- no product code -- over the rows of that shape, their
    parameter sets and signals and the tier's time factors: the worst kappa-normalised figure, and the shares the caps are about
    (excused bins; Tier B: bins with an allowance above ALLOWANCE_LARGE; the quiet stream's fallback and normal shares)."""
    limit = bound(M, channels, tier) if limit is None else limit
    rows = [r for r in ROWS.values() if (r["sc"]["bands"], r["sc"]["channels"]) == (M, channels) and (tier == "A" or r["tier_b"])]
    sc = rows[0]["sc"]
    sets = sorted({name for r in rows for name in r["sets"]})
    kinds = ("normal", "quiet", "silent") if channels > 1 else ("normal", "quiet")
    fig = dict(yardstick=0.0, excused=0.0, allowance_share=0.0, fallback=None, normal=None, silent_bins=0)
    counts = np.zeros(3)  # excused bins, bins with a large allowance, bins with energy: over the whole case
    for name in sets:
        p = fs.PARAMS[name]
        for kind in (kinds if name == "none" else ("normal",)):
            for tf_name in (TIER_A if tier == "A" else TIER_B):
                for h in (hops if kind == "normal" else hops[:2]):
                    g, a, b, x, r = checker_pair(ref, lambda r: Geometry(r, channels), channels, p, kind, tf_name, h, configure=_configure(sc, channels))
                    assert g.M == M
                    op = operands(g, a, b, p.mapped, tf_name, 0, WARMUP_HOPS + h, x, r.window() if tier == "B" else None)
                    r64 = evaluate(op, np.float64)
                    share = _shares(op, r64, limit)
                    counts += np.array([share["excused"], share["allowance_large"], 1.0])*share["bins"]
                    if kind == "quiet":
                        fig["fallback"] = min(share["fallback"], 1.0 if fig["fallback"] is None else fig["fallback"])
                        fig["normal"] = min(share["normal"], 1.0 if fig["normal"] is None else fig["normal"])
                    if kind == "silent":
                        fig["silent_bins"] += int(np.count_nonzero(op.E[1] == 0))
                    op.prev_in_error = 0.0  # (both evaluations see the same previous input)
                    out32 = evaluate(op, np.float32)["out"]
                    d = deviations(op, out32, limit)
                    live = ~np.isnan(d["dev"]) & ~d["excused"][None]
                    if live.any():
                        fig["yardstick"] = max(fig["yardstick"], float(np.max(np.where(live, d["dev"]/d["kappa"][None], 0.0))))
    fig["excused"], fig["allowance_share"] = float(counts[0]/max(counts[2], 1)), float(counts[1]/max(counts[2], 1))
    return fig


def _shares(op, r64, limit):
    """of a hop, from the float64 mirror alone"""
    E = op.E.astype(np.float64)
    live = E.max(axis=0) > 0
    n = max(int(live.sum()), 1)
    clear = 10*limit*r64["kappa"]
    amb = (np.abs(r64["n_m"]/float(NOISE_FLOOR) - 1) <= clear) | ((np.abs(r64["n_c"]/float(NOISE_FLOOR) - 1) <= clear) & (np.arange(E.shape[0])[:, None] != r64["mc"][None])).any(axis=0)
    tied = op.max_channel()[1] >= 0
    weak_any = (r64["weak"] & (E > 0)).any(axis=0)
    return dict(bins=n, excused=float(np.count_nonzero((amb | tied) & live))/n, allowance_large=float(np.count_nonzero((r64["allowance"] > ALLOWANCE_LARGE) & live))/n,
                fallback=float(np.count_nonzero(weak_any & live))/n, normal=float(np.count_nonzero(~weak_any & live))/n)


def assert_caps(fig, label, tier):
    print("%s: %s" % (label, {k: (float("%.3g" % v) if isinstance(v, float) else v) for k, v in fig.items()}))
    assert fig["excused"] <= CAP_EXCUSED, (label, fig)
    if tier == "B":
        assert fig["allowance_share"] <= CAP_ALLOWANCE_SHARE, (label, fig)
    # the fallback must actually run: the quiet stream takes it on at least 5 % of its bins and the normal branch on at least 5 %
    assert fig["fallback"] >= 0.05 and fig["normal"] >= 0.05, (label, fig)


# ---------------------------------------------------------------------------------------------------------------------------------
# The product against the mirror
# ---------------------------------------------------------------------------------------------------------------------------------
_windows = {}


def _window(ref, sc, channels):
    key = (sc["preset"], sc["block"], sc["interval"], sc["sample_rate"])
    if key not in _windows:
        r = ref.RefStretch(0)
        _configure(sc, channels)(r)
        _windows[key] = r.window()
    return _windows[key]


def case_residual(lib, ref, monkeypatch, row, tf_name):
    """One batch of the row's streams through the warm-up call and the measured call at one time factor; every pair's last hop against the
    float64 mirror of its own operands.  Returns the worst figures."""
    pkg = package()
    r = ROWS[row]
    sc, tier = r["sc"], TIME_FACTORS[tf_name][0]
    assert tier == "A" or r["tier_b"], (row, tf_name)
    C = sc["channels"]
    streams, pairs = layout(row, tf_name)
    S = len(streams)
    for k in rf.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("SMST_FFT_TEAMS", "2")
    for k, val in r["env"].items():
        monkeypatch.setenv(k, val)
    counters = tuple(rf.COUNTERS)
    before = {k: pkg.launch_count(k, lib) for k in counters}
    try:
        if sc["preset"]:
            b = pkg.StretchBatch(S, C, preset=sc["preset"], sample_rate=sc["sample_rate"], split=sc["split"], lib=lib)
        else:
            b = pkg.StretchBatch(S, C, block=sc["block"], interval=sc["interval"], split=False, lib=lib)
        try:
            g = Geometry(b, C)
            assert g.M == sc["bands"], (row, g.M)
            adv = TIME_FACTORS[tf_name][1](g.I)
            longest = (WARMUP_HOPS + max(k for _, _, k in streams))*adv
            whole = {kind: signal(kind, C, longest, g.N) for kind in {kind for kind, _, _ in streams}}  # (partners share their signal sample by sample)
            xs = [whole[kind][:, :(WARMUP_HOPS + k)*adv] for kind, _, k in streams]
            for s, (_, name, _) in enumerate(streams):
                fs.PARAMS[name].apply(b, stream=s)
            warm = np.stack([x[:, :WARMUP_HOPS*adv] for x in xs])
            b.process(warm, WARMUP_HOPS*g.I)
            after_warmup = [product_state(b, s) for s in range(S)]
            hops = np.array([k for _, _, k in streams], np.int32)
            xin = np.zeros((S, C, int(hops.max())*adv), np.float32)
            for s, x in enumerate(xs):
                xin[s, :, :hops[s]*adv] = x[:, WARMUP_HOPS*adv:]
            b.process(xin, hops*g.I, in_samples=hops*adv)
            state = [product_state(b, s) for s in range(S)]
        finally:
            b.close()
    finally:
        for k in rf.SWITCHES:
            monkeypatch.delenv(k, raising=False)
    grew = {k: pkg.launch_count(k, lib) - before[k] for k in counters}
    label = "%s, %s" % (row, tf_name)
    shows = r["shows"]
    if tf_name == "2.5x" and C <= 2 and "vocoder_across" not in shows and "vocoder_one" not in shows and "chain_unfused" not in shows:
        shows = ("vocoder_gather",)  # drawn time factors: the gathering producers
    if tier == "B" and row == "default_48k" and tf_name != "2.5x":
        shows = shows + ("vocoder_twisted",)
    assert all(grew[k] > 0 for k in shows), (label, shows, {k: v for k, v in grew.items() if v})
    assert row != "default_48k_no_twist" or grew["vocoder_twisted"] == 0, (label, grew)
    limit = bound(g.M, C, tier)
    window = _window(ref, sc, C) if tier == "B" else None
    fig, excused, bins = {}, 0, 0
    for h, sa, sb in pairs:
        kind, name, _ = streams[sb]
        a = after_warmup[sb] if sa is None else state[sa]
        op = operands(g, a, state[sb], fs.PARAMS[name].mapped, tf_name, sb, WARMUP_HOPS + h, xs[sb], window)
        if kind == "normal":
            assert np.abs(op.out).max() > 0, (label, h, "no output")
        d = assert_within(op, state[sb]["output"], limit, "%s, h = %d, stream %d (%s, %s)" % (label, h, sb, kind, name), fig)
        excused += int(np.count_nonzero(d["excused"]))
        bins += g.M
    fig["excused"] = excused/max(bins, 1)
    print("%s: %d pairs, bound %.2e, worst %s" % (label, len(pairs), limit, {k: float("%.3g" % v) for k, v in fig.items()}))
    assert fig["excused"] <= CAP_EXCUSED, (label, fig)
    return fig
