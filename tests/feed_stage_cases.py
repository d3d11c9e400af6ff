"""The feed stage (csrc/smst_feed.hip: channel-summed energy, its smoothing, the peak list, the output map, the formant envelope, the pitch
estimate and the per-bin energy ratio) against a plain numpy mirror of the reference's steps, in every form launchFeed chooses among.

The FFT is taken out of the comparison: after every hop the product's own Band.input (debug_state(s, 0)) is read back, the mirror evaluates
the feed stage from exactly those float32 values in float64, and what the kernels made of the same values is compared with it: the output
map (debug_map), Prediction.energy (debug_state(s, 3): the map, the ratio and the interpolation together, observable in every form) and,
under SMST_NO_FEED_FUSION=1, the envelope, the ratio and the estimate themselves (debug_formants).  Only the feed arithmetic differs, so
the bounds are a small multiple of float32 rounding, and the discrete decisions that a rounding can flip are found IN THE MIRROR and
excused bin by bin (a clearance), not by an agreement rate.

What the product does not report -- the energies, the smoothed energies and the peak list stay in LDS -- is pinned indirectly: a run that
starts or ends one bin off, a peak more or less, moves its centroid, and with it every map entry of the two segments next to it, by far
more than the bound on inputBin.  The mirror itself is pinned against the checker (check_mirror: peak runs exactly, everything else to a few
ulp), with the float32 instance of the same code.

TOLERANCES.  The yardstick of a continuous quantity is the reference's own float32 rounding: the mirror run with dtype=float32, in the
reference's order, against the float64 mirror on the same spectra (measure_yardsticks: numpy spectra of the cases' signals, no product
code), worst bin outside the excused ones, per band count.  The product must stay within MARGIN = 4 times that figure (the scan forms
re-associate the carry entering a chunk; the device contracts a*b + c).  YARDSTICK holds the measured figures, bound() is derived from them
and from nothing else; EXPERIMENTS.md has the table with the product's own worst figures next to them.
  * inputBin is compared in bins, everything else relatively, with a floor of FLOOR_SHARE of the hop's largest value; Prediction.energy is
    compared with the mirror's scaled inputEnergy interpolated at the map UNDER TEST (prediction_at), on every bin, excused or not;
  * a bin with |energy - smoothed|/max(energy, smoothed) < CLEARANCE is TIED; CLEARANCE = 10 x bound("smoothed"), so a kernel inside its
    bound cannot flip an untied decision.  A tied bin excuses the map bins between the outputs of the peaks on either side of it; a peak
    output within bound("inputBin") of an integer excuses that one bin (for the last peak, whose output is truncated as well as rounded
    up, the bin below too);
  * in estimateFrequency a comparison that decides the outcome (a local maximum that could enter the top three, a top-three comparison,
    the 0.1 / 0.01 thresholds of the folding) within CLEARANCE excuses the estimate of that hop and of the stream's later hops, and the
    envelope, ratio and Prediction.energy that depend on it;
  * per case at most CAP_MAP_SHARE of the map bins may be excused and at most one estimating stream in four may lose its estimate: the
    inputs below were chosen so that the float64 mirror alone stays inside both (test_feed_stage_emu.py::test_inputs_stay_within_caps)."""
import hashlib
import math

import numpy as np

import geometry_cases as gc
from conftest import package

MARGIN = 4.0
FLOOR_SHARE = 1e-12
CAP_MAP_SHARE = 0.05
CAP_ESTIMATE_STREAMS = 0.25
HOPS = 8

# band count -> (block, interval): the smallest shapes that reach each form and each boundary of launchFeed / withFeedBins
_COUNTS = gc.band_counts()
BANDS = {
    160: (300, 75),                                        # threads 160..255 of a feed workgroup own no bin
    256: (512, 128),                                       # one bin per thread
    max(m for m in _COUNTS if m <= 4096): None,            # 16 bins per thread: the last <16>
    min(m for m in _COUNTS if m > 4096): None,             # the first <24>
    max(m for m in _COUNTS if m <= 6144): None,            # 24 bins per thread: the last register form (and the last with a one-pass / folded form)
    min(m for m in _COUNTS if m > 6144): None,             # 32 bins per thread, 8192 bands: the LDS form and the bisection
}
BANDS = {M: (g or (2*M, M//2)) for M, g in BANDS.items()}
assert sorted(BANDS) == [160, 256, 4096, 5120, 6144, 8192]
REGISTER_BANDS = 6144  # kFeedRegisterBins*256

# The reference's own float32 rounding, per band count and quantity: float32 mirror against float64 mirror on numpy spectra of the cases'
# signals, the worst bin outside the excused ones over every mix, stream and hop (measure_yardsticks(); EXPERIMENTS.md).  inputBin in
# bins, the others relative.
YARDSTICK = {  # (bands, channels)
    (160, 2): dict(energy=1.35e-07, smoothed=5.01e-07, avgBand=2.31e-07, inputBin=2.55e-05, freqGrad=2.45e-05, envelope=2.18e-06, ratio=2.08e-05, estimate=1.85e-07, prediction=2.07e-05),
    (256, 1): dict(energy=1.14e-07, smoothed=6.04e-07, avgBand=1.98e-07, inputBin=2.42e-05, freqGrad=3.35e-05, envelope=7.24e-06, ratio=1.25e-05, estimate=1.29e-07, prediction=1.12e-05),
    (256, 2): dict(energy=1.50e-07, smoothed=6.09e-07, avgBand=2.22e-07, inputBin=2.98e-05, freqGrad=3.97e-05, envelope=4.16e-06, ratio=1.30e-05, estimate=1.36e-07, prediction=1.09e-05),
    (256, 3): dict(energy=1.49e-07, smoothed=6.03e-07, avgBand=2.38e-07, inputBin=2.59e-05, freqGrad=5.30e-05, envelope=4.04e-06, ratio=1.26e-05, estimate=9.54e-08, prediction=1.17e-05),
    (256, 8): dict(energy=2.26e-07, smoothed=5.92e-07, avgBand=2.54e-07, inputBin=3.17e-05, freqGrad=3.26e-05, envelope=4.06e-06, ratio=1.23e-05, estimate=1.32e-07, prediction=1.31e-05),
    (256, 9): dict(energy=2.48e-07, smoothed=5.82e-07, avgBand=2.01e-07, inputBin=3.24e-05, freqGrad=2.95e-05, envelope=5.29e-06, ratio=1.27e-05, estimate=1.26e-07, prediction=1.03e-05),
    (4096, 2): dict(energy=1.57e-07, smoothed=1.04e-06, avgBand=2.85e-07, inputBin=5.87e-04, freqGrad=7.92e-04, envelope=4.84e-05, ratio=5.08e-04, estimate=1.00e-07, prediction=4.41e-04),
    (5120, 2): dict(energy=1.51e-07, smoothed=1.05e-06, avgBand=2.39e-07, inputBin=9.35e-04, freqGrad=1.28e-03, envelope=1.33e-04, ratio=3.34e-04, estimate=8.18e-08, prediction=3.34e-04),
    (6144, 2): dict(energy=1.47e-07, smoothed=9.93e-07, avgBand=2.25e-07, inputBin=1.13e-03, freqGrad=1.31e-03, envelope=6.70e-05, ratio=2.28e-04, estimate=1.18e-07, prediction=2.28e-04),
    (8192, 2): dict(energy=1.52e-07, smoothed=9.24e-07, avgBand=2.43e-07, inputBin=1.12e-03, freqGrad=1.81e-03, envelope=1.42e-04, ratio=1.42e-04, estimate=1.49e-07, prediction=1.42e-04),
}
QUANTITIES = ("energy", "smoothed", "avgBand", "inputBin", "freqGrad", "envelope", "ratio", "estimate", "prediction")


def bound(M, quantity, channels=2):
    return MARGIN*YARDSTICK[(M, channels)][quantity]


def clearance(M, channels=2):
    return 10*bound(M, "smoothed", channels)


# ---------------------------------------------------------------------------------------------------------------------------------
# Parameters
# ---------------------------------------------------------------------------------------------------------------------------------
def semitones(st):
    return float(np.float32(2.0**(st/12.0)))


class Params:
    """One stream's parameters as the float32 values both implementations hold (signalsmith-stretch.h:107-135): set through the *Factor
    calls, so that no pow() of either side enters."""

    def __init__(self, transpose=None, tonality=0.0, table=None, formant=1.0, compensate=False, base=0.0):
        self.transpose, self.tonality, self.formant, self.compensate, self.base = transpose, tonality, formant, compensate, base
        self.table = None if table is None else np.ascontiguousarray(table, np.float32)
        self.freq_multiplier = np.float32(1.0 if transpose is None else transpose)
        self.tonality_limit = np.float32(0.5) if transpose is None else (np.float32(tonality)/np.sqrt(self.freq_multiplier) if tonality > 0 else np.float32(1.0))
        self.formant_multiplier = np.float32(formant)
        self.inv_formant_multiplier = np.float32(1.0)/np.float32(formant)
        self.base_freq = np.float32(base)
        self.mapped = self.table is not None or self.freq_multiplier != 1
        self.formants = bool(self.formant_multiplier != 1 or (compensate and self.mapped))
        self.estimates = self.formants and not self.base_freq > 0

    def apply(self, obj, **stream):
        """On a StretchBatch (stream=s) or on a checker instance."""
        if self.transpose is not None:
            obj.setTransposeFactor(self.transpose, self.tonality, **stream)
        if self.table is not None:
            obj.setFreqMapTable(self.table, **stream)
        obj.setFormantFactor(self.formant, self.compensate, **stream)
        obj.setFormantBase(self.base, **stream)


def _table(n, seed):
    """A strictly increasing map table of n knots around the identity (knot i at (i + 0.5)/(2n), include/smst.h)."""
    g = np.random.default_rng(seed)
    steps = g.uniform(0.6, 1.5, n)
    centre = (np.arange(n) + 0.5)/(2*n)
    return (np.cumsum(steps)/steps.sum()*0.5*g.uniform(0.8, 1.2) + 0.02*centre).astype(np.float32)


PARAMS = {
    "up12_limit": Params(transpose=semitones(12), tonality=8000/48000),
    "down12": Params(transpose=semitones(-12)),
    "up0.1": Params(transpose=semitones(0.1)),
    "table7": Params(table=_table(7, 7)),
    "table64": Params(table=_table(64, 64)),
    "none": Params(),
    "comp_given": Params(transpose=semitones(4), tonality=8000/48000, compensate=True, base=200/48000),
    "comp_estimated": Params(transpose=semitones(4), tonality=8000/48000, compensate=True),
    "shift_up3": Params(formant=semitones(3), base=150/48000),                                      # invMapFormant below the limit
    "shift_down5_limit": Params(transpose=semitones(2), tonality=0.11, formant=semitones(-5), base=150/48000),  # ... and above it
    "shift_down5_estimated": Params(transpose=semitones(2), tonality=0.11, formant=semitones(-5)),
    "clamp": Params(formant=0.53, base=300/48000),                                                   # target band up to 1.9*bands: getFormant's min(band, bands)
    "clamp_estimated": Params(formant=0.53),
    "table7_comp": Params(table=_table(7, 7), compensate=True, base=200/48000),
}
# A mix = the (parameter set, signal) of each stream of one batch; with 4 streams (above 4096 bands) the first four.  "maps": no formant
# processing anywhere (FEED_PASS_A_FOLDED); "given": formant streams with a base frequency each (FEED_ONE_PASS); "estimated": some estimate
# theirs (FEED_ENVELOPE_PASS_A).  Mapped and unmapped streams share every tile.
MIXES = {
    "maps": (("up12_limit", "partials"), ("table7", "partials"), ("down12", "chirp"), ("up0.1", "silent"),
             ("none", "partials"), ("table64", "partials"), ("up0.1", "partials"), ("down12", "partials")),
    "given": (("comp_given", "partials"), ("shift_down5_limit", "partials"), ("clamp", "chirp"), ("shift_up3", "silent"),
              ("none", "partials"), ("shift_up3", "partials"), ("table7_comp", "partials"), ("up12_limit", "partials")),
    "estimated": (("comp_estimated", "partials"), ("shift_down5_estimated", "partials"), ("comp_estimated", "chirp"), ("comp_estimated", "silent"),
                  ("clamp_estimated", "partials"), ("comp_given", "partials"), ("none", "partials"), ("table64", "partials")),
}


def streams_of(mix, M):
    return MIXES[mix][:4] if M > 4096 else MIXES[mix]


def signals(mix, M, channels, interval, hops=HOPS):
    """[S, C, hops*interval] float32: per stream a harmonic series on a fundamental that is no bin centre, a different level per channel
    (1 - 0.07 c), over a noise floor 40 dB below the strongest partial; one chirp stream; one silent stream."""
    n = hops*interval
    t = np.arange(n, dtype=np.float64)
    N = 2*M
    out = []
    for s, (_, kind) in enumerate(streams_of(mix, M)):
        g = np.random.default_rng(1000*M + 10*s + len(mix) + 1)
        x = np.zeros((channels, n))
        if kind != "silent":
            for c in range(channels):
                if kind == "partials":
                    f0 = ((0.021 + 0.004*s)*M + 0.37 + 0.11*s + 0.5)/N
                    for h, a in ((1, 0.3), (2, 0.2), (3, 0.12), (5, 0.06), (8, 0.03)):
                        x[c] += a*np.sin(2*np.pi*h*f0*t + 0.4*c + h)
                else:
                    f_lo, f_hi = 0.01, 0.37
                    x[c] = 0.3*np.sin(2*np.pi*(f_lo*t + 0.5*(f_hi - f_lo)/n*t*t) + 0.4*c)
                x[c] = (1 - 0.07*c)*x[c] + 0.003*g.standard_normal(n)
        out.append(x)
    return np.asarray(out, np.float32)


# ---------------------------------------------------------------------------------------------------------------------------------
# The mirror: the reference's feed steps (signalsmith-stretch.h: smoothEnergy, findPeaks, updateOutputMap, estimateFrequency, updateFormants
# and the energy of the preliminary prediction), bin after bin in the reference's order, in `dtype` arithmetic.  Columns (stream, hop)
# are independent up to the hop-to-hop smoothing of the estimate, so the loops over the bins carry K columns at a time ([M, K] arrays).
# ---------------------------------------------------------------------------------------------------------------------------------
def map_freq(p, f, T):
    """mapFreq for an array of frequencies: the table form of setFreqMap (knots at (i + 0.5)/(2n), linear in between and beyond) or the
    tonality-limit rule."""
    f = np.asarray(f, T)
    if p.table is not None:
        t = p.table.astype(T)
        n = len(t)
        pos = f*T(2)*T(n) - T(0.5)
        lo = np.clip(np.floor(pos), 0, n - 2).astype(np.int64)
        inside = t[lo] + (t[lo + 1] - t[lo])*(pos - lo.astype(T))
        below = t[0] + (t[1] - t[0])*pos
        above = t[n - 1] + (t[n - 1] - t[n - 2])*(pos - T(n - 1))
        return np.where(pos <= 0, below, np.where(pos >= n - 1, above, inside))
    mult, limit = T(p.freq_multiplier), T(p.tonality_limit)
    return np.where(f > limit, f + (mult - T(1))*limit, f*mult)


def _channel_energies(inputs, T):
    """[K, C, M] complex -> |input|^2 per channel in T."""
    re, im = np.asarray(inputs.real, T), np.asarray(inputs.imag, T)
    return re*re + im*im


def _smooth(en, slew):
    """smoothEnergy: a copy, then (down, up) twice with the state carried through.  en: [M, K]."""
    sm = en.copy()
    M = len(sm)
    e = np.zeros_like(sm[0])
    for _ in range(2):
        for b in range(M - 1, -1, -1):
            e = e + (sm[b] - e)*slew
            sm[b] = e
        for b in range(M):
            e = e + (sm[b] - e)*slew
            sm[b] = e
    return sm


def _envelope(metric, decay):
    """updateFormants' second step: (down, up) twice as a decaying maximum, (down, up) twice as a growing minimum; std::max / std::min keep
    their first argument when the second is not a number (decay = 0 on a silent hop makes 0*inf)."""
    m = metric.copy()
    M = len(m)
    e = np.zeros_like(m[0])
    with np.errstate(all="ignore"):
        for _ in range(2):
            for b in range(M - 1, -1, -1):
                e = np.fmax(m[b], e*decay)
                m[b] = e
            for b in range(M):
                e = np.fmax(m[b], e*decay)
                m[b] = e
        decay = 1/decay
        for _ in range(2):
            for b in range(M - 1, -1, -1):
                e = np.fmin(m[b], e*decay)
                m[b] = e
            for b in range(M):
                e = np.fmin(m[b], e*decay)
                m[b] = e
    return m


def _find_peaks(en, sm, p, N, T):
    """findPeaks of one column: (first bin, last bin, avgBand, output) of every maximal run with energy > smoothed."""
    above = np.concatenate(([False], en > sm, [False]))
    edges = np.flatnonzero(above[1:] != above[:-1])
    first, last = edges[0::2], edges[1::2] - 1
    avg = np.zeros(len(first), T)
    weighted = np.arange(len(en)).astype(T)*en
    for i, (a, z) in enumerate(zip(first, last)):
        avg[i] = np.cumsum(weighted[a:z + 1], dtype=T)[-1]/np.cumsum(en[a:z + 1], dtype=T)[-1]  # (summed bin after bin, from zero)
    out = map_freq(p, (avg + T(0.5))/T(N), T)*T(N) - T(0.5)
    return first, last, avg, np.asarray(out, T)


def _output_map(peaks, M, T):
    """updateOutputMap, in the reference's write order: bottom offset, smoothstep segments, top offset."""
    _, _, inp, out = peaks
    b_all = np.arange(M).astype(T)
    input_bin, grad = b_all.copy(), np.ones(M, T)
    if len(inp) == 0:
        return input_bin, grad
    end = min(M, int(math.ceil(out[0])))
    if end > 0:
        input_bin[:end] = b_all[:end] + (inp[0] - out[0])
        grad[:end] = 1
    with np.errstate(all="ignore"):
        for q in range(1, len(inp)):
            range_scale = T(1)/(out[q] - out[q - 1])
            out_offset = inp[q - 1] - out[q - 1]
            out_scale = inp[q] - out[q] - inp[q - 1] + out[q - 1]
            grad_scale = out_scale*range_scale
            start, end = max(0, int(math.ceil(out[q - 1]))), min(M, int(math.ceil(out[q])))
            if end > start:
                b = b_all[start:end]
                r = (b - out[q - 1])*range_scale
                h = r*r*(T(3) - T(2)*r)
                input_bin[start:end] = b + out_offset + h*out_scale
                grad[start:end] = T(1) + (T(6)*r*(T(1) - r))*grad_scale
    start = max(0, int(out[-1]))
    if start < M:
        input_bin[start:] = b_all[start:] + (inp[-1] - out[-1])
        grad[start:] = 1
    return input_bin, grad


def _raw_estimate(m, T, clear=None):
    """estimateFrequency up to its smoothing: (peakEstimate*weight, weight) from the three highest local maxima of the metric and the two
    modulo folds.  With `clear`: also whether a comparison that decides the outcome was closer than that (relative)."""
    M = len(m)
    mid, lo, hi = m[1:M - 1], m[0:M - 2], m[2:M]
    is_max = ~((mid < lo) | (mid <= hi))
    cand = is_max
    if clear is not None:
        scale = np.maximum(np.maximum(mid, lo), hi)
        near = ((np.abs(mid - lo) < clear*scale) | (np.abs(mid - hi) < clear*scale)) & (scale > 0)
        cand = is_max | near
    def close(a, b):
        return clear is not None and max(a, b) > 0 and abs(a - b) < clear*max(a, b)
    idx = [0, 0, 0]
    for b in np.flatnonzero(is_max) + 1:
        e = m[b]
        if e > m[idx[0]]:
            if e > m[idx[1]]:
                if e > m[idx[2]]:
                    idx = [idx[1], idx[2], b]
                else:
                    idx = [idx[1], b, idx[2]]
            else:
                idx[0] = b
    tied = False
    if clear is not None:
        # The loop is an insertion into a sorted triple that starts as three copies of bin 0: it ends with the three largest of (bin 0 three
        # times, the local maxima).  A rounding changes that outcome only through the order of the four largest candidates, or through the
        # local-maximum decision of a bin as large as the third of them.
        pool = sorted([(float(m[0]), 0)]*3 + [(float(m[b]), int(b)) for b in np.flatnonzero(cand) + 1], key=lambda vb: -vb[0])[:4]
        for (va, ba), (vb, bb) in zip(pool[:-1], pool[1:]):
            tied = tied or (ba != bb and close(va, vb))
        third = float(m[idx[0]])
        tied = tied or bool(np.any(near & (mid >= third*(1 - clear)) & (mid > 0)))
    estimate = int(idx[2])
    tied = tied or close(float(m[idx[1]]), float(m[idx[2]])*0.1)
    if m[idx[1]] > m[idx[2]]*T(0.1):
        diff = abs(estimate - int(idx[1]))
        if diff > estimate//8 and diff < estimate*7//8:
            estimate = estimate % diff
        tied = tied or close(float(m[idx[0]]), float(m[idx[2]])*0.01)
        if m[idx[0]] > m[idx[2]]*T(0.01):
            diff = abs(estimate - int(idx[0]))
            if diff > estimate//8 and diff < estimate*7//8:
                estimate = estimate % diff
    weight = m[idx[2]]
    return T(estimate)*weight, weight, tied


def _ratio(env, p, N, T):
    """updateFormants' third step for one column: the envelope at each bin's formant-mapped frequency (getFormant: nothing below band 0, the
    band clamped to `bands`, entries bands and bands + 1 of the metric zero) over the envelope at the bin."""
    M = len(env)
    metric = np.concatenate((env, np.zeros(2, T)))
    input_f = (np.arange(M).astype(T) + T(0.5))/T(N)
    output_f = map_freq(p, input_f, T) if p.compensate else input_f
    inv, limit, mult = T(p.inv_formant_multiplier), T(p.tonality_limit), T(p.formant_multiplier)
    output_f = np.where(output_f*inv > limit, output_f + (T(1) - mult)*limit, output_f*inv)  # invMapFormant
    band = output_f*T(N) - T(0.5)
    clamped = np.minimum(np.maximum(band, T(0)), T(M))
    fl = np.floor(clamped).astype(np.int64)
    frac = clamped - fl.astype(T)
    target = metric[fl] + (metric[fl + 1] - metric[fl])*frac
    target = np.where(band < 0, T(0), target)
    return np.asarray(target/(env + T(1e-30)), T)


def _prediction_energy(input_energy, input_bin, grad, T):
    """Prediction.energy of one column: inputEnergy [C, M] interpolated at inputBin (nothing outside [0, bands)), times max(0, freqGrad)."""
    C, M = input_energy.shape
    low = np.floor(input_bin)
    frac = input_bin - low
    idx = np.clip(low, -2, M).astype(np.int64)  # (clipped before the conversion: far outside, every tap is zero anyway)
    padded = np.concatenate((np.zeros((C, 1), T), input_energy, np.zeros((C, 1), T)), axis=1)  # bins -1 .. M
    lo, hi = padded[:, np.clip(idx + 1, 0, M + 1)], padded[:, np.clip(idx + 2, 0, M + 1)]
    return (lo + (hi - lo)*frac)*np.maximum(T(0), grad)


def smooth_estimate(state, weighted, weight, T):
    """estimateFrequency's smoothing from hop to hop; state = [freqEstimateWeighted, freqEstimateWeight], updated in place."""
    state[0] = T(state[0]) + (weighted - T(state[0]))*T(0.25)
    state[1] = T(state[1]) + (weight - T(state[1]))*T(0.25)
    with np.errstate(all="ignore"):
        return state[0]/(state[1] + T(1e-30))


def feed_mirror_run(inputs, params, fft_samples, interval, dtype=np.float64, states=None, clear=None):
    """The feed stage of H consecutive hops of S streams.  inputs: Band.input [H, S, C, M] (complex64 values), params: S Params,
    states: per stream [freqEstimateWeighted, freqEstimateWeight] carried from hop to hop (updated in place; from reset when None).
    Returns a dict of [H][S] lists / arrays: energy, smoothed, peaks (first, last, avgBand, output), inputBin, freqGrad, and for formant
    streams estimate, envelope, ratio; scaled (inputEnergy as updateFormants leaves it) and prediction [C, M] always; estimate_tied when
    `clear` is given."""
    T = dtype
    inputs = np.asarray(inputs)
    H, S, C, M = inputs.shape
    N = fft_samples
    states = states if states is not None else [[T(0), T(0)] for _ in range(S)]
    ec = _channel_energies(inputs.reshape(H*S, C, M), T)  # [K, C, M]
    en = np.zeros((H*S, M), T)
    for c in range(C):
        en = en + ec[:, c]
    enT = np.ascontiguousarray(en.T)
    slew = T(1)/(T(1) + (T(N)/T(interval))*T(0.5))
    smT = _smooth(enT, slew)
    sm = np.ascontiguousarray(smT.T)
    res = dict(energy=en.reshape(H, S, M), smoothed=sm.reshape(H, S, M), peaks=[[None]*S for _ in range(H)],
               inputBin=np.zeros((H, S, M), T), freqGrad=np.ones((H, S, M), T), estimate=np.zeros((H, S), T), envelope=np.zeros((H, S, M), T),
               ratio=np.ones((H, S, M), T), scaled=np.zeros((H, S, C, M), T), prediction=np.zeros((H, S, C, M), T), estimate_tied=np.zeros((H, S), bool))
    # the maps
    for h in range(H):
        for s, p in enumerate(params):
            k = h*S + s
            if p.mapped:
                res["peaks"][h][s] = _find_peaks(en[k], sm[k], p, N, T)
                res["inputBin"][h, s], res["freqGrad"][h, s] = _output_map(res["peaks"][h][s], M, T)
            else:
                res["inputBin"][h, s] = np.arange(M).astype(T)
    # the estimates, smoothed from hop to hop
    for s, p in enumerate(params):
        if not p.formants:
            continue
        for h in range(H):
            if p.estimates:
                weighted, weight, tied = _raw_estimate(en[h*S + s], T, clear)
                res["estimate"][h, s] = smooth_estimate(states[s], weighted, weight, T)
                res["estimate_tied"][h, s] = tied
            else:
                res["estimate"][h, s] = T(p.base_freq)*T(N) - T(0.5)
    # the envelopes of every formant column together, then ratio and prediction
    cols = [(h, s) for h in range(H) for s, p in enumerate(params) if p.formants]
    if cols:
        est = np.array([res["estimate"][h, s] for h, s in cols])
        decay = (1 - 1/(est.astype(np.float64)*0.5 + 1)).astype(T)  # (the reference's 0.5 is a double: one rounding, at the end)
        envT = _envelope(np.ascontiguousarray(np.stack([en[h*S + s] for h, s in cols], axis=1)), decay)
        for i, (h, s) in enumerate(cols):
            res["envelope"][h, s] = envT[:, i]
            with np.errstate(all="ignore"):
                res["ratio"][h, s] = _ratio(np.ascontiguousarray(envT[:, i]), params[s], N, T)
    for h in range(H):
        for s, p in enumerate(params):
            res["scaled"][h, s] = ec[h*S + s]*res["ratio"][h, s] if p.formants else ec[h*S + s]
            res["prediction"][h, s] = _prediction_energy(res["scaled"][h, s], res["inputBin"][h, s], res["freqGrad"][h, s], T)
    return res


def feed_mirror(band_input, params, state, fft_samples, interval, dtype=np.float64):
    """One hop of one stream: Band.input [C, M], the stream's Params, the carried [freqEstimateWeighted, freqEstimateWeight]."""
    r = feed_mirror_run(np.asarray(band_input)[None, None], [params], fft_samples, interval, dtype, [state])
    return {k: v[0][0] for k, v in r.items()}


# ---------------------------------------------------------------------------------------------------------------------------------
# Excuses (found in the float64 mirror) and deviations
# ---------------------------------------------------------------------------------------------------------------------------------
def excused_bins(res, h, s, M, clear, bin_bound):
    """Map bins of column (h, s) that a decision closer than `clear` (or a peak output within bin_bound of an integer) may move."""
    ex = np.zeros(M, bool)
    pk = res["peaks"][h][s]
    if pk is None:
        return ex, 0
    first, last, _, out = pk
    en, sm = res["energy"][h, s], res["smoothed"][h, s]
    top = np.maximum(en, sm)
    tied = np.flatnonzero((top > 0) & (np.abs(en - sm) < clear*top))
    for t in tied:
        i = int(np.searchsorted(last, t, "left")) - 1  # the peak below: its run ends before t
        j = int(np.searchsorted(first, t, "right"))    # the peak above: its run starts after t
        lo = 0 if i < 0 else max(0, int(math.floor(out[i] - bin_bound)))
        hi = M if j >= len(first) else min(M, int(math.ceil(out[j] + bin_bound)))
        ex[lo:max(lo, hi)] = True
    for q, o in enumerate(out):
        n = int(round(float(o)))
        if abs(float(o) - n) < bin_bound:
            for b in ((n - 1, n) if q == len(out) - 1 else (n,)):
                if 0 <= b < M:
                    ex[b] = True
    return ex, len(tied)


def relative(got, want):
    """|got - want| relative to |want|, floored at FLOOR_SHARE of the largest |want| (of the hop)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    floor = max(FLOOR_SHARE*float(np.abs(want).max(initial=0.0)), 1e-300)
    with np.errstate(all="ignore"):
        return np.abs(got - want)/np.maximum(np.abs(want), floor)


def prediction_at(res64, h, s, input_bin, grad):
    """Prediction.energy of column (h, s) from the float64 mirror's scaled inputEnergy, interpolated at the map under test (its own float32
    inputBin and freqGrad, taken exactly).  The map has its own bounds; Prediction.energy is ill-conditioned in it without limit (inputBin
    just above a bin whose neighbour is 60 dB stronger, or just below `bands`, where the upper tap is nothing: 1e-3 bins are 100 % there),
    so against the mirror's own map its worst bin is decided by where the noise floor puts such a bin, not by the arithmetic."""
    return _prediction_energy(res64["scaled"][h, s], np.asarray(input_bin, np.float64), np.asarray(grad, np.float64), np.float64)


def _worst(fig, key, values, mask=None):
    values = np.asarray(values, np.float64)
    if mask is not None:
        values = values[~mask]
    if values.size:
        fig[key] = max(fig.get(key, 0.0), float(np.nanmax(values)) if not np.all(np.isnan(values)) else float("inf"))


def analyse(res64, params, M, clear, bin_bound):
    """The excuses of a run of the float64 mirror: per (hop, stream) the excused map bins and whether the estimate is still trusted, the
    shares against their caps."""
    H, S = res64["estimate"].shape
    ex = np.zeros((H, S, M), bool)
    lost = np.zeros((H, S), bool)
    tied = np.zeros((H, S), int)
    for s, p in enumerate(params):
        gone = False
        for h in range(H):
            ex[h, s], tied[h, s] = excused_bins(res64, h, s, M, clear, bin_bound)
            gone = gone or bool(res64["estimate_tied"][h, s])
            lost[h, s] = gone and p.estimates
    mapped = [s for s, p in enumerate(params) if p.mapped]
    estimating = [s for s, p in enumerate(params) if p.estimates]
    shares = dict(map_share=float(ex[:, mapped].mean()) if mapped else 0.0,
                  estimate_streams=float(np.mean([lost[-1, s] for s in estimating])) if estimating else 0.0,
                  tied_bins=tied)
    return ex, lost, shares


def assert_caps(shares, label):
    print("%s: excused share of the map bins %.4f (<= %.2f), streams that lost their estimate %.2f (<= %.2f)" % (
        label, shares["map_share"], CAP_MAP_SHARE, shares["estimate_streams"], CAP_ESTIMATE_STREAMS))
    assert shares["map_share"] <= CAP_MAP_SHARE, (label, shares)
    assert shares["estimate_streams"] <= CAP_ESTIMATE_STREAMS, (label, shares)


def mirror_deviations(res, res64, params, ex, lost, tied):
    """Worst deviation of a second mirror run (float32: the yardstick) from the float64 one, per quantity, outside the excuses."""
    fig = {}
    H, S = lost.shape
    for h in range(H):
        for s, p in enumerate(params):
            _worst(fig, "energy", relative(res["energy"][h, s], res64["energy"][h, s]))
            if p.mapped:
                _worst(fig, "smoothed", relative(res["smoothed"][h, s], res64["smoothed"][h, s]))
                a, b = res["peaks"][h][s], res64["peaks"][h][s]
                if not tied[h, s]:
                    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), ("peak runs differ without a tie", h, s)
                    if len(a[2]):
                        _worst(fig, "avgBand", relative(a[2], b[2]))
                _worst(fig, "inputBin", np.abs(res["inputBin"][h, s].astype(np.float64) - res64["inputBin"][h, s]), ex[h, s])
                _worst(fig, "freqGrad", relative(res["freqGrad"][h, s], res64["freqGrad"][h, s]), ex[h, s])
            if p.formants and not lost[h, s]:
                _worst(fig, "envelope", relative(res["envelope"][h, s], res64["envelope"][h, s]))
                _worst(fig, "ratio", relative(res["ratio"][h, s], res64["ratio"][h, s]))
                _worst(fig, "estimate", relative(res["estimate"][h, s], res64["estimate"][h, s]))
            if not lost[h, s]:
                _worst(fig, "prediction", relative(res["prediction"][h, s], prediction_at(res64, h, s, res["inputBin"][h, s], res["freqGrad"][h, s])))
    return fig


# ---------------------------------------------------------------------------------------------------------------------------------
# The yardstick: float32 against float64 on spectra that no product code has touched
# ---------------------------------------------------------------------------------------------------------------------------------
def numpy_spectra(mix, M, channels, hops=HOPS):
    """Band.input-like spectra [H, S, C, M] (complex64) of the case's signals: a Hann window over the block that ends at each hop, the
    modified DFT of geometry_cases in float64, rounded to float32."""
    block, interval = BANDS[M]
    x = signals(mix, M, channels, interval, hops)
    w = (0.5 - 0.5*np.cos(2*np.pi*(np.arange(block) + 0.5)/block)).astype(np.float32)
    out = np.zeros((hops, x.shape[0], channels, M), np.complex64)
    for k in range(hops):
        for s in range(x.shape[0]):
            out[k, s] = gc.dft_spectrum(gc._block_ending(x[s], k*interval, block), w, 2*M).astype(np.complex64)
    return out


def measure_yardsticks(M, channels=2, mixes=tuple(MIXES), clear=None, bin_bound=None):
    """float32 mirror against float64 mirror at one band count: worst figures per quantity over the mixes, and the excused shares of the
    float64 mirror alone.  `clear` / `bin_bound`: the clearances to excuse with (the constants' own when None)."""
    clear = clearance(M, channels) if clear is None else clear
    bin_bound = bound(M, "inputBin", channels) if bin_bound is None else bin_bound
    block, interval = BANDS[M]
    worst, shares = {}, {}
    for mix in mixes:
        params = [PARAMS[name] for name, _ in streams_of(mix, M)]
        spectra = numpy_spectra(mix, M, channels)
        r64 = feed_mirror_run(spectra, params, 2*M, interval, np.float64, clear=clear)
        r32 = feed_mirror_run(spectra, params, 2*M, interval, np.float32)
        ex, lost, shares[mix] = analyse(r64, params, M, clear, bin_bound)
        for k, v in mirror_deviations(r32, r64, params, ex, lost, shares[mix]["tied_bins"]).items():
            worst[k] = max(worst.get(k, 0.0), v)
    return worst, shares


# ---------------------------------------------------------------------------------------------------------------------------------
# The mirror against the checker
# ---------------------------------------------------------------------------------------------------------------------------------
ULPS = 8*2.0**-24  # the float32 mirror and the checker run the same operations in the same order: a few ulp for the compiler's freedom


def check_mirror(ref, hops=7, channels=2, block=512, interval=128):
    """Pins the mirror before it judges anything: a few hops at 256 bands on the checker, and the float32 mirror, fed with the checker's own
    Band.input, against the checker's peak list (runs exactly), energies, output map, envelope, estimate, scaled inputEnergy and
    Prediction.energy.  The port restates none of these members: there only the mirror's own sanity checks run."""
    T = np.float32
    # (the identity: no peak gives the identity map, silence gives no peak and a zero ratio)
    M = 64
    silent = feed_mirror(np.zeros((2, M), np.complex64), PARAMS["comp_estimated"], [0.0, 0.0], 2*M, M//2)
    assert np.array_equal(silent["inputBin"], np.arange(M)) and np.all(silent["freqGrad"] == 1) and np.all(silent["ratio"] == 0) and len(silent["peaks"][0]) == 0
    if getattr(ref, "is_port", False):
        return None
    compared = 0
    for name in ("up12_limit", "down12", "table7", "table64", "comp_given", "comp_estimated", "shift_up3", "shift_down5_limit", "clamp", "none", "table7_comp"):
        p = PARAMS[name]
        r = ref.RefStretch(0)
        r.configure(channels, block, interval)
        p.apply(r)
        M, N = r.bands(), r.fftSamples()
        x = signals("maps", M, channels, interval, hops)[0]
        state = [T(0), T(0)]
        for k in range(hops):
            r.process(x[:, k*interval:(k + 1)*interval], interval)
            band_input = r.bands_complex(0).astype(np.complex64)
            got = feed_mirror(band_input, p, state, N, interval, T)
            where = "%s, hop %d" % (name, k)
            raw_energy = _channel_energies(band_input[None], T)[0]
            if p.mapped:
                energy, smoothed = r.energy()
                assert np.array_equal(got["energy"], energy), where
                assert np.all(relative(got["smoothed"], smoothed) <= ULPS), (where, float(relative(got["smoothed"], smoothed).max()))
                peaks = r.peaks()
                first, last, avg, out = got["peaks"]
                assert len(peaks) == len(first), (where, len(peaks), len(first))
                if len(first):
                    above = energy > smoothed
                    assert above[first].all() and above[last].all() and not above[np.maximum(first - 1, 0)][first > 0].any() and not above[np.minimum(last + 1, M - 1)][last < M - 1].any(), where
                    assert np.all(relative(avg, peaks[:, 0]) <= ULPS) and np.all(np.abs(out - peaks[:, 1]) <= ULPS*M), where
            ref_map = r.output_map()
            assert np.all(np.abs(got["inputBin"] - ref_map[:, 0]) <= 4*ULPS*M), (where, float(np.abs(got["inputBin"] - ref_map[:, 0]).max()))
            assert np.all(np.abs(got["freqGrad"] - ref_map[:, 1]) <= 1e-4*np.maximum(1, np.abs(ref_map[:, 1]))), (where, float(np.abs(got["freqGrad"] - ref_map[:, 1]).max()))
            scaled = r.bands_real(3)
            if p.formants:
                metric, est = r.formant_metric()
                assert len(metric) == M + 2 and not metric[M:].any(), where
                assert abs(got["estimate"] - est) <= ULPS*max(1.0, abs(est)), (where, got["estimate"], est)
                assert np.all(relative(got["envelope"], metric[:M]) <= 4*ULPS), (where, float(relative(got["envelope"], metric[:M]).max()))
                assert np.all(relative(raw_energy*got["ratio"], scaled) <= 1e-4), (where, float(relative(raw_energy*got["ratio"], scaled).max()))
            else:
                assert np.array_equal(raw_energy, scaled), where
            pred = r.bands_real(4)
            assert np.all(relative(got["prediction"], pred) <= 1e-3), (where, float(relative(got["prediction"], pred).max()))
            compared += 1
    return compared


# ---------------------------------------------------------------------------------------------------------------------------------
# The product against the mirror
# ---------------------------------------------------------------------------------------------------------------------------------
MODES = {"default": {}, "separate": {"SMST_NO_FEED_FUSION": "1"}, "serial": {"SMST_FEED_SERIAL": "1"}}
_mirrors = {}  # the float64 mirror of a case's spectra: the forms of the feed stage see the same Band.input, so they share it


def _mirror_of(key, inputs, params, N, interval, M, channels):
    digest = hashlib.sha1(np.ascontiguousarray(inputs).tobytes()).hexdigest()
    if (key, digest) not in _mirrors:
        r64 = feed_mirror_run(inputs, params, N, interval, np.float64, clear=clearance(M, channels))
        _mirrors[(key, digest)] = (r64,) + analyse(r64, params, M, clearance(M, channels), bound(M, "inputBin", channels))
    return _mirrors[(key, digest)]


def case_feed_stage(lib, monkeypatch, M, mix, mode, channels=2, split=False, hops=HOPS):
    """One batch of the mix's streams at M bands, fed hop by hop from reset in the given form of the feed stage; after every hop every
    stream's map, Prediction.energy and (mode "separate") envelope, ratio and estimate against the float64 mirror of the product's own
    Band.input.  Returns the worst figures per quantity and the excused shares."""
    pkg = package()
    for key in ("SMST_NO_FEED_FUSION", "SMST_FEED_SERIAL"):
        monkeypatch.delenv(key, raising=False)
    for key, v in MODES[mode].items():
        monkeypatch.setenv(key, v)
    block, interval = BANDS[M]
    names = streams_of(mix, M)
    params = [PARAMS[name] for name, _ in names]
    S = len(params)
    x = signals(mix, M, channels, interval, hops)
    counters = ("feed_one_pass", "chain_unfused")
    before = {k: pkg.launch_count(k, lib) for k in counters}
    b = pkg.StretchBatch(S, channels, block=block, interval=interval, split=split, lib=lib)
    try:
        assert b.bands() == M and b.intervalSamples() == interval, (b.bands(), M)
        N = b.fftSamples()
        for s, p in enumerate(params):
            p.apply(b, stream=s)
        inputs = np.zeros((hops, S, channels, M), np.complex64)
        maps, preds, forms = [], [], []
        for k in range(hops):
            b.process(np.ascontiguousarray(x[:, :, k*interval:(k + 1)*interval]), interval)
            for s in range(S):
                inputs[k, s] = b.debug_state(s, 0)
            maps.append([b.debug_map(s) for s in range(S)])
            preds.append([b.debug_state(s, 3) for s in range(S)])
            forms.append([b.debug_formants(s) for s in range(S)])
    finally:
        b.close()
        for key in MODES[mode]:
            monkeypatch.delenv(key, raising=False)
    grew = {k: pkg.launch_count(k, lib) - before[k] for k in counters}
    label = "%d bands, %d ch, %s, %s%s" % (M, channels, mix, mode, ", split" if split else "")
    one_pass = mode == "default" and mix == "given" and M <= REGISTER_BANDS
    assert (grew["feed_one_pass"] > 0) == one_pass, (label, "feed_one_pass", grew)
    assert (grew["chain_unfused"] > 0) == (channels > 8), (label, "chain_unfused", grew)
    assert np.abs(inputs[-1]).max() > 0, label
    r64, ex, lost, shares = _mirror_of((M, mix, channels, split), inputs, params, N, interval, M, channels)
    assert_caps(shares, label)
    fig, failures = {}, []

    def check(key, values, limit, where, mask=None):
        values = np.asarray(values, np.float64)
        kept = values if mask is None else values[~mask]
        if kept.size == 0:
            return
        w = float(kept.max()) if np.isfinite(kept).all() else float("inf")
        fig[key] = max(fig.get(key, 0.0), w)
        if not w <= limit:
            at = int(np.argmax(np.where(mask, -1.0, values) if mask is not None else values))
            failures.append("%s %s: %s %.3e > %.3e (flat index %d)" % (label, where, key, w, limit, at))
    for k in range(hops):
        for s, p in enumerate(params):
            where = "stream %d (%s, %s) hop %d" % (s, names[s][0], names[s][1], k)
            got_map = maps[k][s]
            assert (got_map is None) == (not p.mapped), (label, where, "debug_map() is None exactly when the stream has no map")
            if p.mapped:
                check("inputBin", np.abs(got_map[:, 0].astype(np.float64) - r64["inputBin"][k, s]), bound(M, "inputBin", channels), where, ex[k, s])
                check("freqGrad", relative(got_map[:, 1], r64["freqGrad"][k, s]), bound(M, "freqGrad", channels), where, ex[k, s])
                if names[s][1] == "silent":
                    assert np.array_equal(got_map[:, 0], np.arange(M, dtype=np.float32)) and np.all(got_map[:, 1] == 1), (label, where, "identity map on silence")
            reported = forms[k][s]
            assert (reported is not None) == (mode == "separate" and p.formants), (label, where, "debug_formants", reported is not None)
            if reported is not None and not lost[k, s]:
                ratio, envelope, estimate = reported
                check("envelope", relative(envelope, r64["envelope"][k, s]), bound(M, "envelope", channels), where)
                check("ratio", relative(ratio, r64["ratio"][k, s]), bound(M, "ratio", channels), where)
                check("estimate", relative(estimate, r64["estimate"][k, s]), bound(M, "estimate", channels), where)
            if not lost[k, s]:
                at = (got_map[:, 0], got_map[:, 1]) if p.mapped else (np.arange(M), np.ones(M))
                check("prediction", relative(preds[k][s], prediction_at(r64, k, s, *at)), bound(M, "prediction", channels), where)
    print("%s: worst %s" % (label, {k: float("%.2e" % v) for k, v in fig.items()}))
    assert not failures, "%d failures, the first: %s" % (len(failures), "\n".join(failures[:5]))
    return fig, shares
