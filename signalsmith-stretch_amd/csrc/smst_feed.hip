// The feed-forward passes over a hop's spectrum (K2b-e: energies, smoothing, peaks, frequency map, formant envelope) and their launcher.
#include "smst_recurrence.h"

namespace smst {

// ------------------------------------------------------------------------------------------------------
// K2b-e: channel-summed energy, 4-pass one-pole smoothing, peak centroids, output map, formant envelope and ratio
// (signalsmith-stretch.h:818-848, :859-880, :882-917, :929-966, :972-1036).  All of these are recurrences over the
// bin index; the reference's rounding is kept by evaluating them serially IN THE REFERENCE'S ORDER -- the
// parallel axis is (stream, hop): one wave per stream, lane k = hop k of the tile, scratch arrays laid out
// [bin][64 hops] so that every serial step of the wave is one coalesced 256-byte access.
//   kFeedEnergy : energyT[s][b][k] = sum_c |input_c[b]|^2           (parallel, LDS-transposed)
//   kFeedSerial : everything else, lanes = hops
// ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void kFeedEnergy(DevBatch d, int sBase, int hopBase) {
	extern __shared__ __attribute__((aligned(16))) unsigned char smemRaw[];
	float *tile = reinterpret_cast<float *>(smemRaw); // [64 hops][65]
	const int s = blockIdx.y, sg = sBase + s;
	const int b0 = blockIdx.x*64;
	const int nh = d.nHops[s];
	if (nh == 0) return;
	const int M = d.M, C = d.C;
	const int lane = threadIdx.x & 63, rq = threadIdx.x >> 6;
	for (int k = rq; k < 64; k += 4) {
		float e = 0;
		const int b = b0 + lane;
		if (k < nh && b < M) {
			const HopDesc hd = d.hops[(size_t)sg*d.hopStride + hopBase + k];
			if (hd.flags & (HOP_MAPPED | HOP_FORMANTS)) {
				for (int c = 0; c < C; ++c) e += cnorm(inputRow(d, hd, s, sg, c)[b]);
			}
		}
		tile[k*65 + lane] = e;
	}
	__syncthreads();
	float *eT = d.energyT + (size_t)s*M*64;
	for (int bq = rq; bq < 64; bq += 4) {
		const int b = b0 + bq;
		if (b < M) eT[(size_t)b*64 + lane] = tile[lane*65 + bq];
	}
}

// ------------------------------------------------------------------------------------------------------
// The steps that the bin-by-bin form (kFeedSerial) and the scan form (kFeedScanA / kFeedScanC) share: one definition each.
// ------------------------------------------------------------------------------------------------------
// The three recurrences over the bins.  step(acc, x) is the reference's formula for one bin; the same bin as a composable map of
// the scan form is  y -> mStep()*y + cOf(x)  (OP 0),  y -> max(cOf(x), mStep()*y)  (OP 1)  or  y -> min(cOf(x), mStep()*y)  (OP 2).
struct Pole { // one-pole smoothing, :837-847
	static constexpr int OP = 0;
	float slew;
	__device__ __forceinline__ float step(float acc, float x) const { return acc + (x - acc)*slew; }
	__device__ __forceinline__ float cOf(float x) const { return slew*x; }
	__device__ __forceinline__ float mStep() const { return 1 - slew; }
};
struct MaxDecay { // the formant envelope's decaying maximum, :987-996
	static constexpr int OP = 1;
	float dk;
	__device__ __forceinline__ float step(float acc, float x) const { return fmaxf(x, acc*dk); }
	__device__ __forceinline__ float cOf(float x) const { return x; }
	__device__ __forceinline__ float mStep() const { return dk; }
};
struct MinGrow { // ... and its growing minimum, :997-1006
	static constexpr int OP = 2;
	float dk;
	__device__ __forceinline__ float step(float acc, float x) const { return fminf(x, acc*dk); }
	__device__ __forceinline__ float cOf(float x) const { return x; }
	__device__ __forceinline__ float mStep() const { return dk; }
};
// The pass sequences, over the thing that runs one pass: run.pass<DOWN, FIRST>(carry, recurrence) -> the value after the pass's last
// bin.  The FIRST pass of a sequence reads the channel-summed energies, the others run in place on its result.
// smoothEnergy, :837-847: (down, up) x 2 with the state carried through
template <typename Run>
__device__ __forceinline__ void smoothingPasses(Run run, float slew) {
	const Pole pole{slew};
	float e = 0;
	e = run.template pass<true, true>(e, pole);
	e = run.template pass<false, false>(e, pole);
	e = run.template pass<true, false>(e, pole);
	e = run.template pass<false, false>(e, pole);
}
// the formant envelope, :984-1006: (down, up) x 2 max-decay, then (down, up) x 2 min-grow, state carried throughout
template <typename Run>
__device__ __forceinline__ void envelopePasses(Run run, float freqEstimate) {
	float decay = 1 - 1/(freqEstimate*0.5f + 1);
	float e = 0;
	const MaxDecay maxDecay{decay};
	e = run.template pass<true, true>(e, maxDecay);
	e = run.template pass<false, false>(e, maxDecay);
	e = run.template pass<true, false>(e, maxDecay);
	e = run.template pass<false, false>(e, maxDecay);
	decay = 1/decay;
	const MinGrow minGrow{decay};
	for (int rep = 0; rep < 2; ++rep) {
		e = run.template pass<true, false>(e, minGrow);
		e = run.template pass<false, false>(e, minGrow);
	}
}

// updateOutputMap's rule for bin b, :882-917: the segments reproduce the reference's write order (top segment written last).
// first / last: the first and the last peak, (prev, next): the pair of consecutive peaks with ceil(prev.out) <= b that lies highest
// (read only between bottomEnd and topStart, with two peaks or more) -- how that pair is found is the caller's.
__device__ __forceinline__ float2 mapSegment(int b, int nPeaks, float2 first, float2 last, float2 prev, float2 next, int topStart, int bottomEnd, int M) {
	float2 mp = make_float2(float(b), 1.0f);
	if (nPeaks > 0) {
		if (b >= topStart) {
			mp = make_float2(b + (last.x - last.y), 1.0f);
		} else if (b < bottomEnd) {
			mp = make_float2(b + (first.x - first.y), 1.0f);
		} else if (nPeaks >= 2) {
			if (b < min(M, (int)ceilf(next.y))) {
				float rangeScale = 1/(next.y - prev.y);
				float outOffset = prev.x - prev.y;
				float outScale = next.x - next.y - prev.x + prev.y;
				float gradScale = outScale*rangeScale;
				float r = (b - prev.y)*rangeScale;
				float h = r*r*(3 - 2*r);
				float outB = b + outOffset + h*outScale;
				float gradH = 6*r*(1 - r);
				mp = make_float2(outB, 1 + gradH*gradScale);
			} // else: not covered by any segment (non-monotonic map only): identity, see DESIGN.md
		}
	}
	return mp;
}

// estimateFrequency() raw part, :929-960: the three highest local maxima of the metric (metric(b) = the channel-summed energy), ties
// to the earlier bin, three copies of bin 0 as the initial entries, then the modulo folding -- compares only, no arithmetic.
// Returns (peakEstimate*e2, e2), the pair that the hop-to-hop smoothing takes.
template <typename Metric>
__device__ __forceinline__ float2 rawPitchEstimate(int M, Metric metric) {
	int p0 = 0, p1 = 0, p2 = 0;
	float e0 = metric(0), e1 = metric(0), e2 = metric(0); // metric at p0, p1, p2
	float em = metric(0), ec = metric(1);                 // metric at b-1, b
	for (int b = 1; b < M - 1; ++b) {
		const float en = metric(b + 1);
		const float e = ec;
		if (!(e < em || e <= en)) {
			if (e > e0) {
				if (e > e1) {
					if (e > e2) { p0 = p1; e0 = e1; p1 = p2; e1 = e2; p2 = b; e2 = e; }
					else { p0 = p1; e0 = e1; p1 = b; e1 = e; }
				} else {
					p0 = b; e0 = e;
				}
			}
		}
		em = ec;
		ec = en;
	}
	int peakEstimate = p2;
	if (e1 > e2*0.1f) {
		int diff = abs(peakEstimate - p1);
		if (diff > peakEstimate/8 && diff < peakEstimate*7/8) peakEstimate = peakEstimate%diff;
		if (e0 > e2*0.01f) {
			int diff2 = abs(peakEstimate - p0);
			if (diff2 > peakEstimate/8 && diff2 < peakEstimate*7/8) peakEstimate = peakEstimate%diff2;
		}
	}
	return make_float2(peakEstimate*e2, e2);
}
// ... and its smoothing from hop to hop, :962-965: one hop's raw pair into the carried (w, wt); the estimate in bins
__device__ __forceinline__ float smoothedPitchEstimate(float &w, float &wt, float pw, float ww) {
	w += (pw - w)*0.25f;
	wt += (ww - wt)*0.25f;
	return w/(wt + 1e-30f);
}

// The energy ratio of bin b, :1018-1033: the envelope at the bin's formant-mapped frequency over the envelope at the bin.
// envelope(b), b < M: the formant envelope (entries M and M+1 of the reference's metric are zero).
template <typename Envelope>
__device__ __forceinline__ float formantRatio(const DevBatch &d, const StreamParams &prm, int sg, int b, int M, float Nf, Envelope envelope) {
	float inputF = (b + 0.5f)/Nf;
	float outputF = prm.formantCompensation ? mapFreqDev(d, prm, sg, inputF) : inputF;
	// invMapFormant, :920-925
	if (outputF*prm.invFormantMultiplier > prm.freqTonalityLimit) outputF = mulAdd2(1 - prm.formantMultiplier, prm.freqTonalityLimit, outputF);
	else outputF = outputF*prm.invFormantMultiplier;
	const float inputE = envelope(b);
	float band = freqToBandDev(outputF, Nf);
	float targetE = 0;
	if (!(band < 0)) { // getFormant, :1009-1016
		band = fminf(band, float(M));
		const int fl = (int)floorf(band);
		const float fr = band - fl;
		const float low = (fl < M) ? envelope(fl) : 0.0f, high = (fl + 1 < M) ? envelope(fl + 1) : 0.0f;
		targetE = low + (high - low)*fr;
	}
	return targetE/(inputE + 1e-30f);
}

// One serial pass over the M bins of a [bin][64]-strided column, software-pipelined: the 16 loads of a chunk are
// independent of the recurrence and are issued together, the recurrence then runs on registers.
template <bool DOWN, typename R>
__device__ __forceinline__ float serialPass(const float *src, float *dst, int M, float e, R rec) {
	// double-buffered: chunk c+1 is fetched before chunk c is reduced, so no memory round trip sits between chunks
	// (src may equal dst: the in-place passes only ever overwrite elements that were already fetched)
	constexpr int U = 16;
	float cur[U], nxt[U];
	auto fetch = [&](float (&x)[U], int c0) {
#pragma unroll
		for (int i = 0; i < U; ++i) {
			const int b = DOWN ? (M - 1 - c0 - i) : (c0 + i);
			const int bc = min(max(b, 0), M - 1);
			x[i] = src[(size_t)bc*64];
		}
	};
	fetch(cur, 0);
	for (int c0 = 0; c0 < M; c0 += U) {
		fetch(nxt, c0 + U); // clamped: past the end it re-reads the last element, which is never used
#pragma unroll
		for (int i = 0; i < U; ++i) {
			const int b = DOWN ? (M - 1 - c0 - i) : (c0 + i);
			if (b >= 0 && b < M) {
				e = rec.step(e, cur[i]);
				dst[(size_t)b*64] = e;
			}
		}
#pragma unroll
		for (int i = 0; i < U; ++i) cur[i] = nxt[i];
	}
	return e;
}
struct SerialPasses { // one lane's column of the [bin][64] scratch arrays
	const float *eT;
	float *sT;
	int M;
	template <bool DOWN, bool FIRST, typename R>
	__device__ __forceinline__ float pass(float e, R rec) const { return serialPass<DOWN>(FIRST ? eT : sT, sT, M, e, rec); }
};

__global__ __launch_bounds__(64) void kFeedSerial(DevBatch d, int sBase, int hopBase) {
	const int s = blockIdx.x, sg = sBase + s, k = threadIdx.x;
	const int nh = d.nHops[s];
	if (nh == 0) return;
	const int M = d.M;
	const float Nf = float(d.N);
	const HopDesc hd = d.hops[(size_t)sg*d.hopStride + hopBase + (k < nh ? k : 0)];
	const bool active = k < nh;
	const bool mapped = active && (hd.flags & HOP_MAPPED), formants = active && (hd.flags & HOP_FORMANTS);
	const StreamParams prm = d.paramsPeaks[sg], prmF0 = d.paramsForm0[sg], prmF2 = d.paramsForm2[sg]; // findPeaks / updateFormants(0) / (2) may see different live values (smst_device.h)
	const float *eT = d.energyT + (size_t)s*M*64 + k;
	float *sT = d.smoothT + (size_t)s*M*64 + k;
	float2 *pk = d.peaksT + (size_t)s*(M/2 + 2)*64 + k;

	if (__any(mapped)) {
		const float smoothingBins = Nf/float(d.I);
		const float slew = 1/(1 + smoothingBins*0.5f);
		smoothingPasses(SerialPasses{eT, sT, M}, slew);
		// findPeaks, :859-880: maximal runs with energy > smoothed, centroid, mapped centre
		int nPeaks = 0;
		bool inRun = false;
		float bandSum = 0, energySum = 0;
		for (int c0 = 0; c0 <= M; c0 += 16) {
			float en16[16], sm16[16];
#pragma unroll
			for (int i = 0; i < 16; ++i) {
				const int b = c0 + i;
				en16[i] = (b < M) ? eT[(size_t)b*64] : 0.0f;
				sm16[i] = (b < M) ? sT[(size_t)b*64] : 0.0f;
			}
#pragma unroll
			for (int i = 0; i < 16; ++i) {
				const int b = c0 + i;
				if (b > M) break;
				const float en = en16[i];
				const bool above = (b < M) && en > sm16[i];
				if (above) {
					if (!inRun) { bandSum = 0; energySum = 0; inRun = true; }
					bandSum += b*en;
					energySum += en;
				} else if (inRun) {
					inRun = false;
					const float avgBand = bandSum/energySum;
					const float avgFreq = (avgBand + 0.5f)/Nf;
					if (mapped) pk[(size_t)nPeaks*64] = make_float2(avgBand, freqToBandDev(mapFreqDev(d, prm, sg, avgFreq), Nf));
					++nPeaks;
				}
			}
		}
		// updateOutputMap, :882-917: p walks up the peaks with b
		if (mapped) {
			float2 *mapRow = d.map + ((size_t)s*d.T + k)*M;
			const float2 first = nPeaks > 0 ? pk[0] : make_float2(0.f, 0.f);
			const float2 lastP = nPeaks > 0 ? pk[(size_t)(nPeaks - 1)*64] : make_float2(0.f, 0.f);
			const int topStart = max(0, (int)lastP.y), bottomEnd = min(M, (int)ceilf(first.y));
			int p = 1;
			float2 prev = first, next = nPeaks > 1 ? pk[64] : first;
			for (int b = 0; b < M; ++b) {
				if (nPeaks >= 2 && b < topStart && b >= bottomEnd) {
					// largest p in [1, nPeaks) with ceil(peaks[p-1].out) <= b
					while (p + 1 < nPeaks && max(0, (int)ceilf(next.y)) <= b) {
						++p;
						prev = next;
						next = pk[(size_t)p*64];
					}
				}
				mapRow[b] = mapSegment(b, nPeaks, first, lastP, prev, next, topStart, bottomEnd, M);
			}
		}
	}

	if (__any(formants)) {
		// updateFormants, :972-1036.  The metric is the channel-summed energy (:974-980).
		const bool autoBase = formants && prmF0.formantBaseFreq <= 0;
		float pw = 0, ww = 0;
		if (__any(autoBase)) {
			const float2 raw = rawPitchEstimate(M, [&](int b) { return eT[(size_t)b*64]; });
			pw = raw.x;
			ww = raw.y;
			if (autoBase) {
				d.est[((size_t)s*d.T + k)*2] = pw;
				d.est[((size_t)s*d.T + k)*2 + 1] = ww;
			}
		}
		float freqEstimate = freqToBandDev(prmF0.formantBaseFreq, Nf); // freqToBand, :982
		if (__any(autoBase)) { // the estimate is smoothed from hop to hop: replay the hops of the tile in order
			float w = d.stFreq[2*sg], wt = d.stFreq[2*sg + 1];
			for (int j = 0; j < 64; ++j) {
				const float pwj = __shfl(pw, j), wwj = __shfl(ww, j);
				const int on = __shfl((int)autoBase, j);
				if (on) {
					const float smoothed = smoothedPitchEstimate(w, wt, pwj, wwj);
					if (j == k) freqEstimate = smoothed;
				}
			}
		}
		envelopePasses(SerialPasses{eT, sT, M}, freqEstimate);
		if (formants) {
			float *ratio = d.ratio + ((size_t)s*d.T + k)*M;
			for (int b = 0; b < M; ++b) ratio[b] = formantRatio(d, prmF2, sg, b, M, Nf, [&](int bb) { return sT[(size_t)bb*64]; });
		}
	}
}

// ------------------------------------------------------------------------------------------------------
// K2b-e, scan form.  The same recurrences, one workgroup per (stream, hop) with the hop's arrays in LDS: every pass over
// the bins is a composition of per-bin maps  y -> m*y + c  (one-pole smoothing),  y -> max(c, m*y)  (formant decay) or
// y -> min(c, m*y)  (formant growth), which are closed under composition.  Each thread composes the maps of its own
// chunk of bins, the chunks' maps are scanned across the workgroup, and each thread then RE-RUNS THE REFERENCE'S SERIAL
// FORMULA over its chunk from the carry it received -- so only the carry entering a chunk is rounded differently from a
// bin-by-bin evaluation (and its influence decays geometrically inside the chunk).  Peak runs are summed by the thread
// that owns the run's first bin, in the reference's order.  The serial form above (kFeedEnergy + kFeedSerial) streams
// five [bin][64] arrays per tile through HBM (10 GB per 64-hop tile of 1024 streams, 4 ms); this form reads the input
// spectra once.
// ------------------------------------------------------------------------------------------------------
struct ScanMap { float m, c; };
template <int OP> __device__ __forceinline__ ScanMap scanIdentity() { return ScanMap{1.0f, OP == 0 ? 0.0f : (OP == 1 ? -INFINITY : INFINITY)}; }
template <int OP> __device__ __forceinline__ float scanApply(ScanMap f, float y) { // OP 0: m*y + c, 1: max(c, m*y), 2: min(c, m*y)
	const float v = f.m*y;
	return OP == 0 ? v + f.c : (OP == 1 ? fmaxf(f.c, v) : fminf(f.c, v));
}
template <int OP> __device__ __forceinline__ ScanMap scanCompose(ScanMap second, ScanMap first) { // second after first
	ScanMap r;
	r.m = second.m*first.m;
	r.c = scanApply<OP>(second, first.c);
	return r;
}
__device__ __forceinline__ ScanMap waveShuffle(ScanMap v, int lane) { return ScanMap{__shfl(v.m, lane), __shfl(v.c, lane)}; }
__device__ __forceinline__ int waveShuffle(int v, int lane) { return __shfl(v, lane); }
// Inclusive scan across the 64 lanes of a wave (Hillis-Steele over lane shuffles): lane l gets combine(v_l, combine(v_l-1, ... v_0))
// -- DOWN: the scan runs from lane 63 towards lane 0.  combine(later, earlier); every lane of the wave must call this.
template <bool DOWN, typename T, typename Combine>
__device__ __forceinline__ T waveScan(T inc, int lane, Combine combine) {
#pragma unroll
	for (int dlt = 1; dlt < 64; dlt <<= 1) {
		const T prev = waveShuffle(inc, DOWN ? min(lane + dlt, 63) : max(lane - dlt, 0));
		if (DOWN ? (lane + dlt <= 63) : (lane >= dlt)) inc = combine(inc, prev);
	}
	return inc;
}
// ... and the exclusive one from it: the scan's value at the lane before this one in scan order, `identity` at the first
template <bool DOWN, typename T>
__device__ __forceinline__ T waveScanBefore(T inc, int lane, T identity) {
	const T ex = waveShuffle(inc, DOWN ? min(lane + 1, 63) : max(lane - 1, 0));
	return lane == (DOWN ? 63 : 0) ? identity : ex;
}

// One pass over src[0..M) in the given direction, result to dst (may alias src); `carry` enters the first bin of the
// pass and the value after the last bin is returned.  rec: the recurrence (Pole, MaxDecay, MinGrow).
// maps: 4 entries of LDS scratch (the wave totals).  All 256 threads must call this.
template <bool DOWN, typename R>
__device__ __forceinline__ float scanPass(const float *src, float *dst, int M, float carry, R rec, ScanMap *maps) {
	constexpr int OP = R::OP;
	const int t = threadIdx.x;
	const int n = (M + 255)/256;              // bins per thread, in pass order
	const int p0 = t*n, p1 = min(M, p0 + n);  // pass positions [p0, p1); position p is bin DOWN ? M-1-p : p
	ScanMap f = scanIdentity<OP>();
	for (int p = p0; p < p1; ++p) {
		ScanMap g; g.m = rec.mStep(); g.c = rec.cOf(src[DOWN ? M - 1 - p : p]);
		f = scanCompose<OP>(g, f);
	}
	// inclusive scan of the chunk maps inside each wave, the wave totals through LDS
	const int lane = t & 63;
	const ScanMap inc = waveScan<false>(f, lane, [](ScanMap later, ScanMap earlier) { return scanCompose<OP>(later, earlier); });
	const ScanMap ex = waveScanBefore<false>(inc, lane, scanIdentity<OP>()); // the composition of the chunks before this one inside the wave
	if (lane == 63) maps[t >> 6] = inc;
	__syncthreads();
	float waveCarry = carry; // value entering this thread's wave
	for (int w = 0; w < (t >> 6); ++w) waveCarry = scanApply<OP>(maps[w], waveCarry);
	float e = scanApply<OP>(ex, waveCarry);
	float total = carry;
	for (int w = 0; w < 4; ++w) total = scanApply<OP>(maps[w], total);
	// the chunk again, with the reference's own formula, from the carry (src may alias dst: every thread reads and then
	// writes only its own chunk, and nobody reads another chunk after the barriers above)
	for (int p = p0; p < p1; ++p) {
		const int b = DOWN ? M - 1 - p : p;
		e = rec.step(e, src[b]);
		dst[b] = e;
	}
	__syncthreads();
	return total;
}

// The same pass with every thread's chunk in REGISTERS.  Thread t owns bins [t*n, t*n + cnt) in both directions (the LDS form
// above partitions by pass position, so an up pass and a down pass give a thread different bins and every pass goes through
// LDS with two barriers and two dependent-latency walks); only the chunk maps cross lanes (shuffles, towards higher lanes for
// an up pass, towards lower lanes for a down pass) and the four wave totals cross waves (LDS, one barrier: the totals of
// consecutive passes use alternate halves of `maps`).  v[i], i < cnt: in = the pass's source, out = its result.
template <bool DOWN, int NMAX, typename R>
__device__ __forceinline__ float scanPassReg(float (&v)[NMAX], int cnt, float carry, R rec, ScanMap *maps) {
	constexpr int OP = R::OP;
	const int t = threadIdx.x, lane = t & 63, w = t >> 6;
	ScanMap f = scanIdentity<OP>();
#pragma unroll
	for (int j = 0; j < NMAX; ++j) {
		const int i = DOWN ? NMAX - 1 - j : j;
		if (i < cnt) { ScanMap g; g.m = rec.mStep(); g.c = rec.cOf(v[i]); f = scanCompose<OP>(g, f); }
	}
	const ScanMap inc = waveScan<DOWN>(f, lane, [](ScanMap later, ScanMap earlier) { return scanCompose<OP>(later, earlier); });
	const ScanMap ex = waveScanBefore<DOWN>(inc, lane, scanIdentity<OP>()); // the chunks before this one in pass order, inside the wave
	if (lane == (DOWN ? 0 : 63)) maps[w] = inc;
	__syncthreads();
	float e = carry, total = carry;
#pragma unroll
	for (int j = 0; j < 4; ++j) {
		const int ww = DOWN ? 3 - j : j; // waves in pass order
		if (DOWN ? (ww > w) : (ww < w)) e = scanApply<OP>(maps[ww], e);
		total = scanApply<OP>(maps[ww], total);
	}
	e = scanApply<OP>(ex, e);
#pragma unroll
	for (int j = 0; j < NMAX; ++j) {
		const int i = DOWN ? NMAX - 1 - j : j;
		if (i < cnt) { e = rec.step(e, v[i]); v[i] = e; }
	}
	return total;
}

// The LDS of a feed workgroup (256 threads, one hop of one stream), feedLdsBytes() on the host.  Regions that are reused once their
// first content is dead have a second name.
constexpr int kFeedPerThread = 256 + 8; // an entry per thread and one per wave, rounded up: the length of `maps` and of `counts`
struct FeedWorkgroup {
	float *en;       // [M] channel-summed energy; the energy ratios once the envelope kernel's pass A follows (formantEnvelopeAndRatio)
	float *sm;       // [M] smoothed energy, then the formant envelope
	float2 *pk;      // [M/2 + 2] peaks (input band, output band); kFeedScanA only
	ScanMap *maps;   // [kFeedPerThread]: 0..3 and 4..7 the wave totals of a pass (consecutive passes alternate), from 8 on see waveMax()
	int *counts;     // [kFeedPerThread]: run starts before each thread's chunk, at 256 + w the total of wave w; kFeedScanA only
	__device__ __forceinline__ FeedWorkgroup(unsigned char *smem, int M, bool withPeaks) {
		en = reinterpret_cast<float *>(smem);
		sm = en + M;
		pk = reinterpret_cast<float2 *>(sm + M);
		maps = reinterpret_cast<ScanMap *>(withPeaks ? pk + M/2 + 2 : pk);
		counts = reinterpret_cast<int *>(maps + kFeedPerThread);
	}
	__device__ __forceinline__ int *cover() const { return reinterpret_cast<int *>(sm); }          // [M] index of the peak pair covering each bin: the smoothed energies are dead after the run sums
	__device__ __forceinline__ int *waveMax() const { return reinterpret_cast<int *>(maps + 8); }  // [4] the waves' maxima of the cover scan
};
static size_t feedLdsBytes(int M, bool withPeaks) {
	const size_t passes = (size_t)2*M*sizeof(float) + kFeedPerThread*sizeof(ScanMap);
	return withPeaks ? passes + (size_t)(M/2 + 2)*sizeof(float2) + kFeedPerThread*sizeof(int) : passes;
}

// The two ways a workgroup runs a pass sequence from wg.en into wg.sm: NMAX > 0 with every thread's chunk in registers between the
// passes, NMAX == 0 through LDS (any M).
template <int NMAX>
struct RegisterPasses {
	float (&v)[NMAX];
	int cnt;
	ScanMap *maps;
	template <bool DOWN, bool FIRST, typename R>
	__device__ __forceinline__ float pass(float e, R rec) const { return scanPassReg<DOWN>(v, cnt, e, rec, DOWN ? maps : maps + 4); }
};
struct LdsPasses {
	const float *en;
	float *sm;
	int M;
	ScanMap *maps;
	template <bool DOWN, bool FIRST, typename R>
	__device__ __forceinline__ float pass(float e, R rec) const { return scanPass<DOWN>(FIRST ? en : sm, sm, M, e, rec, maps); }
};
template <int NMAX, typename Sequence> // sequence(run): smoothingPasses or envelopePasses over `run`
__device__ __forceinline__ void feedPasses(const FeedWorkgroup &wg, int M, Sequence sequence) {
	if constexpr (NMAX > 0) {
		const int t = threadIdx.x, n = (M + 255)/256, cnt = min(max(M - t*n, 0), n);
		float v[NMAX];
#pragma unroll
		for (int i = 0; i < NMAX; ++i) v[i] = (i < cnt) ? wg.en[t*n + i] : 0.0f;
		sequence(RegisterPasses<NMAX>{v, cnt, wg.maps});
#pragma unroll
		for (int i = 0; i < NMAX; ++i) if (i < cnt) wg.sm[t*n + i] = v[i];
		__syncthreads();
	} else {
		sequence(LdsPasses{wg.en, wg.sm, M, wg.maps});
	}
}

// channel-summed energy of one hop into LDS, en[b] = sum_c |input_c[b]|^2 in channel order.  Eight independent loads per
// channel are in flight at a time: the plain loop (one bin per iteration, trip count unknown to the compiler) paid a full
// memory round trip per iteration -- 13 of them per workgroup, 27 % of the kernel (ablation on the GPU: 16.1 -> 11.7 ms
// per step of config 3 with the loads removed).
__device__ __forceinline__ void feedEnergyToLds(const DevBatch &d, const HopDesc &hd, int s, int sg, float *en) {
	const int M = d.M, C = d.C, t = threadIdx.x;
	for (int b0 = t; b0 < M; b0 += 8*256) {
		float acc[8];
#pragma unroll
		for (int i = 0; i < 8; ++i) acc[i] = 0.0f;
		for (int c = 0; c < C; ++c) {
			const float2 *row = inputRow(d, hd, s, sg, c);
			float2 v[8];
#pragma unroll
			for (int i = 0; i < 8; ++i) v[i] = row[min(b0 + 256*i, M - 1)];
#pragma unroll
			for (int i = 0; i < 8; ++i) acc[i] += cnorm(v[i]);
		}
#pragma unroll
		for (int i = 0; i < 8; ++i) if (b0 + 256*i < M) en[b0 + 256*i] = acc[i];
	}
}

// The formant envelope of one hop (envelopePasses over the channel-summed energies in wg.en) and the per-bin energy ratio -- into wg.en in
// place of the energies (FUSE_PE: pass A follows in the same kernel) or to the tile's ratio rows.  One workgroup of 256 threads.
// Shared by kFeedScanC and the one-pass form of kFeedScanA.
template <int NMAX, bool FUSE_PE>
__device__ __forceinline__ void formantEnvelopeAndRatio(const DevBatch &d, const StreamParams &prm, int s, int sg, int k, float freqEstimate, const FeedWorkgroup &wg) {
	const int M = d.M, t = threadIdx.x;
	const float Nf = float(d.N);
	feedPasses<NMAX>(wg, M, [&](auto run) { envelopePasses(run, freqEstimate); });
	float *ratio = d.ratio + ((size_t)s*d.T + k)*M;
	for (int b = t; b < M; b += 256) {
		const float inputE = wg.sm[b];
		const float r = formantRatio(d, prm, sg, b, M, Nf, [&](int bb) { return wg.sm[bb]; });
		if constexpr (FUSE_PE) wg.en[b] = r; // the energies are dead: the ratios take their place in LDS
		else { ratio[b] = r; if (d.envelope) d.envelope[((size_t)s*d.T + k)*M + b] = inputE; }
	}
}

// energy, smoothing, peaks, output map, raw pitch estimate: one workgroup per (hop, stream)
// FUSE_PE: pass A (Prediction.input / .energy rows: feedPredictionRows, smst_recurrence.h) for the hop is folded into this kernel when no hop of
// the tile has formant processing: the thread that has just computed the map entry of a bin forms the bin's (P, E) at once -- the map row is
// not read back (8 B per bin) and the input rows, which this workgroup read a moment ago for the energies, come out of L2
// instead of HBM.  Same arithmetic as kPredictA (smst_vocoder_n.hip): bit-identical entries.  Eight bins per thread in flight.
// FUSE_FORM (tiles WITH formant processing in which no stream estimates its base frequency -- BASELINE config 4 gives 200 Hz): the formant
// envelope, the energy ratio and pass A follow in the SAME kernel, from the channel-summed energies that are still in LDS.  The pitch
// estimate is what forces three kernels otherwise (it is smoothed from hop to hop: a serial walk over the tile's hops, kFeedFreq, between the
// energies and the envelope); with a given base frequency the spectra are read once instead of twice.  Same code (formantEnvelopeAndRatio,
// feedPredictionRows), same values: bit-identical to kFeedScanA + kFeedFreq + kFeedScanC.
template <int NMAX, bool FUSE_PE = false, bool FUSE_FORM = false> // NMAX: bins per thread held in registers during the smoothing passes; 0: through LDS (any M)
__global__ __launch_bounds__(256) void kFeedScanA(DevBatch d, int sBase, int hopBase) {
	static_assert(!FUSE_PE || NMAX > 0, "pass A is folded into the register form only");
	static_assert(!(FUSE_PE && FUSE_FORM), "FUSE_PE: tiles without formant processing; FUSE_FORM: tiles with it");
	extern __shared__ __attribute__((aligned(16))) unsigned char smemRaw[];
	const int k = blockIdx.x, s = blockIdx.y, sg = sBase + s;
	if (k >= d.nHops[s]) return;
	const HopDesc hd = d.hops[(size_t)sg*d.hopStride + hopBase + k];
	const bool mapped = hd.flags & HOP_MAPPED, formants = hd.flags & HOP_FORMANTS;
	if (!mapped && !formants) {
		if constexpr (FUSE_PE || FUSE_FORM) feedPredictionRows(d, hd, s, sg, k, false, [](int bb) { return make_float2(float(bb), 1.0f); }, false, nullptr);
		return;
	}
	const int M = d.M, t = threadIdx.x;
	const float Nf = float(d.N);
	const FeedWorkgroup wg(smemRaw, M, true);
	float *const en = wg.en, *const sm = wg.sm;
	float2 *const pk = wg.pk;
	int *const counts = wg.counts;
	const StreamParams prm = d.paramsPeaks[sg];
	feedEnergyToLds(d, hd, s, sg, en);
	__syncthreads();
	if (mapped) {
		const float smoothingBins = Nf/float(d.I);
		const float slew = 1/(1 + smoothingBins*0.5f);
		feedPasses<NMAX>(wg, M, [&](auto run) { smoothingPasses(run, slew); });
		// findPeaks: every thread counts the runs that START in its chunk, an exclusive scan numbers them, and the owner
		// of a run's first bin sums the run in the reference's order (:866-873)
		const int n = (M + 255)/256, b0 = t*n, b1 = min(M, b0 + n);
		int starts = 0;
		unsigned startMask = 0; // bit i: a run starts at bin b0 + i
		if constexpr (NMAX > 0) { // the chunk's energies and smoothed energies side by side in registers: 2 n independent LDS reads
			bool prevAbove = b0 > 0 && b0 <= M && en[b0 - 1] > sm[b0 - 1];
#pragma unroll
			for (int i = 0; i < NMAX; ++i) {
				const bool above = (b0 + i < b1) && en[min(b0 + i, M - 1)] > sm[min(b0 + i, M - 1)];
				if (above && !prevAbove) { startMask |= 1u << i; ++starts; }
				prevAbove = above;
			}
		} else {
			for (int b = b0; b < b1; ++b) starts += (en[b] > sm[b]) && !(b > 0 && en[b - 1] > sm[b - 1]);
		}
		{ // exclusive prefix sum of the run starts: inside the wave by lane shuffles (a serial 64-entry loop by one lane per wave
			// cost 6 us per workgroup), wave totals through LDS
			const int lane = t & 63;
			const int inc = waveScan<false>(starts, lane, [](int later, int earlier) { return later + earlier; });
			counts[t] = inc - starts;
			if (lane == 63) counts[256 + (t >> 6)] = inc;
		}
		__syncthreads();
		int idx = counts[t];
		for (int w = 0; w < (t >> 6); ++w) idx += counts[256 + w];
		const int nPeaks = counts[256] + counts[257] + counts[258] + counts[259];
		for (int b = b0; b < b1; ++b) {
			if (NMAX > 0 ? ((startMask >> (b - b0)) & 1u) != 0 : ((en[b] > sm[b]) && !(b > 0 && en[b - 1] > sm[b - 1]))) {
				float bandSum = 0, energySum = 0;
				for (int q = b; q < M; q += 4) { // four bins per LDS round trip; the additions stay in the reference's order
					float e4[4], s4[4];
#pragma unroll
					for (int i = 0; i < 4; ++i) { const int qi = min(q + i, M - 1); e4[i] = en[qi]; s4[i] = sm[qi]; }
					bool open = true;
#pragma unroll
					for (int i = 0; i < 4; ++i) {
						open = open && (q + i < M) && e4[i] > s4[i];
						if (open) { bandSum += (q + i)*e4[i]; energySum += e4[i]; }
					}
					if (!open) break;
				}
				const float avgBand = bandSum/energySum;
				const float avgFreq = (avgBand + 0.5f)/Nf;
				pk[idx++] = make_float2(avgBand, freqToBandDev(mapFreqDev(d, prm, sg, avgFreq), Nf));
			}
		}
		__syncthreads();
		// updateOutputMap, :882-917 (mapSegment, as the serial form; the covering pair from the cover array or by bisection)
		float2 *mapRow = d.map + ((size_t)s*d.T + k)*M;
		const float2 first = nPeaks > 0 ? pk[0] : make_float2(0.f, 0.f);
		const float2 lastP = nPeaks > 0 ? pk[nPeaks - 1] : make_float2(0.f, 0.f);
		const int topStart = max(0, (int)lastP.y), bottomEnd = min(M, (int)ceilf(first.y));
		// lo = largest q in [0, nPeaks-2] with max(0, ceil(peaks[q].out)) <= b (only used between bottomEnd and topStart)
		auto mapOf = [&](int b, int lo) { return mapSegment(b, nPeaks, first, lastP, pk[lo], pk[lo + 1], topStart, bottomEnd, M); };
		if constexpr (NMAX > 0) {
			// The covering pair of every bin without a search: every peak marks the bin its segment starts at (LDS atomic max:
			// several peaks may start at one bin, the last one counts), a prefix maximum over the bins spreads the marks.  The
			// bisection it replaces cost ten rounds of nine instructions per bin for a noise spectrum (700 peaks): 5.2 of the
			// kernel's 13 ms per step of config 3.  Same result for ascending peak positions (every map the tonality-limit rule
			// or an ascending table produces); for a descending custom map both are arbitrary.
			int *cover = wg.cover(), *waveMax = wg.waveMax();
			const int cnt = max(b1 - b0, 0), lane = t & 63, w = t >> 6;
#pragma unroll
			for (int i = 0; i < NMAX; ++i) if (i < cnt) cover[b0 + i] = -1;
			__syncthreads();
			for (int q = t; q <= nPeaks - 2; q += 256) {
				const int start = max(0, (int)ceilf(pk[q].y));
				if (start < M) atomicMax(&cover[start], q);
			}
			__syncthreads();
			int c[NMAX], run = -1;
#pragma unroll
			for (int i = 0; i < NMAX; ++i) { if (i < cnt) run = max(run, cover[b0 + i]); c[i] = run; }
			const int inc = waveScan<false>(run, lane, [](int later, int earlier) { return max(later, earlier); });
			int base = waveScanBefore<false>(inc, lane, -1);
			if (lane == 63) waveMax[w] = inc;
			__syncthreads();
			for (int ww = 0; ww < w; ++ww) base = max(base, waveMax[ww]);
#pragma unroll
			for (int i = 0; i < NMAX; ++i) if (i < cnt) cover[b0 + i] = max(c[i], base);
			__syncthreads();
			if constexpr (FUSE_PE) feedPredictionRows(d, hd, s, sg, k, true, [&](int bb) { return mapOf(bb, max(cover[bb], 0)); }, true, nullptr);
			else for (int b = t; b < M; b += 256) mapRow[b] = mapOf(b, max(cover[b], 0)); // coalesced stores
		} else {
			// by bisection; a thread's bins are 256 apart, so eight independent bisections run in lock step
			for (int bb = t; bb < M; bb += 8*256) {
				int lo[8], hi[8];
#pragma unroll
				for (int i = 0; i < 8; ++i) { lo[i] = 0; hi[i] = nPeaks - 2; }
				if (nPeaks >= 2) {
					for (int span = nPeaks - 2; span > 0; span >>= 1) { // ceil(log2(nPeaks - 1)) rounds settle every bisection
						float y[8];
#pragma unroll
						for (int i = 0; i < 8; ++i) y[i] = pk[(lo[i] + hi[i] + 1) >> 1].y;
#pragma unroll
						for (int i = 0; i < 8; ++i) {
							const int mid = (lo[i] + hi[i] + 1) >> 1;
							if (lo[i] < hi[i]) { if (max(0, (int)ceilf(y[i])) <= bb + 256*i) lo[i] = mid; else hi[i] = mid - 1; }
						}
					}
				}
#pragma unroll
				for (int i = 0; i < 8; ++i) if (bb + 256*i < M) mapRow[bb + 256*i] = mapOf(bb + 256*i, max(lo[i], 0));
			}
		}
	}
	if constexpr (FUSE_FORM) {
		// (every stream of the tile has a base frequency: the host's condition for this form)
		__syncthreads(); // the map row is complete (its stores are visible to the workgroup behind the barrier); `sm` / `cover` and the peaks are dead
		if (formants) {
			formantEnvelopeAndRatio<NMAX, true>(d, d.paramsForm2[sg], s, sg, k, freqToBandDev(d.paramsForm0[sg].formantBaseFreq, Nf), wg);
			__syncthreads();
		}
		const float2 *mapRowIn = d.map + ((size_t)s*d.T + k)*M;
		feedPredictionRows(d, hd, s, sg, k, mapped, [&](int bb) { return mapRowIn[bb]; }, false, formants ? en : nullptr);
		return;
	}
	if (formants && d.paramsForm0[sg].formantBaseFreq <= 0) {
		// the raw pitch estimate: a serial walk by one thread (3 k steps)
		__syncthreads();
		if (t == 0) {
			const float2 raw = rawPitchEstimate(M, [&](int b) { return en[b]; });
			d.est[((size_t)s*d.T + k)*2] = raw.x;
			d.est[((size_t)s*d.T + k)*2 + 1] = raw.y;
		}
	}
}

// The pitch estimate is smoothed from hop to hop (:962-965): one thread per stream replays the tile's hops in order
__global__ __launch_bounds__(64) void kFeedFreq(DevBatch d, int sBase, int nStreams, int hopBase) {
	const int s = blockIdx.x*blockDim.x + threadIdx.x;
	if (s >= nStreams) return;
	const int sg = sBase + s, nh = d.nHops[s];
	const StreamParams prm = d.paramsForm0[sg];
	const float Nf = float(d.N);
	float w = d.stFreq[2*sg], wt = d.stFreq[2*sg + 1];
	for (int j = 0; j < nh; ++j) {
		const HopDesc hj = d.hops[(size_t)sg*d.hopStride + hopBase + j];
		float fe = freqToBandDev(prm.formantBaseFreq, Nf); // freqToBand, :982
		if ((hj.flags & HOP_FORMANTS) && prm.formantBaseFreq <= 0) fe = smoothedPitchEstimate(w, wt, d.est[((size_t)s*d.T + j)*2], d.est[((size_t)s*d.T + j)*2 + 1]);
		d.freqEst[(size_t)s*d.T + j] = fe;
	}
}

// formant envelope (2 x (down, up) max-decay, 2 x (down, up) min-grow, :987-1006) and the per-bin energy ratio (:1018-1033)
template <int NMAX, bool FUSE_PE = false> // FUSE_PE: pass A of the tile's hops here (tiles WITH formant processing; the ratios stay in LDS)
__global__ __launch_bounds__(256) void kFeedScanC(DevBatch d, int sBase, int hopBase) {
	extern __shared__ __attribute__((aligned(16))) unsigned char smemRaw[];
	const int k = blockIdx.x, s = blockIdx.y, sg = sBase + s;
	if (k >= d.nHops[s]) return;
	const HopDesc hd = d.hops[(size_t)sg*d.hopStride + hopBase + k];
	if (!(hd.flags & HOP_FORMANTS)) {
		if constexpr (FUSE_PE) {
			const float2 *mapRowIn = d.map + ((size_t)s*d.T + k)*d.M;
			feedPredictionRows(d, hd, s, sg, k, (hd.flags & HOP_MAPPED) != 0, [&](int bb) { return mapRowIn[bb]; }, false, nullptr);
		}
		return;
	}
	const int M = d.M;
	const FeedWorkgroup wg(smemRaw, M, false);
	feedEnergyToLds(d, hd, s, sg, wg.en);
	__syncthreads();
	formantEnvelopeAndRatio<NMAX, FUSE_PE>(d, d.paramsForm2[sg], s, sg, k, d.freqEst[(size_t)s*d.T + k], wg);
	if constexpr (FUSE_PE) {
		__syncthreads();
		const float2 *mapRowIn = d.map + ((size_t)s*d.T + k)*M;
		feedPredictionRows(d, hd, s, sg, k, (hd.flags & HOP_MAPPED) != 0, [&](int bb) { return mapRowIn[bb]; }, false, wg.en);
	}
}

// ------------------------------------------------------------------------------------------------------
// host-side launcher
// ------------------------------------------------------------------------------------------------------
// The forms of the feed stage.  Pass A = the (P, E) rows of the recurrence (kPredictA where no feed kernel does it).
enum FeedForm {
	FEED_SERIAL,            // SMST_FEED_SERIAL=1: kFeedEnergy + kFeedSerial, bin by bin
	FEED_PASS_A_FOLDED,     // tiles without formant processing: kFeedScanA<.., FUSE_PE> does pass A too
	FEED_ONE_PASS,          // formant tiles, every base frequency given: kFeedScanA<.., FUSE_FORM> is the whole stage, ONE pass over the spectra
	FEED_ENVELOPE_PASS_A,   // formant tiles otherwise: kFeedScanA, kFeedFreq, kFeedScanC<.., FUSE_PE> with pass A at its end, the ratios still in LDS
	FEED_SEPARATE,          // kFeedScanA and, with formants, kFeedFreq + kFeedScanC: pass A is left to kPredictA
};
constexpr int kFeedRegisterBins = 24; // bins per thread that the register-resident forms hold (M <= 6144); beyond, through LDS
static FeedForm feedForm(const DevBatch &d, bool anyFormants, bool anyEstimatedBase) {
	const bool inRegisters = divUp(d.M, 256) <= kFeedRegisterBins; // (the folded and the one-pass form exist in registers only)
	if (d.feedSerial) return FEED_SERIAL;
	if (!anyFormants && inRegisters && d.noFeedFusion != 1) return FEED_PASS_A_FOLDED;
	if (anyFormants && !anyEstimatedBase && inRegisters && d.noFeedFusion == 0) return FEED_ONE_PASS;
	if (anyFormants && d.noFeedFusion != 1) return FEED_ENVELOPE_PASS_A; // (SMST_NO_FEED_FUSION=2: this form even where one pass would do)
	return FEED_SEPARATE;
}
// f(NMAX as a compile-time constant) for the first of NMAXS that holds the plan's bins per thread (0: any number, the LDS form)
template <int... NMAXS, typename F>
static void withFeedBins(int M, F f) { (void)(((NMAXS == 0 || divUp(M, 256) <= NMAXS) && (f(std::integral_constant<int, NMAXS>()), true)) || ...); }

// returns true if pass A (the (P, E) rows) has been done here
bool launchFeed(const DevBatch &d, int sBase, int nStreams, int hopBase, int tileHops, bool anyFormants, bool anyEstimatedBase, hipStream_t st) {
	const FeedForm form = feedForm(d, anyFormants, anyEstimatedBase);
	const dim3 hopsByStreams(tileHops, nStreams);
	const size_t ldsA = feedLdsBytes(d.M, true), ldsC = feedLdsBytes(d.M, false);
	switch (form) {
	case FEED_SERIAL:
		hipLaunchKernelGGL(kFeedEnergy, dim3(divUp(d.M, 64), nStreams), dim3(256), 64*65*sizeof(float), st, d, sBase, hopBase);
		hipLaunchKernelGGL(kFeedSerial, dim3(nStreams), dim3(64), 0, st, d, sBase, hopBase);
		return false;
	case FEED_PASS_A_FOLDED:
		withFeedBins<16, 24>(d.M, [&](auto nmax) { hipLaunchKernelGGL((kFeedScanA<nmax.value, true>), hopsByStreams, dim3(256), ldsA, st, d, sBase, hopBase); });
		return true;
	case FEED_ONE_PASS:
		withFeedBins<16, 24>(d.M, [&](auto nmax) { hipLaunchKernelGGL((kFeedScanA<nmax.value, false, true>), hopsByStreams, dim3(256), ldsA, st, d, sBase, hopBase); });
		countLaunch(LK_FEED_ONE_PASS);
		return true;
	case FEED_ENVELOPE_PASS_A:
	case FEED_SEPARATE:
		break;
	}
	withFeedBins<16, 24, 0>(d.M, [&](auto nmax) { hipLaunchKernelGGL(kFeedScanA<nmax.value>, hopsByStreams, dim3(256), ldsA, st, d, sBase, hopBase); });
	if (!anyFormants) return false;
	hipLaunchKernelGGL(kFeedFreq, dim3(divUp(nStreams, 64)), dim3(64), 0, st, d, sBase, nStreams, hopBase);
	withFeedBins<16, 24, 0>(d.M, [&](auto nmax) {
		if (form == FEED_ENVELOPE_PASS_A) hipLaunchKernelGGL((kFeedScanC<nmax.value, true>), hopsByStreams, dim3(256), ldsC, st, d, sBase, hopBase);
		else hipLaunchKernelGGL(kFeedScanC<nmax.value>, hopsByStreams, dim3(256), ldsC, st, d, sBase, hopBase);
	});
	return form == FEED_ENVELOPE_PASS_A;
}

} // namespace smst
