// Loudness range (EBU Tech 3342) and the maximum momentary and short-term loudness (EBU Tech 3341) of whole clips (include/smst.h, "Loudness
// range", has the definition): Batch::exact runs kLoudRange behind kLoudGate, on the sub-block sums and the block powers that the four passes of
// smst_loudness.h left in their scratch, and in front of everything that reads a stream's gain gL -- which the stage lowers in place where a
// cap on one of the two maxima asks for it.  Included by smst_state.hip only, behind smst_loudness.h.  Everything is float64 and integers.
//
// One workgroup per stream, four stages:
//   short-term powers   st_i from 30 sub-block sums per channel.  The sums of a tile of kLoudRangeThreads powers -- that many plus 29 -- go
//                       through LDS, a channel at a time: every sum is read from memory once, not 30 times            -> st[stream][i]
//   maxima              of the block powers and of st.  A power that counts is above 0, and positive doubles order as their 64-bit patterns:
//                       the maximum is one of integers, so its order does not matter                                   -> M, ST
//   gates               the absolute gate's mean with its sum in block order by lane 0, kLoudGate's way; the count past both gates is a sum
//                       of integers                                                                                   -> rel, n
//   selection           v[kLo] and v[kHi] of the n gated values by a radix select over their bit patterns: kLoudRangePasses passes from the
//                       top digit down, each a histogram of the digit over the values that share the digits chosen so far, both ranks in
//                       the same passes.  The values stay where they are, in st[]: any n the call accepts is served, at n reads per pass
// Nothing here depends on the scheduling: the histograms and the counts are integer atomics in LDS, and there is no floating-point atomic.
//
// The top digits of n powers of similar size are the same for nearly all of them, so a lane does not add 1 per value: it counts the run of
// equal digits it meets and adds the run -- in those passes one atomic per lane, not n on one LDS word.
#pragma once
#include "smst_loudness.h"

namespace smst {

constexpr int kLoudRangeThreads = 256;                       // lanes of a stream's workgroup = the short-term powers of one tile of every stage
constexpr int kLoudRangeWindow = 30;                         // 100-ms sub-blocks of a short-term power
constexpr int kLoudRangeDigitBits = 8, kLoudRangeBins = 1 << kLoudRangeDigitBits, kLoudRangePasses = 64/kLoudRangeDigitBits;
constexpr int kLoudRangeTileDoubles = 2*kLoudRangeThreads;   // LDS: a tile of sums (threads + 29), or the two maxima's words (2*threads)
static_assert(kLoudRangeThreads + kLoudRangeWindow - 1 <= kLoudRangeTileDoubles && kLoudRangeBins <= kLoudRangeThreads, "the LDS tile holds a stage-1 tile; a lane clears a bin");
inline size_t loudRangeLdsBytes() { return kLoudRangeTileDoubles*sizeof(double) + 2*kLoudRangeBins*sizeof(int) + 2*sizeof(unsigned long long) + 4*sizeof(int); }

__device__ inline unsigned long long loudRangeBits(double v) { return __builtin_bit_cast(unsigned long long, v); }
__device__ inline unsigned long long loudRangeMax(unsigned long long a, unsigned long long b) { return a > b ? a : b; }
// the cap gain of a maximum `top` under the cap power `cap`: float32(sqrt(cap/top)), +inf where there is no cap or nothing to cap
__device__ inline float loudRangeCapGain(double cap, double top) {
	const double inf = __builtin_inf();
	return (cap < inf && top > 0.0 && top < inf) ? float(sqrt(cap/top)) : float(inf);
}

// grid (S), kLoudRangeThreads threads; LDS: loudRangeLdsBytes().  Writes every stream's meters: one that is not metered has none
__global__ __launch_bounds__(kLoudRangeThreads) void kLoudRange(const ClipSeg *__restrict__ segs, const LoudEntry *__restrict__ loud, const float *__restrict__ weights, int C, LoudScratch w, LoudRangeScratch r) {
	extern __shared__ __attribute__((aligned(16))) unsigned char smemRaw[];
	double *tile = reinterpret_cast<double *>(smemRaw);                                       // [kLoudRangeTileDoubles]
	unsigned long long *best = reinterpret_cast<unsigned long long *>(smemRaw);               // (the same words)
	int *hist = reinterpret_cast<int *>(tile + kLoudRangeTileDoubles);                        // [2][kLoudRangeBins]: the low rank's, the high rank's
	unsigned long long *pick = reinterpret_cast<unsigned long long *>(hist + 2*kLoudRangeBins); // [2]: the digits chosen so far
	int *rank = reinterpret_cast<int *>(pick + 2);                                            // [2]: the ranks among the values that share them; [2]: n
	constexpr int T = kLoudRangeThreads, W = kLoudRangeWindow;
	const int s = blockIdx.x, tid = threadIdx.x;
	const int h = loud[s].h;
	const ClipSeg g0 = segs[2*s], g1 = segs[2*s + 1];
	double *meters = r.meters + (size_t)4*s;
	if (h == 0 || !loud[s].meter || g0.zeros || g1.zeros) {
		if (tid == 0) { meters[0] = meters[1] = meters[2] = meters[3] = 0.0; r.counts[2*s] = r.counts[2*s + 1] = 0; }
		return;
	}
	const int N = max(g0.count, 0) + max(g1.count, 0);
	const int nSub = N/4 >= h ? N/h : 0, nb = nSub ? nSub - 3 : 0, ns = nSub >= W ? nSub - (W - 1) : 0;
	const double *sub = w.sub + (size_t)s*C*w.maxSub, *z = w.z + (size_t)s*w.maxSub;
	double *st = r.st + (size_t)s*r.maxSt;
	// 1. the short-term powers
	for (int base = 0; base < ns; base += T) {
		const int cnt = min(T + W - 1, nSub - base);
		double acc = 0.0;
		for (int c = 0; c < C; ++c) {
			const double *q = sub + (size_t)c*w.maxSub + base;
			for (int j = tid; j < cnt; j += T) tile[j] = q[j];
			__syncthreads();
			if (base + tid < ns) {
				double sum = 0.0;
				for (int j = 0; j < W; ++j) sum += tile[tid + j];
				acc += double(weights[c])*sum;
			}
			__syncthreads(); // (the next channel goes into the same tile)
		}
		if (base + tid < ns) st[base + tid] = acc/(double(W)*h);
	}
	__syncthreads();
	// 2. the maxima: a power that is NaN or 0 leaves the word as it is
	{
		unsigned long long m = 0, t = 0;
		for (int i = tid; i < nb; i += T) { const double v = z[i]; if (v > 0.0) m = loudRangeMax(m, loudRangeBits(v)); }
		for (int i = tid; i < ns; i += T) { const double v = st[i]; if (v > 0.0) t = loudRangeMax(t, loudRangeBits(v)); }
		best[tid] = m; best[T + tid] = t;
		__syncthreads();
		for (int off = T/2; off > 0; off >>= 1) {
			if (tid < off) { best[tid] = loudRangeMax(best[tid], best[tid + off]); best[T + tid] = loudRangeMax(best[T + tid], best[T + tid + off]); }
			__syncthreads();
		}
	}
	const double M = __builtin_bit_cast(double, best[0]), ST = __builtin_bit_cast(double, best[T]);
	__syncthreads(); // (the tile is written again)
	// 3. the gates, power domain.  The powers go through LDS a tile at a time; lane 0 sums them in block order
	const double gate = loud[s].gate;
	double sum = 0.0;
	int passed = 0;
	for (int base = 0; base < ns; base += T) {
		if (base + tid < ns) tile[tid] = st[base + tid];
		__syncthreads();
		if (tid == 0) for (int i = 0; i < min(T, ns - base); ++i) if (tile[i] > gate) { sum += tile[i]; ++passed; }
		__syncthreads();
	}
	if (tid == 0) { tile[0] = passed ? 0.01*(sum/passed) : 0.0; rank[2] = 0; }
	__syncthreads();
	const double rel = tile[0];
	{
		int mine = 0;
		for (int i = tid; i < ns; i += T) { const double v = st[i]; if (v > gate && v > rel) ++mine; }
		if (mine) atomicAdd(&rank[2], mine);
	}
	__syncthreads();
	const int n = rank[2];
	// 4. the two order statistics of the n gated values
	unsigned long long chosen[2] = {0, 0};
	if (n > 0) { // (uniform: every lane has the same n)
		if (tid == 0) { rank[0] = ((n - 1)*10 + 50)/100; rank[1] = ((n - 1)*95 + 50)/100; }
		for (int pass = 0; pass < kLoudRangePasses; ++pass) {
			const int shift = 64 - kLoudRangeDigitBits*(pass + 1);
			const unsigned long long above = pass ? ~0ull << (shift + kLoudRangeDigitBits) : 0ull; // the digits chosen so far
			if (tid < kLoudRangeBins) hist[tid] = hist[kLoudRangeBins + tid] = 0;
			__syncthreads();
			int bin[2] = {0, 0}, run[2] = {0, 0};
			for (int i = tid; i < ns; i += T) {
				const double v = st[i];
				if (!(v > gate && v > rel)) continue;
				const unsigned long long b = loudRangeBits(v);
				const int d = int((b >> shift) & (kLoudRangeBins - 1));
				for (int k = 0; k < 2; ++k) {
					if ((b & above) != chosen[k]) continue;
					if (d != bin[k]) {
						if (run[k]) atomicAdd(&hist[k*kLoudRangeBins + bin[k]], run[k]);
						bin[k] = d; run[k] = 0;
					}
					++run[k];
				}
			}
			for (int k = 0; k < 2; ++k) if (run[k]) atomicAdd(&hist[k*kLoudRangeBins + bin[k]], run[k]);
			__syncthreads();
			if (tid == 0 || tid == 64) { // (two wavefronts: one walks the low rank's bins, one the high rank's)
				const int k = tid ? 1 : 0;
				int left = rank[k], d = 0;
				for (; d < kLoudRangeBins - 1 && left >= hist[k*kLoudRangeBins + d]; ++d) left -= hist[k*kLoudRangeBins + d];
				rank[k] = left;
				pick[k] = chosen[k] | (unsigned long long)d << shift;
			}
			__syncthreads();
			chosen[0] = pick[0]; chosen[1] = pick[1];
		}
	}
	if (tid) return;
	meters[0] = M; meters[1] = ST;
	meters[2] = __builtin_bit_cast(double, chosen[0]); meters[3] = __builtin_bit_cast(double, chosen[1]);
	r.counts[2*s] = ns; r.counts[2*s + 1] = n;
	// the caps: gL' = min(gL, gm, gs), over gL where kLoudGate wrote it; a stream without a finite cap keeps the bits of gL
	const float gm = loudRangeCapGain(loud[s].Pm, M), gs = loudRangeCapGain(loud[s].Ps, ST), gL = w.gain[s];
	const float capped = min(gL, min(gm, gs));
	if (capped < gL) w.gain[s] = capped;
}

void launchClipLoudnessRange(const ClipSeg *segs, int S, int C, const LoudEntry *loud, const float *weights, const LoudScratch &w, const LoudRangeScratch &r, hipStream_t st) {
	hipLaunchKernelGGL(kLoudRange, dim3(S), dim3(kLoudRangeThreads), loudRangeLdsBytes(), st, segs, loud, weights, C, w, r);
	countLaunch(LK_CLIP_LOUDNESS_RANGE);
}

} // namespace smst
