// True peak of whole clips at the batch API's boundary (include/smst.h, "True peak", has the definition): Batch::exact measures the planar fp32
// output image in front of the levelled kClipOut, which takes a flagged stream's true-peak word in the place of its clip peak.
// Included by smst_state.hip only, behind smst_loudness.h.  Everything up to the final comparison is float64.
//
// One kernel, one pass.  A workgroup takes a tile of kTruePeakTile frames of one channel of one clip, in CLIP ORDER (position n of a clip lies
// at seg0.src + n of its row for n < seg0.count, at seg1.src + n - seg0.count behind that), and stages it into LDS with the 5 frames in front
// of it and the 6 behind it that the 12 taps of its first and last frame reach -- across the join of the two segments and across the tile's
// edges; positions outside [0, N) are written as 0.0.  The staging is loudStageWord's: the aligned 16-byte words that cover a run, one that
// lies inside the segment read whole (a neighbour's floats: read, never used beyond the halo), one at a segment's end element by element; a
// tile that the join cuts has two runs.  Nothing outside a stream's segments is read.
//
// Per-lane work.  A lane takes kTruePeakRun consecutive frames: it converts their kTruePeakRun + 11 floats to float64 once and forms the
// three phases of each frame from that register window.  Lane l's window begins at float l*kTruePeakRun of the LDS image, so for a run of 4
// the reads are aligned 16-byte ones of consecutive lanes; a run of 1 is the plain form -- consecutive lanes on consecutive frames, 12
// stride-1 reads per frame.  (EXPERIMENTS.md, "True peak", has what either form measured.)
// Every product of two float32 values is exact in float64, so y is the same whether or not a*b + y is contracted into an FMA.
// The maximum is one of bit patterns: lane -> wavefront -> workgroup -> one atomicMax where the tile holds anything above 0, as kClipPeak ends.
#pragma once
#include "smst_loudness.h"
#include <cmath>

namespace smst {

#ifndef SMST_TRUE_PEAK_RUN
#define SMST_TRUE_PEAK_RUN 4
#endif
constexpr int kTruePeakRun = SMST_TRUE_PEAK_RUN;                 // consecutive frames of one lane
constexpr int kTruePeakHalo = kTruePeakLead + kTruePeakTrail;    // 11 floats beside a tile
constexpr int kTruePeakLds = kTruePeakTile + kTruePeakHalo + 1;  // floats of the LDS image: position t0 - 5 + i at [i]; a multiple of 4
static_assert(kTruePeakTile%(256*kTruePeakRun) == 0 && kTruePeakLds%4 == 0, "a tile is whole passes of the workgroup's lanes; the image is whole words");
static_assert(kTruePeakLead + kTruePeakTrail + 1 == kTruePeakTaps, "the taps of a frame reach 5 frames back and 6 ahead");
inline size_t truePeakLdsBytes() { return size_t(kTruePeakLds)*sizeof(float) + 4*sizeof(int); }

// Per frame, the largest bit pattern of the sample and its three phases: m[i] of the F frames whose window begins at `at` -- frame i is
// at[i + 5], its taps reach at[i ... i + 11].  (The per-frame form: the limiter's detector, smst_limiter.h, keeps every frame's word.)
template <int F> __device__ inline void truePeakFrameBits(const float *at, const TruePeakTable &taps, unsigned (&m)[F]) {
	double w[F + kTruePeakHalo];
#pragma unroll
	for (int i = 0; i < F + kTruePeakHalo; ++i) w[i] = double(at[i]);
#pragma unroll
	for (int i = 0; i < F; ++i) { // (unrolled: w[] stays in registers)
		unsigned most = pcmPeakBits(at[i + kTruePeakLead]);
#pragma unroll
		for (int p = 0; p < 3; ++p) {
			double y = 0.0;
#pragma unroll
			for (int j = 0; j < kTruePeakTaps; ++j) y += double(taps.c[p][j])*w[i + j];
			most = max(most, pcmPeakBits(float(y)));
		}
		m[i] = most;
	}
}
// The largest of them among the first `valid` frames (a frame behind the clip's end is formed from the image's zeros and dropped)
template <int F> __device__ inline unsigned truePeakFrames(const float *at, int valid, const TruePeakTable &taps) {
	unsigned m[F], most = 0u;
	truePeakFrameBits<F>(at, taps, m);
#pragma unroll
	for (int i = 0; i < F; ++i) if (i < valid) most = max(most, m[i]);
	return most;
}

// The LDS image of the tile that begins at position t0 of a clip of N = n0 + n1 frames, of the channel whose row of the image is `row`:
// position t0 - 5 + i at lds[i], i < kTruePeakLds, 0.0 outside [0, N).  Every lane of the workgroup calls it; the caller synchronises.
__device__ inline void truePeakStage(const float *__restrict__ row, const ClipSeg &g0, const ClipSeg &g1, int t0, float *lds) {
	const int tid = threadIdx.x;
	const int n0 = max(g0.count, 0), n1 = max(g1.count, 0), N = n0 + n1;
	// [a, b): the clip's positions that the image holds, [i0, i1) their places in it; the rest of it is 0.0
	const int a = max(t0 - kTruePeakLead, 0), b = N - t0 > kTruePeakTile + kTruePeakTrail ? t0 + kTruePeakTile + kTruePeakTrail : N;
	const int i0 = a - t0 + kTruePeakLead, i1 = b - t0 + kTruePeakLead;
	for (int i = tid; i < kTruePeakLds; i += 256) if (i < i0 || i >= i1) lds[i] = 0.0f;
	// the two runs: [a, endA) of segment 0, [startB, b) of segment 1
	const int endA = min(b, n0), nA = max(endA - a, 0), startB = max(a, n0), nB = max(b - startB, 0), q = startB - n0;
	const float *runA = row + (size_t)g0.src + a, *runB = row + (size_t)g1.src + q;
	const int wordsA = loudWordsOf(runA, nA), wordsB = loudWordsOf(runB, nB);
	for (int word = tid; word < wordsA + wordsB; word += 256) {
		if (word < wordsA) loudStageWord(runA, nA, word, -a, n0 - a, lds + i0);
		else loudStageWord(runB, nB, word - wordsA, -q, n1 - q, lds + (startB - t0 + kTruePeakLead));
	}
}

// grid (tiles of kTruePeakTile frames in clip order, C, S), 256 threads.  The flag of level[s] off, a run of zeros, nothing to measure: returns at once
__global__ __launch_bounds__(256) void kClipTruePeak(const float *__restrict__ image, long long imageStreamStride, long long imageChannelStride, const ClipSeg *__restrict__ segs,
		const PcmLevel *__restrict__ level, TruePeakTable taps, int *__restrict__ truePeak) {
	extern __shared__ __attribute__((aligned(16))) unsigned char smemRaw[];
	float *lds = reinterpret_cast<float *>(smemRaw);       // [kTruePeakLds]
	int *waveMost = reinterpret_cast<int *>(lds + kTruePeakLds); // [4]
	const int s = blockIdx.z, c = blockIdx.y, tid = threadIdx.x;
	if (!(level[s].flags & kPcmFlagTruePeak)) return;
	const ClipSeg g0 = segs[2*s], g1 = segs[2*s + 1];
	if (g0.zeros || g1.zeros) return;
	const int N = max(g0.count, 0) + max(g1.count, 0);
	if ((long long)blockIdx.x*kTruePeakTile >= N) return;
	const int t0 = int(blockIdx.x)*kTruePeakTile;
	truePeakStage(image + (size_t)s*imageStreamStride + (size_t)c*imageChannelStride, g0, g1, t0, lds);
	__syncthreads();
	const int frames = min(N - t0, kTruePeakTile);
	unsigned most = 0u;
	for (int f = tid*kTruePeakRun; f < frames; f += 256*kTruePeakRun) most = max(most, truePeakFrames<kTruePeakRun>(lds + f, frames - f, taps));
	int m = int(most);
	for (int k = 32; k; k >>= 1) m = max(m, __shfl(m, (tid & 63) ^ k));
	if ((tid & 63) == 0) waveMost[tid >> 6] = m;
	__syncthreads();
	if (tid == 0) {
		m = max(max(waveMost[0], waveMost[1]), max(waveMost[2], waveMost[3]));
		if (m > 0) atomicMax(truePeak + s, m);
	}
}

// c[p - 1][j] = float32(h/sum_j h), h = sinc(t)*hann(t), t = j - 5 - p/4: in double, each phase normalised to unit DC gain, one rounding
const TruePeakTable &truePeakTable() {
	static const TruePeakTable table = [] {
		TruePeakTable t;
		const double pi = 3.14159265358979323846;
		for (int p = 1; p <= 3; ++p) {
			double h[kTruePeakTaps], sum = 0.0;
			for (int j = 0; j < kTruePeakTaps; ++j) {
				const double x = (j - kTruePeakLead) - p/4.0;
				h[j] = std::sin(pi*x)/(pi*x)*0.5*(1.0 + std::cos(pi*x/6.0));
				sum += h[j];
			}
			for (int j = 0; j < kTruePeakTaps; ++j) t.c[p - 1][j] = float(h[j]/sum);
		}
		return t;
	}();
	return table;
}

void launchClipTruePeak(const float *image, long long imageSS, long long imageCS, const ClipSeg *segs, int S, int C, int maxFrames, const PcmLevel *level, int *truePeak, hipStream_t st) {
	if (maxFrames < 1) return;
	hipLaunchKernelGGL(kClipTruePeak, dim3(divUp(maxFrames, kTruePeakTile), C, S), dim3(256), truePeakLdsBytes(), st, image, imageSS, imageCS, segs, level, truePeakTable(), truePeak);
	countLaunch(LK_CLIP_TRUE_PEAK);
}

} // namespace smst
