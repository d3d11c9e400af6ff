// Lookahead limiter of whole clips at the batch API's boundary (include/smst.h, "Limiter", has the definition): Batch::exact runs the two passes
// on the planar fp32 output image behind the peak, loudness and true-peak passes and in front of the limited kClipOut, which multiplies every
// frame of a limited stream by its r.  Included by smst_state.hip only, behind smst_true_peak.h.  The gain curve is non-recursive: every
// frame's r is a function of need over 4H + 1 frames around it, so the tiles are independent and a run is bit-reproducible.
//
// kClipLimitNeed.  A workgroup takes a tile of kLimitTile frames of one clip, in CLIP ORDER, and every channel of it in turn: the channel's
// tile goes into LDS through truePeakStage -- the true-peak kernel's image, halo of 5 and 6 included --, a lane keeps the running maximum of
// its kLimitRun consecutive frames' words (the bits of |x|; with the stream's true-peak flag the three phases of the frame as well:
// truePeakFrameBits, the true-peak kernel's own sums), and behind the last channel forms need from the maximum, the stream's gain in its
// limited form (clipGain) and the ceiling: one fp32 multiply, one comparison, one correctly rounded division.
//
// kClipLimitGain (its body is limitGainTile, which the streaming form shares).  A workgroup stages its tile's need with 2H frames on either side (1.0 outside the clip) into LDS; a tile in which all of
// that is 1.0 writes r = 1.0f and ends -- the definition's idle rule makes this exact.  Else the windowed minimum by doubling: M_1 = need,
// M_2k[i] = min(M_k[i], M_k[i + k]) between two LDS arrays while 2k <= 2H + 1, then hold[i] = min(M_k[i], M_k[i + 2H + 1 - k]) -- two
// overlapping spans of k frames that cover the 2H + 1; the minimum is exact and associative, so the scheme does not show in the result.
// Then, per frame, the float64 sum over the window in the order k = -H ... H from 0.0 (exact products: contraction changes nothing), the
// minimum of hold over the same frames for the idle rule, and r = min(float32(y), need(n)).  Consecutive lanes take consecutive frames: the
// LDS reads of a tap are conflict-free, the window's float is the same for every lane.  The meters are integers: lane -> wavefront ->
// workgroup through LDS -> one atomicMax and one atomicAdd per workgroup that limited anything.
//
// LDS: two arrays of kLimitTile + 4H floats -- 10.3 KiB at the default H = 72, 40 KiB at H = 1024.
#pragma once
#include "smst_true_peak.h"
#include <vector>

namespace smst {

constexpr int kLimitRun = kLimitTile/256; // consecutive frames of one lane of the need pass
static_assert(kLimitTile == kTruePeakTile && kLimitRun*256 == kLimitTile, "the need pass stages the true-peak kernel's image: one pass of the workgroup's lanes per channel");
inline size_t limitNeedLdsBytes() { return size_t(kTruePeakLds)*sizeof(float); }
inline int limitSpan(int H) { return kLimitTile + 4*H; }
inline size_t limitGainLdsBytes(int H) { return size_t(2*limitSpan(H))*sizeof(float) + 12*sizeof(int); }

// need of a frame whose loudest word is mBits, at the whole-clip gain g: ceiling/w where w = m*g is finite and above the ceiling, else 1
__device__ inline float limitNeed(unsigned mBits, float g, float ceiling) {
	const float w = __fmul_rn(__int_as_float(int(mBits)), g);
	return (w > ceiling && w <= 3.402823466e38f) ? ceiling/w : 1.0f;
}

// grid (tiles of kLimitTile frames in clip order, S), 256 threads.  A stream that is not limited, a run of zeros, nothing to do: returns at once
__global__ __launch_bounds__(256) void kClipLimitNeed(const float *__restrict__ image, long long imageStreamStride, long long imageChannelStride, const ClipSeg *__restrict__ segs, int C,
		PcmLevelIo level, TruePeakTable taps, float *__restrict__ need, long long pitch) {
	extern __shared__ __attribute__((aligned(16))) unsigned char smemRaw[];
	float *lds = reinterpret_cast<float *>(smemRaw); // [kTruePeakLds]
	const int s = blockIdx.y, tid = threadIdx.x;
	const PcmLevel l = level.table[s];
	if (!pcmLimited(l)) return;
	const ClipSeg g0 = segs[2*s], g1 = segs[2*s + 1];
	if (g0.zeros || g1.zeros) return;
	const int N = max(g0.count, 0) + max(g1.count, 0);
	if ((long long)blockIdx.x*kLimitTile >= N) return;
	const int t0 = int(blockIdx.x)*kLimitTile, frames = min(N - t0, kLimitTile), f = tid*kLimitRun;
	unsigned m[kLimitRun];
#pragma unroll
	for (int i = 0; i < kLimitRun; ++i) m[i] = 0u;
	for (int c = 0; c < C; ++c) {
		if (c) __syncthreads(); // (the image of the channel before has been read)
		truePeakStage(image + (size_t)s*imageStreamStride + (size_t)c*imageChannelStride, g0, g1, t0, lds);
		__syncthreads();
		if (f >= frames) continue;
		if (l.flags & kPcmFlagTruePeak) {
			unsigned mc[kLimitRun];
			truePeakFrameBits<kLimitRun>(lds + f, taps, mc);
#pragma unroll
			for (int i = 0; i < kLimitRun; ++i) m[i] = max(m[i], mc[i]);
		} else {
#pragma unroll
			for (int i = 0; i < kLimitRun; ++i) m[i] = max(m[i], pcmPeakBits(lds[f + i + kTruePeakLead]));
		}
	}
	const float g = clipGain(l, 0, l.mode == kPcmLevelLoudness && level.loudGain ? level.loudGain[s] : 1.0f, true);
	float *row = need + (size_t)s*pitch + t0;
#pragma unroll
	for (int i = 0; i < kLimitRun; ++i) if (f + i < frames) row[f + i] = limitNeed(m[i], g, l.ceiling);
}

// Steps 4 to 6 of the definition for one tile, the one definition of kClipLimitGain and of the streaming form (kPcmLimitGain,
// smst_stream_limiter.h): r of the `frames` frames from t0 on -> out[0 ... frames), and the stream's two meter words.  need(j) = row[j] for
// lo <= j < hi and 1 outside; the tile's own frames lie inside.  Every lane of the workgroup calls it, with limitGainLdsBytes(H) of LDS at
// smemRaw.  Staging, the idle rule, the doubling minimum, the float64 sum in order, min(float(y), need) and the meter reduction; the loops run
// over the frames the tile has plus 4H.  win: [2H + 1]; meters: [2][S]
__device__ inline void limitGainTile(unsigned char *smemRaw, const float *__restrict__ row, long long lo, long long hi, int t0, int frames, float *__restrict__ out,
		const float *__restrict__ win, int H, int *__restrict__ meters, int s, int S) {
	const int tid = threadIdx.x, span = frames + 4*H, W = 2*H + 1;
	float *cur = reinterpret_cast<float *>(smemRaw), *nxt = cur + (kLimitTile + 4*H); // [limitSpan(H)] each
	int *words = reinterpret_cast<int *>(nxt + (kLimitTile + 4*H));                   // [0]: the tile is active; [1 ... 4], [5 ... 8]: the wavefronts' meters
	if (tid == 0) words[0] = 0;
	__syncthreads();
	// need(t0 - 2H + i) at cur[i]; outside [lo, hi) it is 1
	bool active = false;
	for (int i = tid; i < span; i += 256) {
		const long long j = (long long)t0 - 2*H + i;
		const float v = (j >= lo && j < hi) ? row[j] : 1.0f;
		cur[i] = v;
		active = active || v != 1.0f;
	}
	if (active) words[0] = 1; // (every lane that writes writes the same)
	__syncthreads();
	if (!words[0]) { // idle: no need below 1 within 2H frames of any frame of the tile
		for (int f = tid; f < frames; f += 256) out[f] = 1.0f;
		return;
	}
	// cur[i] = the minimum of need over len frames from t0 - 2H + i on, for i + len <= span
	int len = 1;
	for (; 2*len <= W; len *= 2) {
		for (int i = tid; i + 2*len <= span; i += 256) nxt[i] = fminf(cur[i], cur[i + len]);
		__syncthreads();
		float *t = cur; cur = nxt; nxt = t;
	}
	// hold(t0 - H + i) at nxt[i], i < frames + 2H: the 2H + 1 frames from t0 - 2H + i on, as two spans of len
	for (int i = tid; i < frames + 2*H; i += 256) nxt[i] = fminf(cur[i], cur[i + W - len]);
	__syncthreads();
	const float *hold = nxt;
	unsigned deepest = 0u;
	int limited = 0;
	for (int f = tid; f < frames; f += 256) {
		const float *h = hold + f; // hold(n + k) at h[k + H]
		double y = 0.0;
		float lowest = 1.0f;
		for (int k = 0; k < W; ++k) {
			const float v = h[k];
			lowest = fminf(lowest, v);
			y += double(win[k])*double(v);
		}
		const float rr = lowest == 1.0f ? 1.0f : fminf(float(y), row[(long long)t0 + f]);
		out[f] = rr;
		deepest = max(deepest, 0x3f800000u - unsigned(__float_as_int(rr))); // (0 < r <= 1: need is, and r <= need)
		limited += rr < 1.0f ? 1 : 0;
	}
	int most = int(deepest), count = limited;
	for (int k = 32; k; k >>= 1) { most = max(most, __shfl(most, (tid & 63) ^ k)); count += __shfl(count, (tid & 63) ^ k); }
	if ((tid & 63) == 0) { words[1 + (tid >> 6)] = most; words[5 + (tid >> 6)] = count; }
	__syncthreads();
	if (tid == 0) {
		most = max(max(words[1], words[2]), max(words[3], words[4]));
		count = words[5] + words[6] + words[7] + words[8];
		if (most > 0) atomicMax(meters + s, most);
		if (count > 0) atomicAdd(meters + S + s, count);
	}
}

// grid (tiles of kLimitTile frames in clip order, S), 256 threads, limitGainLdsBytes(H) of LDS.  win: [2H + 1]; meters: [2][S]
__global__ __launch_bounds__(256) void kClipLimitGain(const ClipSeg *__restrict__ segs, const PcmLevel *__restrict__ table, int S, const float *__restrict__ need, float *__restrict__ r,
		long long pitch, const float *__restrict__ win, int H, int *__restrict__ meters) {
	extern __shared__ __attribute__((aligned(16))) unsigned char smemRaw[];
	const int s = blockIdx.y;
	if (!pcmLimited(table[s])) return;
	const ClipSeg g0 = segs[2*s], g1 = segs[2*s + 1];
	if (g0.zeros || g1.zeros) return;
	const int N = max(g0.count, 0) + max(g1.count, 0);
	if ((long long)blockIdx.x*kLimitTile >= N) return;
	const int t0 = int(blockIdx.x)*kLimitTile, frames = min(N - t0, kLimitTile);
	limitGainTile(smemRaw, need + (size_t)s*pitch, 0, N, t0, frames, r + (size_t)s*pitch + t0, win, H, meters, s, S);
}

void limitWindow(int H, float *win) {
	const double pi = 3.14159265358979323846;
	std::vector<double> h((size_t)2*H + 1);
	double sum = 0.0;
	for (int k = -H; k <= H; ++k) { h[size_t(k + H)] = 0.5*(1.0 + std::cos(pi*k/(H + 1))); sum += h[size_t(k + H)]; }
	for (int k = 0; k <= 2*H; ++k) win[k] = float(h[size_t(k)]/sum);
}

void launchClipLimit(const float *image, long long imageSS, long long imageCS, const ClipSeg *segs, int S, int C, int maxFrames, const PcmLevelIo &level, int H, const float *window,
                     float *need, float *r, long long pitch, int *meters, hipStream_t st) {
	if (maxFrames < 1) return;
	const dim3 grid(divUp(maxFrames, kLimitTile), S);
	hipLaunchKernelGGL(kClipLimitNeed, grid, dim3(256), limitNeedLdsBytes(), st, image, imageSS, imageCS, segs, C, level, truePeakTable(), need, pitch);
	countLaunch(LK_CLIP_LIMIT_NEED);
	hipLaunchKernelGGL(kClipLimitGain, grid, dim3(256), limitGainLdsBytes(H), st, segs, level.table, S, need, r, pitch, window, H, meters);
	countLaunch(LK_CLIP_LIMIT_GAIN);
}

} // namespace smst
