// The limiter's streaming form at the batch API's boundary (include/smst.h, "Stream limiter", has the definition): smst_batch_process_pcm and
// smst_batch_flush_pcm run the two passes on the call's planar fp32 output image in front of the limited kPcmOut.  Included by smst_state.hip
// only, behind smst_limiter.h.  The clip limiter's curve is non-recursive -- r(n) is a function of need over the 4H + 1 frames around n --, so
// with the output 2H frames late and the last 4H need values carried per stream, a stream cut into calls in any way gets the bits of the
// clip [2H zeros, every frame emitted so far].
//
// A stream's two lines alternate: a call reads the set its level entry names (kPcmFlagStreamLimitSet) and writes the other one, so no kernel
// updates what another workgroup of the same launch reads; the host flips the bit of the streams that took part.  Everything is ordered by
// the batch's stream alone, so one pair of sets and one pair of rows serve calls in flight.  A stream without the setting, with no frame in
// the call or left out by a flush returns at once in every kernel and keeps its lines.
//
// kPcmLimitFeed.  A workgroup takes kLimitTile of the stream's c new frames: need of each -- the maximum of pcmPeakBits over the channels,
// then limitNeed(m, |g|, ceiling) -- into the work row behind the 4H carried values, which workgroup 0 copies in front.  The next line's need
// is the row's last 4H values and the next line's frames the last 2H of [line, image]: every workgroup writes the entries that its own frames
// give, workgroup 0 those that the old line gives (c < 4H, c < 2H).
//
// kPcmLimitGain.  limitGainTile (smst_limiter.h) on the row: the c frames written are the row's frames 2H ... 2H + c - 1, and need is read
// inside the row only -- 2H values on either side, the right-hand ones being need of the frames that stay in the line.
//
// kPcmOutLimited.  kPcmOut's levelled form whose loader takes frame i of a limited stream from the line (i < 2H) or from the image at
// i - 2H, and whose quantiser multiplies by r(i) as well (pcmTileOut<T, Dith, true, true, true>).  No delayed copy of the image exists.
#pragma once
#include "smst_limiter.h"
#include "smst_pcm.h"

namespace smst {

// grid (tiles of kLimitTile frames of the call, S), 256 threads
__global__ __launch_bounds__(256) void kPcmLimitFeed(const float *__restrict__ image, long long imageStreamStride, long long imageChannelStride, const int *__restrict__ counts, int C,
		const PcmLevel *__restrict__ table, PcmStreamLimit lim) {
	const int s = blockIdx.y, tid = threadIdx.x, H = lim.H;
	const PcmLevel l = table[s];
	if (!(l.flags & kPcmFlagStreamLimiter)) return;
	const int c = counts[s];
	if ((long long)blockIdx.x*kLimitTile >= c) return;
	const int t0 = int(blockIdx.x)*kLimitTile, frames = min(c - t0, kLimitTile), set = (l.flags & kPcmFlagStreamLimitSet) ? 1 : 0;
	const float *lineNeed = lim.need[set] + (size_t)s*4*H, *lineFrames = lim.frames[set] + (size_t)s*C*2*H;
	float *nextNeed = lim.need[set ^ 1] + (size_t)s*4*H, *nextFrames = lim.frames[set ^ 1] + (size_t)s*C*2*H;
	float *row = lim.needRow + (size_t)s*lim.needPitch; // need(p - 4H + j) at row[j], p the frames emitted before this call
	if (blockIdx.x == 0) {
		for (int j = tid; j < 4*H; j += 256) {
			const float v = lineNeed[j];
			row[j] = v;
			if (j >= c) nextNeed[j - c] = v;
		}
		for (int ch = 0; ch < C; ++ch)
			for (int j = c + tid; j < 2*H; j += 256) nextFrames[(size_t)ch*2*H + (j - c)] = lineFrames[(size_t)ch*2*H + j];
	}
	const float g = fabsf(l.gain);
	const float *src = image + (size_t)s*imageStreamStride + t0;
	for (int i = tid; i < frames; i += 256) {
		const long long f = (long long)t0 + i, toFrames = f + 2*H - c, toNeed = f + 4*H - c; // (both below the lines' lengths: f < c)
		unsigned m = 0u;
		for (int ch = 0; ch < C; ++ch) {
			const float v = src[(size_t)ch*imageChannelStride + i];
			m = max(m, pcmPeakBits(v));
			if (toFrames >= 0) nextFrames[(size_t)ch*2*H + toFrames] = v;
		}
		const float need = limitNeed(m, g, l.ceiling);
		row[4*H + f] = need;
		if (toNeed >= 0) nextNeed[toNeed] = need;
	}
}

// grid (tiles of kLimitTile frames of the call, S), 256 threads, limitGainLdsBytes(H) of LDS
__global__ __launch_bounds__(256) void kPcmLimitGain(const int *__restrict__ counts, const PcmLevel *__restrict__ table, int S, PcmStreamLimit lim) {
	extern __shared__ __attribute__((aligned(16))) unsigned char smemRaw[];
	const int s = blockIdx.y, H = lim.H;
	if (!(table[s].flags & kPcmFlagStreamLimiter)) return;
	const int c = counts[s];
	if ((long long)blockIdx.x*kLimitTile >= c) return;
	const int t0 = int(blockIdx.x)*kLimitTile, frames = min(c - t0, kLimitTile);
	// frame i of the call is frame 2H + i of the row: need is read from 2H in front of the call's first frame to 2H behind its last one
	limitGainTile(smemRaw, lim.needRow + (size_t)s*lim.needPitch + 2*H, -2LL*H, (long long)c + 2*H, t0, frames, lim.rRow + (size_t)s*lim.rPitch + t0, lim.window, H, lim.meters, s, S);
}

// kPcmOut's levelled form of a call with a limited stream: grid (tiles, S), 256 threads
template <typename T, bool Dith> __global__ __launch_bounds__(256) void kPcmOutLimited(const float *__restrict__ in, long long inStreamStride, long long inChannelStride,
		T *__restrict__ out, long long outStreamStride, long long outFrameStride, const int *__restrict__ counts, int C, unsigned *__restrict__ overs, const PcmDither *__restrict__ dither,
		PcmLevelIo level, PcmStreamLimit lim) {
	extern __shared__ __attribute__((aligned(16))) unsigned char smemRaw[];
	const int s = blockIdx.y;
	PcmDither dp{0u, 0u, 0u, 0u};
	if constexpr (Dith) dp = dither[s];
	const PcmLevel l = level.table[s];
	const bool on = (l.flags & kPcmFlagStreamLimiter) != 0;
	const float *line = on ? lim.frames[(l.flags & kPcmFlagStreamLimitSet) ? 1 : 0] + (size_t)s*C*2*lim.H : nullptr;
	const float *r = on ? lim.rRow + (size_t)s*lim.rPitch : nullptr;
	unsigned over, peak;
	if (!pcmTileOut<T, Dith, true, true, true>(in + (size_t)s*inStreamStride, inChannelStride, out + (size_t)s*outStreamStride, outFrameStride, counts[s], blockIdx.x, C,
	                                           reinterpret_cast<float *>(smemRaw), over, dp, l.gain, &peak, r, line, 2*lim.H)) return;
	if (blockIdx.x == 0 && threadIdx.x == 0) level.applied[s] = l.gain;
	pcmMaxPeak(level.peaks, s, peak);
	pcmAddOvers(overs, s, over);
}

// grid (S), 256 threads: both sets of a stream's lines as a batch begins with them
__global__ __launch_bounds__(256) void kPcmLimitClear(PcmStreamLimit lim, int C, int stream) {
	const int s = stream < 0 ? int(blockIdx.x) : stream, H = lim.H;
	for (int set = 0; set < 2; ++set) {
		for (int j = threadIdx.x; j < 4*H; j += 256) lim.need[set][(size_t)s*4*H + j] = 1.0f;
		for (int j = threadIdx.x; j < C*2*H; j += 256) lim.frames[set][(size_t)s*C*2*H + j] = 0.0f;
	}
}

void launchPcmLimitClear(const PcmStreamLimit &lim, int S, int C, int stream, hipStream_t st) {
	hipLaunchKernelGGL(kPcmLimitClear, dim3(stream < 0 ? S : 1), dim3(256), 0, st, lim, C, stream);
}

void launchPcmOutLimited(int format, const float *in, long long inStreamStride, long long inChannelStride, void *out, long long outStreamStride, long long outFrameStride,
                         const int *counts, int S, int C, int maxFrames, int maxLimited, unsigned *overs, hipStream_t st, const PcmDither *dither, const PcmLevelIo &level,
                         const PcmStreamLimit &lim) {
	if (maxLimited < 1 || maxFrames < maxLimited) throw std::invalid_argument("the limited output conversion needs a limited stream with frames");
	const dim3 tiles(divUp(maxLimited, kLimitTile), S);
	hipLaunchKernelGGL(kPcmLimitFeed, tiles, dim3(256), 0, st, in, inStreamStride, inChannelStride, counts, C, level.table, lim);
	countLaunch(LK_PCM_LIMIT_FEED);
	hipLaunchKernelGGL(kPcmLimitGain, tiles, dim3(256), limitGainLdsBytes(lim.H), st, counts, level.table, S, lim);
	countLaunch(LK_PCM_LIMIT_GAIN);
	const dim3 grid(divUp(maxFrames, kPcmTileFrames), S);
	pcmDispatch(format, dither != nullptr, [&](auto tag, auto dithered) {
		typedef typename decltype(tag)::type T;
		constexpr bool Dith = decltype(dithered)::value;
		const size_t lds = Dith ? pcmDitherLdsBytes(C) : pcmLdsBytes(C);
		hipLaunchKernelGGL((kPcmOutLimited<T, Dith>), grid, dim3(256), lds, st, in, inStreamStride, inChannelStride, static_cast<T *>(out), outStreamStride, outFrameStride, counts, C, overs, dither, level, lim);
	});
	countLaunch(LK_PCM_OUT_LIMITED);
}

} // namespace smst
