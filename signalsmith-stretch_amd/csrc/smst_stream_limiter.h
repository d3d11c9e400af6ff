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
// kPcmLimitFeedTruePeak.  The feed pass of the streams with kPcmFlagStreamLimitTruePeak, which kPcmLimitFeed leaves alone (and the other
// way round).  The taps of a frame reach 6 frames ahead, so the c values a call adds to the row are need of v(p - 6) ... v(p + c - 7), p the
// frames emitted before the call, and the taps of those reach v(p - 11) ... v(p + c - 1): the stream carries its last 2H + 11 frames per
// channel, of which the last 11 are that history and the last 2H + 6 what the output is late by (a uniform length: at H = 1 and 2 the 11
// are the longer part).  Per channel the workgroup stages the kLimitTile + 11 frames of [line, image] that its tile's taps reach into one
// LDS image -- the true-peak kernel's, 0.0 behind the call's last frame --, a lane folds truePeakFrameBits of its frames into its running
// maxima (the one definition of the phases, with kClipLimitNeed and kClipTruePeak), and behind the last channel limitNeed gives the row's
// values; the need line and the frames' line move on as in kPcmLimitFeed.  Long: a lane takes 4 consecutive frames from a register window
// of 15 floats (kClipLimitNeed's form); short calls -- the 128-frame real-time call has one tile per stream -- take the run of 1, lane l on
// frame l + 256k, so that a tile of up to 256 frames has every lane at work (EXPERIMENTS.md, "Stream limiter, true-peak detector").
//
// kPcmLimitGain.  limitGainTile (smst_limiter.h) on the row: the c frames written are the row's frames 2H ... 2H + c - 1, and need is read
// inside the row only -- 2H values on either side, the right-hand ones being need of the frames that stay in the line.
//
// kPcmOutLimited.  kPcmOut's levelled form whose loader takes frame i of a limited stream from the line (i < D) or from the image at
// i - D -- D = 2H and the frames' line, or 2H + 6 and the last 2H + 6 of the flag's line --, and whose quantiser multiplies by r(i) as well
// (pcmTileOut<T, Dith, true, true, true>).  No delayed copy of the image exists.
#pragma once
#include "smst_limiter.h"
#include "smst_pcm.h"

namespace smst {

// The longest call (its longest flagged count) whose true-peak feed pass takes the run of 1 (EXPERIMENTS.md, "Stream limiter, true-peak
// detector", has what either run measured per call size)
#ifndef SMST_STREAM_LIMIT_TRUE_PEAK_SHORT
#define SMST_STREAM_LIMIT_TRUE_PEAK_SHORT 256
#endif
constexpr int kStreamLimitTruePeakShort = SMST_STREAM_LIMIT_TRUE_PEAK_SHORT;

// grid (tiles of kLimitTile frames of the call, S), 256 threads
__global__ __launch_bounds__(256) void kPcmLimitFeed(const float *__restrict__ image, long long imageStreamStride, long long imageChannelStride, const int *__restrict__ counts, int C,
		const PcmLevel *__restrict__ table, PcmStreamLimit lim) {
	const int s = blockIdx.y, tid = threadIdx.x, H = lim.H;
	const PcmLevel l = table[s];
	if ((l.flags & (kPcmFlagStreamLimiter | kPcmFlagStreamLimitTruePeak)) != kPcmFlagStreamLimiter) return;
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

// grid (tiles of kLimitTile frames of the call, S), 256 threads, limitNeedLdsBytes() of LDS.  Strided: the run of 1 (lane l on frames
// l + 256k of the tile) in the place of 4 consecutive frames per lane
template <bool Strided> __global__ __launch_bounds__(256) void kPcmLimitFeedTruePeak(const float *__restrict__ image, long long imageStreamStride, long long imageChannelStride,
		const int *__restrict__ counts, int C, const PcmLevel *__restrict__ table, TruePeakTable taps, PcmStreamLimit lim) {
	extern __shared__ __attribute__((aligned(16))) unsigned char smemRaw[];
	float *lds = reinterpret_cast<float *>(smemRaw); // [kTruePeakLds]: frame p - 11 + t0 + i at [i], p the frames emitted before this call
	const int s = blockIdx.y, tid = threadIdx.x, H = lim.H, L = pcmStreamLimitTruePeakLine(H);
	const PcmLevel l = table[s];
	if ((l.flags & (kPcmFlagStreamLimiter | kPcmFlagStreamLimitTruePeak)) != (kPcmFlagStreamLimiter | kPcmFlagStreamLimitTruePeak)) return;
	const int c = counts[s];
	if ((long long)blockIdx.x*kLimitTile >= c) return;
	const int t0 = int(blockIdx.x)*kLimitTile, frames = min(c - t0, kLimitTile), set = (l.flags & kPcmFlagStreamLimitSet) ? 1 : 0;
	const float *lineNeed = lim.need[set] + (size_t)s*4*H, *lineFrames = lim.truePeakFrames[set] + (size_t)s*C*L;
	float *nextNeed = lim.need[set ^ 1] + (size_t)s*4*H, *nextFrames = lim.truePeakFrames[set ^ 1] + (size_t)s*C*L;
	float *row = lim.needRow + (size_t)s*lim.needPitch; // need(p - 6 - 4H + j) at row[j]
	if (blockIdx.x == 0) {
		for (int j = tid; j < 4*H; j += 256) {
			const float v = lineNeed[j];
			row[j] = v;
			if (j >= c) nextNeed[j - c] = v;
		}
		for (int ch = 0; ch < C; ++ch)
			for (int j = c + tid; j < L; j += 256) nextFrames[(size_t)ch*L + (j - c)] = lineFrames[(size_t)ch*L + j];
	}
	unsigned m[kLimitRun];
#pragma unroll
	for (int i = 0; i < kLimitRun; ++i) m[i] = 0u;
	const float *src = image + (size_t)s*imageStreamStride;
	const int at0 = 2*H + t0; // the image's first frame in [line, call]: the window of frame p - 6 + t0 begins kTruePeakHalo frames before the line's end
	for (int ch = 0; ch < C; ++ch) {
		if (ch) __syncthreads(); // (the image of the channel before has been read)
		const float *lineCh = lineFrames + (size_t)ch*L, *srcCh = src + (size_t)ch*imageChannelStride;
		float *nextCh = nextFrames + (size_t)ch*L;
		for (int i = tid; i < kTruePeakLds; i += 256) {
			const long long j = (long long)at0 + i; // (below L + c where a value is read)
			lds[i] = j < L ? lineCh[j] : j - L < c ? srcCh[j - L] : 0.0f;
		}
		// the call's frames t0 ... t0 + frames - 1 into the next line, where they are among its last L
		for (int i = tid; i < frames; i += 256) {
			const long long f = (long long)t0 + i, to = f + L - c;
			if (to >= 0) nextCh[to] = srcCh[f];
		}
		__syncthreads();
		if constexpr (Strided) {
#pragma unroll
			for (int i = 0; i < kLimitRun; ++i) {
				if (tid + 256*i >= frames) break;
				unsigned mc[1];
				truePeakFrameBits<1>(lds + tid + 256*i, taps, mc);
				m[i] = max(m[i], mc[0]);
			}
		} else if (tid*kLimitRun < frames) {
			unsigned mc[kLimitRun];
			truePeakFrameBits<kLimitRun>(lds + tid*kLimitRun, taps, mc);
#pragma unroll
			for (int i = 0; i < kLimitRun; ++i) m[i] = max(m[i], mc[i]);
		}
	}
	const float g = fabsf(l.gain);
#pragma unroll
	for (int i = 0; i < kLimitRun; ++i) {
		const int fl = Strided ? tid + 256*i : tid*kLimitRun + i;
		if (fl >= frames) continue;
		const long long f = (long long)t0 + fl, toNeed = f + 4*H - c; // (below the line's length: f < c)
		const float need = limitNeed(m[i], g, l.ceiling);
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
	const bool on = (l.flags & kPcmFlagStreamLimiter) != 0, late = (l.flags & kPcmFlagStreamLimitTruePeak) != 0;
	const int set = (l.flags & kPcmFlagStreamLimitSet) ? 1 : 0, pitch = late ? pcmStreamLimitTruePeakLine(lim.H) : 2*lim.H;
	const int delay = late ? 2*lim.H + kStreamLimitTruePeakDelay : 2*lim.H; // the last `delay` frames of each channel's row of the line
	const float *line = on ? (late ? lim.truePeakFrames[set] : lim.frames[set]) + (size_t)s*C*pitch + (pitch - delay) : nullptr;
	const float *r = on ? lim.rRow + (size_t)s*lim.rPitch : nullptr;
	unsigned over, peak;
	if (!pcmTileOut<T, Dith, true, true, true>(in + (size_t)s*inStreamStride, inChannelStride, out + (size_t)s*outStreamStride, outFrameStride, counts[s], blockIdx.x, C,
	                                           reinterpret_cast<float *>(smemRaw), over, dp, l.gain, &peak, r, line, delay, pitch)) return;
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
		const int L = pcmStreamLimitTruePeakLine(H);
		if (lim.truePeakFrames[set]) for (int j = threadIdx.x; j < C*L; j += 256) lim.truePeakFrames[set][(size_t)s*C*L + j] = 0.0f;
	}
}

void launchPcmLimitClear(const PcmStreamLimit &lim, int S, int C, int stream, hipStream_t st) {
	hipLaunchKernelGGL(kPcmLimitClear, dim3(stream < 0 ? S : 1), dim3(256), 0, st, lim, C, stream);
}

void launchPcmOutLimited(int format, const float *in, long long inStreamStride, long long inChannelStride, void *out, long long outStreamStride, long long outFrameStride,
                         const int *counts, int S, int C, int maxFrames, int maxLimited, int maxTruePeak, unsigned *overs, hipStream_t st, const PcmDither *dither,
                         const PcmLevelIo &level, const PcmStreamLimit &lim) {
	const int maxEither = std::max(maxLimited, maxTruePeak);
	if (maxEither < 1 || maxFrames < maxEither) throw std::invalid_argument("the limited output conversion needs a limited stream with frames");
	if (maxTruePeak >= 1 && !(lim.truePeakFrames[0] && lim.truePeakFrames[1])) throw std::invalid_argument("the stream limiter's true-peak lines are missing");
	if (maxLimited >= 1) {
		hipLaunchKernelGGL(kPcmLimitFeed, dim3(divUp(maxLimited, kLimitTile), S), dim3(256), 0, st, in, inStreamStride, inChannelStride, counts, C, level.table, lim);
		countLaunch(LK_PCM_LIMIT_FEED);
	}
	if (maxTruePeak >= 1) {
		const dim3 tiles(divUp(maxTruePeak, kLimitTile), S);
		if (maxTruePeak <= kStreamLimitTruePeakShort)
			hipLaunchKernelGGL(kPcmLimitFeedTruePeak<true>, tiles, dim3(256), limitNeedLdsBytes(), st, in, inStreamStride, inChannelStride, counts, C, level.table, truePeakTable(), lim);
		else
			hipLaunchKernelGGL(kPcmLimitFeedTruePeak<false>, tiles, dim3(256), limitNeedLdsBytes(), st, in, inStreamStride, inChannelStride, counts, C, level.table, truePeakTable(), lim);
		countLaunch(LK_PCM_LIMIT_FEED_TRUE_PEAK);
	}
	const dim3 tiles(divUp(maxEither, kLimitTile), S);
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
