// Whole clips of ragged lengths at the batch API's boundary (include/smst.h: smst_batch_exact, smst_batch_exact_pcm): the engine's kernels address
// caller memory as base + s*streamStride + c*channelStride + i, the same offsets for every stream, while exact() of S clips of S rates
// cuts every clip at places of its own (outputSeekLength(rate_s) in the input, outputIndex_s in the output).  So the engine runs on planar
// fp32 images of its own in which every stream's stage begins at one column, and the two kernels here move the clips: per stream two
// segments (ClipSeg, smst_device.h) of `count` frames from frame `src` of the source to frame `dst` of the destination.
//   kClipIn<T>   the caller's frames of format T -> the input image            (pcmTileIn of smst_pcm.h on a run that begins at the segment)
//   kClipOut<T, Dith, Level>  the output image -> the caller's frames, overs counted  (pcmTileOut; a "zeros" segment has no source; Dith: dithered;
//                Level: every stream's gain applied -- a whole-clip gain formed from the clip's peak --, its peak metered; a fourth flag,
//                Limit: a limited stream's frames multiplied by the gain curve of smst_limiter.h as well)
//   kClipPeak    the output image -> the peak of every stream's clip           (in front of a kClipOut that forms a whole-clip gain)
//   kClipPlanar  planar fp32 -> planar fp32, either direction                  (the caller's buffer is planar itself)
// Included by smst_state.hip only, behind smst_pcm.h: the conversion rule, the tiling of a run and the overs scheme are the ones defined there.
//
// Alignment.  A segment's offset moves the run's base address, so nothing is known about it beyond the element's alignment -- offsets that are
// no multiple of 4 frames are the normal case.  The frame kernels derive the first 16-byte group boundary from the run's ADDRESS
// (pcmTileRun), per segment.  kClipPlanar moves a row's run of floats through LDS: the tiles are cut on the DESTINATION's 16-byte
// boundaries (tile t > 0 begins `lead` floats behind t*kClipTileFloats), so every store in between is one aligned 16-byte store; the source is
// read as the aligned 16-byte words that cover the tile -- a word that reaches over the tile's edge but lies inside the run is read whole (a
// neighbour's floats, read twice, never written), so on both sides narrow accesses happen at a run's two ends only.  The LDS image is
// shifted so that the destination's groups are 16-byte aligned in LDS as well; the source side writes it dword by dword.
#pragma once
#include "smst_pcm.h"

namespace smst {

constexpr int kClipTileFloats = 2048; // floats of one row that one workgroup step of kClipPlanar moves
inline size_t clipPlanarLdsBytes() { return size_t(kClipTileFloats + 16)*sizeof(float); }

// frames of format T -> the planar image.  grid (tiles, S, 2 segments), 256 threads
template <typename T> __global__ __launch_bounds__(256) void kClipIn(const T *__restrict__ in, long long inStreamStride, long long inFrameStride,
		float *__restrict__ image, long long imageStreamStride, long long imageChannelStride, const ClipSeg *__restrict__ segs, int C) {
	extern __shared__ __attribute__((aligned(16))) unsigned char smemRaw[];
	const int s = blockIdx.y;
	const ClipSeg g = segs[2*s + blockIdx.z];
	if (g.count < 1 || g.zeros) return;
	pcmTileIn<T>(in + (size_t)s*inStreamStride + (size_t)g.src*inFrameStride, inFrameStride, g.count, image + (size_t)s*imageStreamStride + g.dst, imageChannelStride,
	             blockIdx.x, C, reinterpret_cast<float *>(smemRaw));
}

// the planar image -> frames of format T.  overs (may be null): [S][2] counters as kPcmOut's (a run of zeros adds nothing: 0.0 has a code in every format).
// Dith (int16 / int24): the frame index of a segment's first frame is its place in the clip, g.dst -- dither[s] gives the stream's mode and
// hash only --, so a clip's codes do not depend on where its two segments meet; a run of zeros stays the code of 0.0.
// Level: every workgroup forms its stream's gain by the same few correctly rounded fp32 operations (clipGain), so all of a clip's workgroups
// agree on it without another launch; the workgroup of the first tile of the stream's first segment that has a source reports it in
// level.applied[s]; a run of zeros is not levelled, metered or reported
// loudGain: gL of a stream in the loudness mode (kLoudGate's, smst_loudness.h), which takes the place of the entry's gain
// limited: the stream goes through the limiter (smst_limiter.h), which meets the ceiling frame by frame -- the form without the quotient
__device__ inline float clipGain(const PcmLevel &l, int peakBits, float loudGain, bool limited = false) {
	const float gain = l.mode == kPcmLevelLoudness ? loudGain : l.gain;
	if (limited || l.mode == kPcmLevelFixed || peakBits <= 0 || peakBits >= 0x7f800000) return gain; // (no peak, or none to divide by: the plain gain)
	const float q = l.ceiling/__int_as_float(peakBits);
	return (l.mode == kPcmLevelNormalise || !(gain <= q)) ? q : gain;
}
// Limit (a levelled launch in which a stream is limited): such a stream's gain is the limited form's and every frame is multiplied by
// level.limit[s*limitPitch + its clip position] as well -- the segment's dst is the position of its first frame; the other streams as Level
template <typename T, bool Dith, bool Level, bool Limit = false> __global__ __launch_bounds__(256) void kClipOut(const float *__restrict__ image, long long imageStreamStride, long long imageChannelStride,
		T *__restrict__ out, long long outStreamStride, long long outFrameStride, const ClipSeg *__restrict__ segs, int C, unsigned *__restrict__ overs, const PcmDither *__restrict__ dither,
		PcmLevelIo level) {
	extern __shared__ __attribute__((aligned(16))) unsigned char smemRaw[];
	const int s = blockIdx.y;
	const ClipSeg g = segs[2*s + blockIdx.z];
	if (g.count < 1) return;
	const float *src = g.zeros ? nullptr : image + (size_t)s*imageStreamStride + g.src;
	PcmDither dp{0u, 0u, 0u, 0u};
	if constexpr (Dith) dp = PcmDither{dither[s].mode, dither[s].h, unsigned(g.dst), 0u};
	unsigned over;
	if constexpr (Level) {
		const PcmLevel l = level.table[s];
		const int *clipPeak = (l.flags & kPcmFlagTruePeak) && level.truePeak ? level.truePeak : level.clipPeak; // (a flagged stream: its true peak, kClipTruePeak's)
		const bool limited = Limit && level.limit && pcmLimited(l);
		const float gain = clipGain(l, l.mode == kPcmLevelFixed ? 0 : clipPeak[s], l.mode == kPcmLevelLoudness && level.loudGain ? level.loudGain[s] : 1.0f, limited);
		const float *r = limited ? level.limit + (size_t)s*level.limitPitch + g.dst : nullptr;
		unsigned peak;
		if (!pcmTileOut<T, Dith, true, Limit>(src, imageChannelStride, out + (size_t)s*outStreamStride + (size_t)g.dst*outFrameStride, outFrameStride, g.count, blockIdx.x, C, reinterpret_cast<float *>(smemRaw), over, dp, gain, &peak, r)) return;
		if (src) {
			const ClipSeg first = segs[2*s];
			const bool reports = blockIdx.z == 0 || first.count < 1 || first.zeros; // (segment 1 reports where segment 0 has no source)
			if (reports && blockIdx.x == 0 && threadIdx.x == 0) level.applied[s] = gain;
			pcmMaxPeak(level.peaks, s, peak);
		}
	} else {
		if (!pcmTileOut<T, Dith>(src, imageChannelStride, out + (size_t)s*outStreamStride + (size_t)g.dst*outFrameStride, outFrameStride, g.count, blockIdx.x, C, reinterpret_cast<float *>(smemRaw), over, dp)) return;
	}
	pcmAddOvers(overs, s, over);
}

// The peak of every stream's clip: the largest pcmPeakBits of the image's samples that the stream's segments cover, into clipPeak[s].
// grid (tiles of kClipTileFloats frames, S, 2 segments), 256 threads; a workgroup takes its tile of every channel's row in turn, as the
// aligned 16-byte words inside the tile and, element by element, what lies in front of the first and behind the last of them (nothing
// outside the tile is read); lane maximum -> wavefront -> workgroup through LDS -> one atomicMax where the tile holds anything above 0
__global__ __launch_bounds__(256) void kClipPeak(const float *__restrict__ image, long long imageStreamStride, long long imageChannelStride, const ClipSeg *__restrict__ segs, int C,
		int *__restrict__ clipPeak) {
	extern __shared__ __attribute__((aligned(16))) unsigned char smemRaw[];
	int *waveMost = reinterpret_cast<int *>(smemRaw); // [4]
	const int s = blockIdx.y, tid = threadIdx.x;
	const ClipSeg g = segs[2*s + blockIdx.z];
	const int e0 = blockIdx.x*kClipTileFloats;
	if (g.count < 1 || g.zeros || e0 >= g.count) return;
	const int e1 = min(e0 + kClipTileFloats, g.count);
	unsigned most = 0u;
	for (int c = 0; c < C; ++c) {
		const float *row = image + (size_t)s*imageStreamStride + (size_t)c*imageChannelStride + g.src;
		const int back = int((reinterpret_cast<uintptr_t>(row + e0) >> 2) & 3u); // floats between the 16-byte boundary at or in front of row + e0 and it
		const int nWords = (back + e1 - e0 + 3)/4;
		for (int w = tid; w < nWords; w += 256) {
			const int a = e0 - back + 4*w; // the word's first element in the run
			if (a >= e0 && a + 4 <= e1) {
				const PcmWord4 v = *reinterpret_cast<const PcmWord4 *>(row + a);
				for (int k = 0; k < 4; ++k) most = max(most, pcmPeakBits(__int_as_float(int(v[k]))));
			} else {
				for (int k = 0; k < 4; ++k) if (a + k >= e0 && a + k < e1) most = max(most, pcmPeakBits(row[a + k]));
			}
		}
	}
	int m = int(most);
	for (int k = 32; k; k >>= 1) m = max(m, __shfl(m, (tid & 63) ^ k));
	if ((tid & 63) == 0) waveMost[tid >> 6] = m;
	__syncthreads();
	if (tid == 0) {
		m = max(max(waveMost[0], waveMost[1]), max(waveMost[2], waveMost[3]));
		if (m > 0) atomicMax(clipPeak + s, m);
	}
}

// Tile t of one row's run of `total` floats, src (null: zeros) -> dst, through `lds`.  Every lane of the workgroup calls it.
__device__ inline void clipRowTile(const float *__restrict__ src, float *__restrict__ dst, int total, int t, float *lds) {
	const int tid = threadIdx.x;
	const int lead = int((0 - (reinterpret_cast<uintptr_t>(dst) >> 2)) & 3u); // floats in front of dst's first 16-byte boundary
	const int e0 = t ? t*kClipTileFloats + lead : 0;
	if (e0 >= total) return;
	const int e1 = (t + 1)*kClipTileFloats + lead;
	const int count = (e1 < total ? e1 : total) - e0;
	const int head = t ? 0 : (lead < count ? lead : count);
	const int shift = (4 - head) & 3; // element e0 + i of the run at lds[shift + i]: the destination's groups begin at multiples of 4
	if (src) {
		const int back = int((reinterpret_cast<uintptr_t>(src + e0) >> 2) & 3u); // floats between the 16-byte boundary at or in front of src + e0 and it
		const int nWords = (back + count + 3)/4;
		for (int w = tid; w < nWords; w += 256) {
			const int a = e0 - back + 4*w;  // the word's first element in the run (negative / beyond the run only at the run's two ends)
			const int i = shift - back + 4*w; // ... and in lds
			if (a >= 0 && a + 4 <= total) {
				const PcmWord4 v = *reinterpret_cast<const PcmWord4 *>(src + a);
				for (int k = 0; k < 4; ++k) if (i + k >= 0) lds[i + k] = __int_as_float(int(v[k]));
			} else {
				for (int k = 0; k < 4; ++k) if (a + k >= 0 && a + k < total && i + k >= 0) lds[i + k] = src[a + k];
			}
		}
		__syncthreads();
	}
	pcmWalk(dst, 1, e0, count, head, 1, // (one channel, dense: dst's groups of 4 floats)
		[&](float &x, int i, const PcmPlace &) { x = src ? lds[shift + i] : 0.0f; },
		[&](float *p, int i, const PcmPlace &) {
			PcmWord4 v;
			for (int k = 0; k < 4; ++k) v[k] = src ? unsigned(__float_as_int(lds[shift + i + k])) : 0u;
			*reinterpret_cast<PcmWord4 *>(p) = v;
		});
	if (src) __syncthreads(); // (the next row's words go into the same image)
}

// planar fp32 -> planar fp32: src[s*srcStreamStride + c*srcChannelStride + seg.src + i] -> dst[s*dstStreamStride + c*dstChannelStride + seg.dst + i], i < seg.count.
// grid (tiles, S, 2 segments), 256 threads; a workgroup takes its tile of every channel's row in turn
__global__ __launch_bounds__(256) void kClipPlanar(const float *__restrict__ src, long long srcStreamStride, long long srcChannelStride,
		float *__restrict__ dst, long long dstStreamStride, long long dstChannelStride, const ClipSeg *__restrict__ segs, int C) {
	extern __shared__ __attribute__((aligned(16))) unsigned char smemRaw[];
	const int s = blockIdx.y;
	const ClipSeg g = segs[2*s + blockIdx.z];
	if (g.count < 1) return;
	for (int c = 0; c < C; ++c) {
		const float *from = g.zeros ? nullptr : src + (size_t)s*srcStreamStride + (size_t)c*srcChannelStride + g.src;
		clipRowTile(from, dst + (size_t)s*dstStreamStride + (size_t)c*dstChannelStride + g.dst, g.count, blockIdx.x, reinterpret_cast<float *>(smemRaw));
	}
}

// format 0: the caller's buffer is planar fp32 itself (kClipPlanar, either direction); else pcmDispatch of smst_pcm.h
static void launchClipPlanar(const float *src, long long srcSS, long long srcCS, float *dst, long long dstSS, long long dstCS, const ClipSeg *segs, int S, int C, int maxCount, hipStream_t st) {
	hipLaunchKernelGGL(kClipPlanar, dim3(divUp(maxCount, kClipTileFloats), S, 2), dim3(256), clipPlanarLdsBytes(), st, src, srcSS, srcCS, dst, dstSS, dstCS, segs, C);
}
void launchClipIn(int format, const void *in, long long inSS, long long inInner, float *image, long long imageSS, long long imageCS, const ClipSeg *segs, int S, int C, int maxCount, hipStream_t st) {
	if (maxCount < 1) return;
	const dim3 grid(divUp(maxCount, kPcmTileFrames), S, 2);
	if (format == 0) launchClipPlanar(static_cast<const float *>(in), inSS, inInner, image, imageSS, imageCS, segs, S, C, maxCount, st);
	else pcmDispatch(format, false, [&](auto tag, auto) {
		typedef typename decltype(tag)::type T;
		hipLaunchKernelGGL(kClipIn<T>, grid, dim3(256), pcmLdsBytes(C), st, static_cast<const T *>(in), inSS, inInner, image, imageSS, imageCS, segs, C);
	});
	countLaunch(LK_CLIP_IN);
}
void launchClipOut(int format, const float *image, long long imageSS, long long imageCS, void *out, long long outSS, long long outInner, const ClipSeg *segs, int S, int C, int maxCount,
                   unsigned *overs, hipStream_t st, const PcmDither *dither, const PcmLevelIo &level) {
	if (maxCount < 1) return;
	const dim3 grid(divUp(maxCount, kPcmTileFrames), S, 2);
	if (format == 0) {
		launchClipPlanar(image, imageSS, imageCS, static_cast<float *>(out), outSS, outInner, segs, S, C, maxCount, st);
		countLaunch(LK_CLIP_OUT);
		return;
	}
	pcmDispatch(format, dither != nullptr, [&](auto tag, auto dithered) {
		typedef typename decltype(tag)::type T;
		constexpr bool Dith = decltype(dithered)::value;
		const size_t lds = Dith ? pcmDitherLdsBytes(C) : pcmLdsBytes(C);
		if (level.table && level.limit) {
			hipLaunchKernelGGL((kClipOut<T, Dith, true, true>), grid, dim3(256), lds, st, image, imageSS, imageCS, static_cast<T *>(out), outSS, outInner, segs, C, overs, dither, level);
			countLaunch(LK_CLIP_OUT_LIMITED);
		} else if (level.table) {
			hipLaunchKernelGGL((kClipOut<T, Dith, true>), grid, dim3(256), lds, st, image, imageSS, imageCS, static_cast<T *>(out), outSS, outInner, segs, C, overs, dither, level);
			countLaunch(LK_CLIP_OUT_LEVELLED);
		} else {
			hipLaunchKernelGGL((kClipOut<T, Dith, false>), grid, dim3(256), lds, st, image, imageSS, imageCS, static_cast<T *>(out), outSS, outInner, segs, C, overs, dither, level);
			countLaunch(Dith ? LK_CLIP_OUT_DITHERED : LK_CLIP_OUT);
		}
	});
}
void launchClipPeak(const float *image, long long imageSS, long long imageCS, const ClipSeg *segs, int S, int C, int maxCount, int *clipPeak, hipStream_t st) {
	if (maxCount < 1) return;
	hipLaunchKernelGGL(kClipPeak, dim3(divUp(maxCount, kClipTileFloats), S, 2), dim3(256), 4*sizeof(int), st, image, imageSS, imageCS, segs, C, clipPeak);
	countLaunch(LK_CLIP_PEAK);
}

} // namespace smst
