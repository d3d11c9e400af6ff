// The sample-rate converter's streaming form in front of the engine (include/smst.h, "Stream resample", has the definition): a stream with the
// setting hands smst_batch_process_pcm / _seek_pcm frames at its own rate, kPcmIn puts them into a raw planar fp32 image, and the kernel here
// forms the k frames at the batch's rate that the call completes, straight into the engine's input image.  Included by smst_state.hip only,
// behind smst_resample.h, whose tap sum (resampleFrameSum) it shares: a stream cut into calls in any way hands the engine, bit for bit, the
// frames that kClipResample makes of the same material.
//
// What a stream carries: its LINE, the last T - 1 raw frames of every channel -- x(fed - (T - 1)) ... x(fed - 1) at [0, T - 1) of a row of
// kStreamResampleLine floats --, twice: a call reads the set its entry names and writes the other.  fed and made are the host's 64-bit
// counters and travel in the entry; nothing is read back.
//
// One kernel.  A workgroup takes a tile of kResampleTile of the call's k frames of one stream: frame made + f sits at i = ((made + f)*M)/L,
// p = ((made + f)*M) mod L, formed once per workgroup in 64 bits as kClipResample does, then stepped in 32 bits.  The tile's input span
// [i0 - (H - 1), iLast + H] is staged into LDS from TWO sources: a position q below fed comes from the line at q - (fed - (T - 1)), one at
// or above fed from the call's raw image at q - fed.  The call's first frame never reaches below fed - (T - 1) (made = ceil((fed - H)*L/M)
// puts i0 at or above fed - H) and its last never beyond fed + n - 1 (i + H <= fed + n - 1 is what makes a frame due); both are guarded all
// the same, with +0.0, so nothing outside the line and the image is read.  An entry with `fresh` reads zeros in the place of the line: that
// is how a cleared line looks, and a clear costs no launch.
// The workgroup behind a stream's last tile writes the stream's new line, x(fed + n - (T - 1)) ... x(fed + n - 1), from the same two
// sources into the other set; a stream with no frame in the call (n < 1) keeps its line and its set.
// No atomics, no scratch: the result does not depend on scheduling.
#pragma once
#include "smst_resample.h"

namespace smst {

// raw frame q of the stream's channel (an absolute position, fed - (T - 1) <= q < fed + n where the proofs above hold): +0.0 outside both sources
__device__ __forceinline__ float streamResampleAt(const StreamResampleEntry &e, const float *__restrict__ line, const float *__restrict__ row, long long q) {
	if (q < e.fed) {
		const long long at = q - (e.fed - (long long)(e.T - 1));
		return (e.fresh || at < 0) ? 0.0f : line[at];
	}
	const long long at = q - e.fed;
	return at < (long long)e.n ? row[at] : 0.0f;
}

// grid (tiles of kResampleTile of the call's frames + 1, S), 256 threads.  A stream without the setting (L == 0) or with no frame in the
// call (n < 1): returns at once.  tileFrames: the most frames a tile of this launch holds (sizes a channel's LDS image)
__global__ __launch_bounds__(256) void kPcmStreamResample(const float *__restrict__ raw, long long rawStreamStride, long long rawChannelStride,
		float *__restrict__ image, long long imageStreamStride, long long imageChannelStride, float *__restrict__ lines, long long lineSetStride,
		const StreamResampleEntry *__restrict__ entries, int C, int tileFrames, int ldsFloats) {
	extern __shared__ __attribute__((aligned(16))) unsigned char smemRaw[];
	float *lds = reinterpret_cast<float *>(smemRaw);
	const int s = blockIdx.y, tid = threadIdx.x;
	const StreamResampleEntry e = entries[s];
	if (e.L < 1 || e.n < 1) return;
	const float *lineIn = lines + (size_t)(e.set & 1)*lineSetStride + (size_t)s*C*kStreamResampleLine;
	const long long f0 = (long long)blockIdx.x*kResampleTile;
	if (f0 >= e.k) {
		if ((int)blockIdx.x != (max(e.k, 0) + kResampleTile - 1)/kResampleTile) return;
		// the stream's new line: x(fed + n - (T - 1) + j) at [j], into the other set
		float *lineOut = lines + (size_t)((e.set & 1) ^ 1)*lineSetStride + (size_t)s*C*kStreamResampleLine;
		const long long from = e.fed + (long long)e.n - (long long)(e.T - 1);
		for (int at = tid; at < C*(e.T - 1); at += 256) {
			const int c = at/(e.T - 1), j = at - c*(e.T - 1);
			lineOut[(size_t)c*kStreamResampleLine + j] = streamResampleAt(e, lineIn + (size_t)c*kStreamResampleLine, raw + (size_t)s*rawStreamStride + (size_t)c*rawChannelStride + e.rawAt, from + j);
		}
		return;
	}
	const int frames = int(min((long long)kResampleTile, (long long)e.k - f0));
	const long long n0 = e.made + f0, at = n0*e.M;
	const long long i0 = at/e.L;
	const int p0 = int(at%e.L);
	const int reach = (p0 + (frames - 1)*e.M)/e.L;            // iLast - i0
	const long long first = i0 - (long long)(e.H - 1);
	const int span = reach + e.T;                             // the stream's positions [first, first + span) at lds[0 ... span) of a channel's image
	const int pitch = resampleSpanPitchOf(e.L, e.M, e.T, tileFrames);
	const int group = min(min(kResampleGroup, C), ldsFloats/pitch);
	if (group < 1 || span > pitch) return; // (the launcher sized the LDS for every entry: never)
	for (int c0 = 0; c0 < C; c0 += group) {
		const int chans = min(group, C - c0);
		for (int k = 0; k < chans; ++k) {
			float *img = lds + k*pitch;
			const float *row = raw + (size_t)s*rawStreamStride + (size_t)(c0 + k)*rawChannelStride + e.rawAt;
			const float *line = lineIn + (size_t)(c0 + k)*kStreamResampleLine;
			for (int i = tid; i < span; i += 256) img[i] = streamResampleAt(e, line, row, first + i);
		}
		__syncthreads();
		for (int f = tid; f < frames; f += 256) {
			const int q = p0 + f*e.M, at0 = q/e.L, p = q - at0*e.L; // frame n0 + f: input position i0 + at0, phase p; its taps at lds[at0 ... at0 + T)
			double y[kResampleGroup];
			resampleFrameSum(e.taps + (size_t)p*e.pitch, lds + at0, pitch, e.T, chans, y);
			const size_t col = (size_t)e.outAt + (size_t)(f0 + f);
#pragma unroll
			for (int k = 0; k < kResampleGroup; ++k) if (k < chans) image[(size_t)s*imageStreamStride + (size_t)(c0 + k)*imageChannelStride + col] = float(y[k]);
		}
		__syncthreads(); // (the next group's spans go into the same image)
	}
}

void launchPcmStreamResample(const float *raw, long long rawSS, long long rawCS, float *image, long long imageSS, long long imageCS, float *lines, long long lineSetStride,
                             const StreamResampleEntry *entries, int S, int C, int maxFrames, int maxSpanPitch, hipStream_t st) {
	const int tileFrames = streamResampleTileFrames(maxFrames);
	const int ldsFloats = resampleLdsFloats(C, maxSpanPitch);
	hipLaunchKernelGGL(kPcmStreamResample, dim3(divUp(std::max(maxFrames, 0), kResampleTile) + 1, S), dim3(256), size_t(ldsFloats)*sizeof(float), st, raw, rawSS, rawCS, image, imageSS, imageCS,
	                   lines, lineSetStride, entries, C, tileFrames, ldsFloats);
	countLaunch(LK_PCM_STREAM_RESAMPLE);
}

} // namespace smst
