// The sample-rate converter's streaming form BEHIND the engine (include/smst.h, "Stream output resample", has the definition): a stream with
// the setting receives the frames of smst_batch_process_pcm / _flush_pcm at its own delivery rate.  The engine renders the call's E frames
// into its output image as ever; the kernel here forms the call's Nd delivered frames from the stream's carried line and those E frames into
// a second image, and a small copy puts them back over the stream's rows of the engine's image, so that every output stage behind it --
// limiter, meter, gain, dither, conversion, overs, peaks -- reads one image, as it did, and sees the frames that are delivered.  Included by
// smst_state.hip only, behind smst_resample.h, whose tap sum (resampleFrameSum) it shares with the three other converters.
//
// Positions.  r(0), r(1), ... are the frames rendered for the stream since its line was last cleared; `delivered` frames have been
// delivered and rendered = ceil(delivered*M/L) rendered (the host's 64-bit counters, which travel in the entry; nothing is read back).
// The call delivers the frames n = delivered ... delivered + Nd - 1 and renders r(rendered) ... r(rendered + E - 1),
// rendered + E = ceil((delivered + Nd)*M/L).  Frame n < Dl = ceil(H*L/M) is +0.0; frame n >= Dl is frame m = n - Dl of "Resample" applied to
// r: i = (m*M)/L, p = (m*M) mod L, taps r(i - (H - 1)) ... r(i + H).
//
// The right edge never enters, so the cuts do not matter.  Dl*M/L >= H, hence i = floor((n - Dl)*M/L) <= n*M/L - H, and i + H, a whole
// number, is at most floor(n*M/L).  ceil((n + 1)*M/L) >= (n + 1)*M/L > n*M/L >= floor(n*M/L), a whole number strictly above it, so
// i + H <= ceil((n + 1)*M/L) - 1 <= rendered + E - 1 for every n of the call: the last tap of every frame is a frame that HAS been rendered,
// in this call or before it, whatever the call's Nd.  The left edge is the line's length (smst_device.h derives T + ceil(M/L) <= 293).
//
// What a stream carries: its LINE, the last kStreamResampleOutLine rendered frames of every channel -- r(rendered - kStreamResampleOutLine + j)
// at [j] of a row --, twice: a call reads the set its entry names and writes the other.
//
// kPcmStreamResampleOut.  A workgroup takes a tile of kResampleTile of the call's Nd frames of one stream.  The tile's leading frames with
// n < Dl are written as +0.0.  The first of the others gives i0 and p0, formed once per workgroup in 64 bits, then stepped in 32 bits as
// kClipResample does.  The tile's span [i0 - (H - 1), iLast + H] is staged into LDS from TWO sources: a position q below `rendered` comes
// from the line at q - (rendered - kStreamResampleOutLine), one at or above it from the call's rendered image at q - rendered.  Both are
// guarded all the same, with +0.0 -- below the line, at or behind E, and everywhere in the line of an entry with `fresh` (that is how a
// cleared line looks, and a clear costs no launch) --, so nothing outside the line and the stream's E frames is read.
// The workgroup behind a stream's last tile writes the stream's new line, r(rendered + E - kStreamResampleOutLine + j), from the same two
// sources into the other set; a stream with no frame in the call (Nd < 1) keeps its line and its set.
// No atomics, no scratch memory: the result does not depend on scheduling.
#pragma once
#include "smst_resample.h"

namespace smst {

// rendered frame q of the stream's channel (an absolute position): +0.0 outside both sources
__device__ __forceinline__ float streamResampleOutAt(const StreamResampleOutEntry &e, const float *__restrict__ line, const float *__restrict__ row, long long q) {
	if (q < e.rendered) {
		const long long at = q - (e.rendered - (long long)kStreamResampleOutLine);
		return (e.fresh || at < 0) ? 0.0f : line[at];
	}
	const long long at = q - e.rendered;
	return at < (long long)e.E ? row[at] : 0.0f;
}

// grid (tiles of kResampleTile of the call's delivered frames + 1, S), 256 threads.  A stream without the setting (L == 0) or with no frame
// in the call (Nd < 1): returns at once.  tileFrames: the most frames a tile of this launch holds (sizes a channel's LDS image)
__global__ __launch_bounds__(256) void kPcmStreamResampleOut(const float *__restrict__ image, long long imageStreamStride, long long imageChannelStride,
		float *__restrict__ out, long long outStreamStride, long long outChannelStride, float *__restrict__ lines, long long lineSetStride,
		const StreamResampleOutEntry *__restrict__ entries, int C, int tileFrames, int ldsFloats) {
	extern __shared__ __attribute__((aligned(16))) unsigned char smemRaw[];
	float *lds = reinterpret_cast<float *>(smemRaw);
	const int s = blockIdx.y, tid = threadIdx.x;
	const StreamResampleOutEntry e = entries[s];
	if (e.L < 1 || e.Nd < 1) return;
	const float *lineIn = lines + (size_t)(e.set & 1)*lineSetStride + (size_t)s*C*kStreamResampleOutLine;
	const long long f0 = (long long)blockIdx.x*kResampleTile;
	if (f0 >= e.Nd) {
		if ((int)blockIdx.x != (e.Nd + kResampleTile - 1)/kResampleTile) return;
		// the stream's new line: r(rendered + E - kStreamResampleOutLine + j) at [j], into the other set
		float *lineOut = lines + (size_t)((e.set & 1) ^ 1)*lineSetStride + (size_t)s*C*kStreamResampleOutLine;
		const long long from = e.rendered + (long long)e.E - (long long)kStreamResampleOutLine;
		for (int at = tid; at < C*kStreamResampleOutLine; at += 256) {
			const int c = at/kStreamResampleOutLine, j = at - c*kStreamResampleOutLine;
			lineOut[(size_t)c*kStreamResampleOutLine + j] = streamResampleOutAt(e, lineIn + (size_t)c*kStreamResampleOutLine, image + (size_t)s*imageStreamStride + (size_t)c*imageChannelStride + e.imageAt, from + j);
		}
		return;
	}
	const int frames = int(min((long long)kResampleTile, (long long)e.Nd - f0));
	// the tile's frames n0 ... n0 + frames - 1; the first `zeros` of them lie below Dl
	const long long n0 = e.delivered + f0;
	const int zeros = int(min((long long)frames, max(0LL, (long long)e.Dl - n0)));
	const int live = frames - zeros;
	const long long at = (n0 + zeros - (long long)e.Dl)*e.M;     // (m of the first live frame)*M, m >= 0
	const long long i0 = live > 0 ? at/e.L : 0;
	const int p0 = live > 0 ? int(at%e.L) : 0;
	const int reach = live > 0 ? (p0 + (live - 1)*e.M)/e.L : 0;  // iLast - i0
	const long long first = i0 - (long long)(e.H - 1);
	const int span = reach + e.T;                                // the stream's positions [first, first + span) at lds[0 ... span) of a channel's image
	const int pitch = resampleSpanPitchOf(e.L, e.M, e.T, tileFrames);
	const int group = min(min(kResampleGroup, C), ldsFloats/pitch);
	if (group < 1 || span > pitch) return; // (the launcher sized the LDS for every entry: never)
	for (int c0 = 0; c0 < C; c0 += group) {
		const int chans = min(group, C - c0);
		if (live > 0) {
			for (int k = 0; k < chans; ++k) {
				float *img = lds + k*pitch;
				const float *row = image + (size_t)s*imageStreamStride + (size_t)(c0 + k)*imageChannelStride + e.imageAt;
				const float *line = lineIn + (size_t)(c0 + k)*kStreamResampleOutLine;
				for (int i = tid; i < span; i += 256) img[i] = streamResampleOutAt(e, line, row, first + i);
			}
		}
		__syncthreads();
		for (int f = tid; f < frames; f += 256) {
			const size_t col = (size_t)e.outAt + (size_t)(f0 + f);
			if (f < zeros) {
				for (int k = 0; k < chans; ++k) out[(size_t)s*outStreamStride + (size_t)(c0 + k)*outChannelStride + col] = 0.0f;
				continue;
			}
			const int q = p0 + (f - zeros)*e.M, at0 = q/e.L, p = q - at0*e.L; // frame n0 + f: rendered position i0 + at0, phase p; its taps at lds[at0 ... at0 + T)
			double y[kResampleGroup];
			resampleFrameSum(e.taps + (size_t)p*e.pitch, lds + at0, pitch, e.T, chans, y);
#pragma unroll
			for (int k = 0; k < kResampleGroup; ++k) if (k < chans) out[(size_t)s*outStreamStride + (size_t)(c0 + k)*outChannelStride + col] = float(y[k]);
		}
		__syncthreads(); // (the next group's spans go into the same image)
	}
}

// grid (tiles of kResampleTile of the call's delivered frames, S), 256 threads: out's frames [outAt, outAt + Nd) of every channel of a stream
// that has the setting, over image's [imageAt, imageAt + Nd)
__global__ __launch_bounds__(256) void kPcmStreamResampleOutCopy(const float *__restrict__ from, long long fromStreamStride, long long fromChannelStride,
		float *__restrict__ image, long long imageStreamStride, long long imageChannelStride, const StreamResampleOutEntry *__restrict__ entries, int C) {
	const int s = blockIdx.y, tid = threadIdx.x;
	const StreamResampleOutEntry e = entries[s];
	if (e.L < 1 || e.Nd < 1) return;
	const long long f0 = (long long)blockIdx.x*kResampleTile;
	if (f0 >= e.Nd) return;
	const int frames = int(min((long long)kResampleTile, (long long)e.Nd - f0));
	for (int c = 0; c < C; ++c) {
		const float *src = from + (size_t)s*fromStreamStride + (size_t)c*fromChannelStride + (size_t)e.outAt + (size_t)f0;
		float *dst = image + (size_t)s*imageStreamStride + (size_t)c*imageChannelStride + (size_t)e.imageAt + (size_t)f0;
		for (int f = tid; f < frames; f += 256) dst[f] = src[f];
	}
}

void launchPcmStreamResampleOut(const float *image, long long imageSS, long long imageCS, float *out, long long outSS, long long outCS, float *lines, long long lineSetStride,
                                const StreamResampleOutEntry *entries, int S, int C, int maxFrames, int maxSpanPitch, hipStream_t st) {
	if (maxFrames < 1) return;
	const int tileFrames = streamResampleTileFrames(maxFrames);
	const int ldsFloats = resampleLdsFloats(C, maxSpanPitch);
	hipLaunchKernelGGL(kPcmStreamResampleOut, dim3(divUp(maxFrames, kResampleTile) + 1, S), dim3(256), size_t(ldsFloats)*sizeof(float), st, image, imageSS, imageCS, out, outSS, outCS,
	                   lines, lineSetStride, entries, C, tileFrames, ldsFloats);
	countLaunch(LK_PCM_STREAM_RESAMPLE_OUT);
}

void launchPcmStreamResampleOutCopy(const float *from, long long fromSS, long long fromCS, float *image, long long imageSS, long long imageCS,
                                    const StreamResampleOutEntry *entries, int S, int C, int maxFrames, hipStream_t st) {
	if (maxFrames < 1) return;
	hipLaunchKernelGGL(kPcmStreamResampleOutCopy, dim3(divUp(maxFrames, kResampleTile), S), dim3(256), 0, st, from, fromSS, fromCS, image, imageSS, imageCS, entries, C);
	countLaunch(LK_PCM_STREAM_RESAMPLE_OUT_COPY);
}

} // namespace smst
