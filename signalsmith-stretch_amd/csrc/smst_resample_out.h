// Sample-rate conversion of whole clips BEHIND the engine (include/smst.h, "Output resample", has the definition): Batch::exact of a frame-format
// call renders an out-resampled stream's E frames at the batch's rate into its output image as ever -- the frames [0, k) of the main process
// from one column, the flush's frames [k, E) from another --, and the kernel here forms the stream's Nd delivered frames from that two-piece
// clip into a third column of the same image, where the level stages and kClipOut then find them as one segment.
// Included by smst_state.hip only, behind smst_resample.h.  Everything up to the final rounding is float64.
//
// One kernel, kClipResample's shape: a workgroup takes a tile of kResampleTile delivered frames of one stream.  Frame n sits at rendered
// position n*M/L (i = (n*M)/L, p = (n*M) mod L); its T taps reach r(i - (H - 1)) ... r(i + H).  What differs is the source.  The tile's span
// [first, first + span) of rendered positions may lie in either piece or straddle the join k, which is any number in [0, E]: the part
// [a, min(b, k)) is staged from piece 0 and [max(a, k), b) from piece 1, each as a run of its own with loudStageWord (smst_loudness.h) -- the
// aligned 16-byte words of the SOURCE run that lie inside the piece read whole, the words at a piece's ends element by element, every float
// stored to its own LDS place.  So the second run's LDS offset need not be congruent to its source alignment: only the global side is read
// in words, by the source's own boundaries.  Positions outside [0, E) are 0.0; nothing outside the two pieces is read -- not the columns
// between piece 0's end and piece 1, not the room behind the flush.  Frames n >= Nd are not formed, though ceil(E*L/M) may exceed Nd.
//
// The tap sum is resampleFrameSum (smst_resample.h), the lane-to-frame mapping kClipResample's: float64 accumulators, no atomics, no scratch.
#pragma once
#include "smst_resample.h"

namespace smst {

// grid (tiles of kResampleTile delivered frames, S), 256 threads.  A stream without a ratio (L == 0), a tile behind the stream's Nd: returns at once.
// `image` and `out` are both __restrict__ although Batch::exact hands the SAME image for both: that holds only because what is read and what
// is written never overlap -- every read lies inside one of the two source pieces (loudStageWord reads a whole word only where all four
// floats are the piece's own, everything else element by element), and the destination runs lie in columns of their own behind both
// pieces (the engine's third column R >= Q + the longest flush).  A change that reads past a piece's end, or a caller whose destination
// overlaps a source piece, breaks it: take the qualifier off `out` first.
__global__ __launch_bounds__(256) void kClipResampleOut(const float *__restrict__ image, long long imageStreamStride, long long imageChannelStride,
		float *__restrict__ out, long long outStreamStride, long long outChannelStride, const ClipSeg *__restrict__ srcSegs, const ClipSeg *__restrict__ dstSegs,
		const ResampleOutEntry *__restrict__ entries, int C, int ldsFloats) {
	extern __shared__ __attribute__((aligned(16))) unsigned char smemRaw[];
	float *lds = reinterpret_cast<float *>(smemRaw);
	const int s = blockIdx.y, tid = threadIdx.x;
	const ResampleOutEntry e = entries[s];
	if (e.L < 1 || e.Nd < 1 || e.E < 1) return;
	const long long n0 = (long long)blockIdx.x*kResampleTile;
	if (n0 >= e.Nd) return;
	const int frames = int(min((long long)kResampleTile, e.Nd - n0));
	const long long at = n0*e.M;
	const int i0 = int(at/e.L), p0 = int(at%e.L);
	const int iLast = i0 + (p0 + (frames - 1)*e.M)/e.L;
	const int first = i0 - (e.H - 1), span = iLast - i0 + e.T;  // the rendered positions [first, first + span) at lds[0 ... span) of a channel's image
	const int pitch = resampleSpanPitch(e.L, e.M, e.T);
	const int group = min(min(kResampleGroup, C), ldsFloats/pitch);
	if (group < 1) return; // (the launcher sized the LDS for every entry: never)
	const ClipSeg r0 = srcSegs[2*s], r1 = srcSegs[2*s + 1];
	const int k = min(max(r0.count, 0), e.E);                  // the join: rendered frames [0, k) in piece 0, [k, E) in piece 1
	// [a, b): the rendered positions that the image holds, at lds[a - first ...); [a, mid) from piece 0, [mid, b) from piece 1
	const int a = max(first, 0), b = max(min(first + span, e.E), a), mid = min(max(k, a), b);
	const int nA = mid - a, nB = b - mid;
	const ClipSeg g0 = dstSegs[2*s], g1 = dstSegs[2*s + 1];
	const int split = max(g0.count, 0);
	for (int c0 = 0; c0 < C; c0 += group) {
		const int chans = min(group, C - c0);
		for (int ch = 0; ch < chans; ++ch) {
			float *img = lds + ch*pitch;
			const float *row = image + (size_t)s*imageStreamStride + (size_t)(c0 + ch)*imageChannelStride;
			for (int i = tid; i < span; i += 256) if (i < a - first || i >= b - first) img[i] = 0.0f;
			const float *runA = row + r0.src + a;              // rendered position a; the piece owns the indices [-a, k - a) around it
			const float *runB = row + r1.src + (mid - k);      // rendered position mid; the piece owns [-(mid - k), E - mid)
			const int wordsA = loudWordsOf(runA, nA), wordsB = loudWordsOf(runB, nB);
			for (int word = tid; word < wordsA + wordsB; word += 256) {
				if (word < wordsA) loudStageWord(runA, nA, word, -a, k - a, img + (a - first));
				else loudStageWord(runB, nB, word - wordsA, -(mid - k), e.E - mid, img + (mid - first));
			}
		}
		__syncthreads();
		for (int f = tid; f < frames; f += 256) {
			const int q = p0 + f*e.M, at0 = q/e.L, p = q - at0*e.L; // frame n0 + f: rendered position i0 + at0, phase p; its taps at lds[at0 ... at0 + T)
			const float *coef = e.taps + (size_t)p*e.pitch;
			const float *x = lds + at0;
			double y[kResampleGroup];
			resampleFrameSum(coef, x, pitch, e.T, chans, y);
			const long long nf = n0 + f;
			const size_t col = nf < split ? (size_t)g0.dst + (size_t)nf : (size_t)g1.dst + (size_t)(nf - split);
#pragma unroll
			for (int ch = 0; ch < kResampleGroup; ++ch) if (ch < chans) out[(size_t)s*outStreamStride + (size_t)(c0 + ch)*outChannelStride + col] = float(y[ch]);
		}
		__syncthreads(); // (the next group's spans go into the same image)
	}
}

void launchClipResampleOut(const float *image, long long imageSS, long long imageCS, float *out, long long outSS, long long outCS, const ClipSeg *srcSegs, const ClipSeg *dstSegs,
                           const ResampleOutEntry *entries, int S, int C, int maxFrames, int maxSpanPitch, hipStream_t st) {
	if (maxFrames < 1) return;
	const int ldsFloats = resampleLdsFloats(C, maxSpanPitch);
	hipLaunchKernelGGL(kClipResampleOut, dim3(divUp(maxFrames, kResampleTile), S), dim3(256), size_t(ldsFloats)*sizeof(float), st, image, imageSS, imageCS, out, outSS, outCS,
	                   srcSegs, dstSegs, entries, C, ldsFloats);
	countLaunch(LK_CLIP_RESAMPLE_OUT);
}

} // namespace smst
