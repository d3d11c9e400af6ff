// Sample-rate conversion of whole clips in front of the engine (include/smst.h, "Resample", has the definition): Batch::exact of a frame-format
// call moves a resampled stream's whole clip into a raw planar fp32 image (kClipIn, one segment from column 0), and the kernel here forms the
// stream's frames at the batch's rate from it, straight into the engine's input image where the call's two input segments put them.
// Included by smst_state.hip only, behind smst_clip.h.  Everything up to the final rounding is float64.
//
// One kernel.  A workgroup takes a tile of kResampleTile resampled frames of one stream.  Frame n sits at input position n*M/L: i = (n*M)/L,
// p = (n*M) mod L; its T taps reach x(i - (H - 1)) ... x(i + H).  The tile's first frame n0 gives i0 and p0 (64-bit, once per workgroup); frame
// n0 + f then has i = i0 + (p0 + f*M)/L and p = (p0 + f*M) mod L in 32 bits (f*M < 1024*640).  The input span [i0 - (H - 1), iLast + H] of a
// channel, at most ceil(1023*M/L) + T floats, is staged into LDS with truePeakStage's idiom (loudStageWord, smst_loudness.h): the aligned
// 16-byte words that cover the part inside [0, N), one that lies inside the row read whole, one at the row's ends element by element; positions
// outside [0, N) are 0.0.  Nothing outside a stream's rows is read.
//
// The channels of a tile go in groups of up to kResampleGroup that fit the launch's LDS.  A lane takes the frames f = lane, lane + 256, ...;
// per frame it keeps one float64 accumulator per channel of the group and walks its phase's row of the table once, as aligned 16-byte words
// (rows are padded to a multiple of 4 floats; the padding is never multiplied: 0*inf would be NaN).  Every product of two float32 values is
// exact in float64, so y is the same whether or not a*b + y is contracted into an FMA; the sum runs j = 0 ... T - 1 from 0.0.  No atomics,
// no scratch: the result does not depend on scheduling.
#pragma once
#include "smst_loudness.h"
#include <cmath>
#include <vector>

namespace smst {

constexpr int kResampleGroup = 4; // channels whose accumulators a lane keeps side by side
static_assert(kResampleTile%256 == 0, "a tile is whole passes of the workgroup's lanes");

// c[p][j] = float32(h/sum_j h), h = rho*sinc(rho*t)*I0(10*sqrt(1 - (t/W)^2))/I0(10) for |t| < W, t = (j - (H - 1)) - p/L: in double, each
// phase normalised to unit DC gain, one rounding.  I0 by its power series (terms below 1e-17 of the sum dropped)
static double resampleBesselI0(double x) {
	const double q = x*x/4;
	double term = 1.0, sum = 1.0;
	for (int k = 1; k < 200; ++k) {
		term *= q/(double(k)*double(k));
		sum += term;
		if (term < 1e-17*sum) break;
	}
	return sum;
}
void resampleTaps(const ResampleShape &g, float *out) {
	const double pi = 3.14159265358979323846;
	const double r = g.L < g.M ? double(g.L)/double(g.M) : 1.0, rho = 0.98*r, W = g.L < g.M ? 32.0*double(g.M)/double(g.L) : 32.0, i0Ten = resampleBesselI0(10.0);
	std::vector<double> h((size_t)g.T);
	for (int p = 0; p < g.L; ++p) {
		double sum = 0.0;
		for (int j = 0; j < g.T; ++j) {
			const double t = double(j - (g.H - 1)) - double(p)/double(g.L);
			double v = 0.0;
			if (std::fabs(t) < W) {
				const double x = pi*rho*t, u = t/W;
				v = rho*(x == 0.0 ? 1.0 : std::sin(x)/x)*resampleBesselI0(10.0*std::sqrt(1.0 - u*u))/i0Ten;
			}
			h[j] = v;
			sum += v;
		}
		float *row = out + (size_t)p*g.pitch;
		for (int j = 0; j < g.pitch; ++j) row[j] = j < g.T ? float(h[j]/sum) : 0.0f;
	}
}

// One resampled frame of the `chans` channels of a group: y[k] = sum_j double(coef[j])*double(x[k*pitch + j]), j = 0 ... T - 1 from 0.0 -- the
// frame's T taps lie at x[0 ... T) of each channel's LDS image, `pitch` floats apart; coef: the phase's row of the table, 16-byte aligned.
// The one definition of the tap sum: kClipResample and kPcmStreamResample (smst_stream_resample.h) both call it
__device__ __forceinline__ void resampleFrameSum(const float *__restrict__ coef, const float *x, int pitch, int T, int chans, double (&y)[kResampleGroup]) {
#pragma unroll
	for (int k = 0; k < kResampleGroup; ++k) y[k] = 0.0;
	const int whole = T & ~3;
	for (int j = 0; j < whole; j += 4) {
		const PcmWord4 v = *reinterpret_cast<const PcmWord4 *>(coef + j);
#pragma unroll
		for (int i = 0; i < 4; ++i) {
			const double w = double(__int_as_float(int(v[i])));
#pragma unroll
			for (int k = 0; k < kResampleGroup; ++k) if (k < chans) y[k] += w*double(x[k*pitch + j + i]);
		}
	}
	for (int j = whole; j < T; ++j) { // (T is even: two taps where it is no multiple of 4)
		const double w = double(coef[j]);
#pragma unroll
		for (int k = 0; k < kResampleGroup; ++k) if (k < chans) y[k] += w*double(x[k*pitch + j]);
	}
}

// grid (tiles of kResampleTile resampled frames, S), 256 threads.  A stream without a ratio (L == 0), a tile behind the stream's Nr: returns at once
__global__ __launch_bounds__(256) void kClipResample(const float *__restrict__ raw, long long rawStreamStride, long long rawChannelStride,
		float *__restrict__ image, long long imageStreamStride, long long imageChannelStride, const ClipSeg *__restrict__ segs, const ResampleEntry *__restrict__ entries, int C, int ldsFloats) {
	extern __shared__ __attribute__((aligned(16))) unsigned char smemRaw[];
	float *lds = reinterpret_cast<float *>(smemRaw);
	const int s = blockIdx.y, tid = threadIdx.x;
	const ResampleEntry e = entries[s];
	if (e.L < 1 || e.Nr < 1) return;
	const long long n0 = (long long)blockIdx.x*kResampleTile;
	if (n0 >= e.Nr) return;
	const int frames = int(min((long long)kResampleTile, e.Nr - n0));
	const long long at = n0*e.M;
	const int i0 = int(at/e.L), p0 = int(at%e.L);
	const int iLast = i0 + (p0 + (frames - 1)*e.M)/e.L;
	const int first = i0 - (e.H - 1), span = iLast - i0 + e.T;  // the clip's positions [first, first + span) at lds[0 ... span) of a channel's image
	const int pitch = resampleSpanPitch(e.L, e.M, e.T);
	const int group = min(min(kResampleGroup, C), ldsFloats/pitch);
	if (group < 1) return; // (the launcher sized the LDS for every entry: never)
	// [a, b): the clip's positions that the image holds, at lds[a - first ...); the rest of it is 0.0
	const int a = max(first, 0), b = min(first + span, e.N), n = max(b - a, 0);
	const ClipSeg g0 = segs[2*s], g1 = segs[2*s + 1];
	const int split = max(g0.count, 0);
	for (int c0 = 0; c0 < C; c0 += group) {
		const int chans = min(group, C - c0);
		for (int k = 0; k < chans; ++k) {
			float *img = lds + k*pitch;
			const float *row = raw + (size_t)s*rawStreamStride + (size_t)(c0 + k)*rawChannelStride;
			for (int i = tid; i < span; i += 256) if (i < a - first || i >= b - first) img[i] = 0.0f;
			const float *run = row + a;
			const int words = loudWordsOf(run, n);
			for (int word = tid; word < words; word += 256) loudStageWord(run, n, word, -a, e.N - a, img + (a - first));
		}
		__syncthreads();
		for (int f = tid; f < frames; f += 256) {
			const int q = p0 + f*e.M, at0 = q/e.L, p = q - at0*e.L; // frame n0 + f: input position i0 + at0, phase p; its taps at lds[at0 ... at0 + T)
			const float *coef = e.taps + (size_t)p*e.pitch;
			const float *x = lds + at0;
			double y[kResampleGroup];
			resampleFrameSum(coef, x, pitch, e.T, chans, y);
			const long long nf = n0 + f;
			const size_t col = nf < split ? (size_t)g0.dst + (size_t)nf : (size_t)g1.dst + (size_t)(nf - split);
#pragma unroll
			for (int k = 0; k < kResampleGroup; ++k) if (k < chans) image[(size_t)s*imageStreamStride + (size_t)(c0 + k)*imageChannelStride + col] = float(y[k]);
		}
		__syncthreads(); // (the next group's spans go into the same image)
	}
}

void launchClipResample(const float *raw, long long rawSS, long long rawCS, float *image, long long imageSS, long long imageCS, const ClipSeg *segs, const ResampleEntry *entries,
                        int S, int C, int maxFrames, int maxSpanPitch, hipStream_t st) {
	if (maxFrames < 1) return;
	const int ldsFloats = resampleLdsFloats(C, maxSpanPitch);
	hipLaunchKernelGGL(kClipResample, dim3(divUp(maxFrames, kResampleTile), S), dim3(256), size_t(ldsFloats)*sizeof(float), st, raw, rawSS, rawCS, image, imageSS, imageCS, segs, entries, C, ldsFloats);
	countLaunch(LK_CLIP_RESAMPLE);
}

} // namespace smst
