// Interleaved PCM at the batch API's boundary (include/smst.h: smst_batch_*_pcm): frames of int16 or float32, channel-interleaved, to
// and from the dense planar fp32 image [S][C][maxLen] that the engine consumes and emits.  Included by smst_state.hip only.
//
// Conversion.  int16 -> float: float(v)/32768 (exact).  float -> int16: q = roundf(v*32768) -- ties away from zero --, clamped to
// [-32768, 32767], no dither: the rule tools/wav_io.h writes files with.  NaN gives 0; wav_io.h has no such case (its clamp turns a NaN
// into -32768): a NaN here is a fault of the signal path, and silence is the one code that is not a full-scale click.
//
// Shape.  A workgroup moves one tile of a stream's run -- kPcmTileFrames frames x C channels -- through LDS.  With frameStride == C the run
// is contiguous: it is read / written as 16-byte accesses (8 int16 or 4 floats per lane).  The pointers are aligned to the element only,
// so the run's first elements up to the first 16-byte boundary (tile 0) and its last ones behind the last whole 16 bytes (the last tile)
// go one by one; the tiles in between begin and end ON 16-byte boundaries (tile t > 0 begins `head` elements behind t*tile, in the middle
// of a frame if it has to), so narrow stores happen at a run's two ends only.  frameStride > C: every element goes by itself.
// The planar side is rows of consecutive frames, one dword per lane.
//
// LDS image: element e of the tile (interleaved order) at dword e + e/32 (one pad dword per 32).  The 16-byte side touches it as V
// ds_*_b32 per lane, lane stride V = 4 or 8 elements: lanes 4j..4j+3 (V = 8; 8j..8j+7 for V = 4) share a pad count and fill a residue
// class of banks, the next group is shifted by one -- 32 lanes, 32 banks, for every C.  The row side has lane stride C: conflict-free
// for C = 1, 2, 4, 8, 16 (the pad makes every 32/C-lane group start one bank further); for the other C one pad boundary inside the
// 32 lanes' span can put two lanes on a bank -- 2-way at the worst (brute force over C = 1..16, every channel and lane group), which
// a ds_write_b32 absorbs (kPcmOut) and which costs kPcmIn's ds_read_b32 one extra LDS cycle against ~100x that in memory time.
#pragma once
#include <cstdint>

namespace smst {

typedef unsigned PcmWord4 __attribute__((vector_size(16), may_alias)); // one 16-byte access

template <typename T> struct PcmFormat;
template <> struct PcmFormat<int16_t> {
	static constexpr int V = 8; // elements per 16 bytes
	static __device__ inline float decode(int16_t v) { return float(v)*(1.0f/32768.0f); }
	static __device__ inline int16_t encode(float v) {
		const float q = fminf(fmaxf(roundf(v*32768.0f), -32768.0f), 32767.0f);
		return (v != v) ? int16_t(0) : int16_t(int(q));
	}
	static __device__ inline void unpack(const PcmWord4 w, float *x) {
		for (int k = 0; k < 4; ++k) {
			x[2*k] = decode(int16_t(w[k] & 0xffffu));
			x[2*k + 1] = decode(int16_t(w[k] >> 16));
		}
	}
	static __device__ inline PcmWord4 pack(const float *x) {
		PcmWord4 w;
		for (int k = 0; k < 4; ++k) w[k] = unsigned(uint16_t(encode(x[2*k]))) | (unsigned(uint16_t(encode(x[2*k + 1]))) << 16);
		return w;
	}
};
template <> struct PcmFormat<float> {
	static constexpr int V = 4;
	static __device__ inline float decode(float v) { return v; }
	static __device__ inline float encode(float v) { return v; }
	static __device__ inline void unpack(const PcmWord4 w, float *x) {
		for (int k = 0; k < 4; ++k) x[k] = __int_as_float(int(w[k]));
	}
	static __device__ inline PcmWord4 pack(const float *x) {
		PcmWord4 w;
		for (int k = 0; k < 4; ++k) w[k] = unsigned(__float_as_int(x[k]));
		return w;
	}
};

__device__ inline int pcmSlot(int e) { return e + (e >> 5); }
inline size_t pcmLdsBytes(int C) { const int most = kPcmTileFrames*C + 8; return size_t(most + most/32 + 1)*sizeof(float); } // (tile 0 is up to V - 1 elements longer)

// The elements [e0, e0 + count) of a stream's run of `total` elements that tile `t` moves, and how many of them (tile 0 only) lie in
// front of the first 16-byte boundary.  false: the tile lies behind the run.
template <typename T> __device__ inline bool pcmTileRun(const T *run, long long total, bool dense, int t, int C, long long &e0, int &count, int &head) {
	constexpr int V = PcmFormat<T>::V;
	const int tileElems = kPcmTileFrames*C; // a multiple of 16 bytes
	const int misaligned = int((reinterpret_cast<uintptr_t>(run)/sizeof(T))%V);
	const int lead = dense ? (V - misaligned)%V : 0;
	e0 = t ? (long long)t*tileElems + lead : 0;
	if (e0 >= total) return false;
	const long long e1 = (long long)(t + 1)*tileElems + lead;
	count = int((e1 < total ? e1 : total) - e0);
	head = t ? 0 : (lead < count ? lead : count);
	return true;
}

// interleaved frames -> planar fp32.  grid (tiles, S), 256 threads; in[s*inStreamStride + i*inFrameStride + c] -> out[s*outStreamStride + c*outChannelStride + i], i < counts[s]
template <typename T> __global__ __launch_bounds__(256) void kPcmIn(const T *__restrict__ in, long long inStreamStride, long long inFrameStride,
		float *__restrict__ out, long long outStreamStride, long long outChannelStride, const int *__restrict__ counts, int C) {
	extern __shared__ __attribute__((aligned(16))) unsigned char smemRaw[];
	float *tile = reinterpret_cast<float *>(smemRaw);
	constexpr int V = PcmFormat<T>::V;
	const int s = blockIdx.y, tid = threadIdx.x;
	const T *run = in + (size_t)s*inStreamStride;
	const bool dense = inFrameStride == C;
	long long e0;
	int count, head;
	if (!pcmTileRun<T>(run, (long long)counts[s]*C, dense, blockIdx.x, C, e0, count, head)) return;
	if (dense) {
		const T *p = run + e0;
		if (tid < head) tile[pcmSlot(tid)] = PcmFormat<T>::decode(p[tid]);
		const int nVec = (count - head)/V;
		for (int v = tid; v < nVec; v += 256) {
			const int e = head + v*V;
			float x[V];
			PcmFormat<T>::unpack(*reinterpret_cast<const PcmWord4 *>(p + e), x);
			for (int k = 0; k < V; ++k) tile[pcmSlot(e + k)] = x[k];
		}
		const int done = head + nVec*V;
		if (tid < count - done) tile[pcmSlot(done + tid)] = PcmFormat<T>::decode(p[done + tid]);
	} else {
		for (int i = tid; i < count; i += 256) {
			const long long e = e0 + i, f = e/C;
			tile[pcmSlot(i)] = PcmFormat<T>::decode(run[f*inFrameStride + (e - f*C)]);
		}
	}
	__syncthreads();
	const long long f0 = e0/C; // (a tile may begin and end inside a frame: each element is moved by the tile that holds it)
	const int nFrames = int((e0 + count - 1)/C - f0) + 1;
	float *dst = out + (size_t)s*outStreamStride + f0;
	for (int c = 0; c < C; ++c) {
		const int first = int(f0*C + c - e0);
		for (int fl = tid; fl < nFrames; fl += 256) {
			const int i = first + fl*C;
			if (i >= 0 && i < count) dst[(size_t)c*outChannelStride + fl] = tile[pcmSlot(i)];
		}
	}
}

// planar fp32 -> interleaved frames: the reverse
template <typename T> __global__ __launch_bounds__(256) void kPcmOut(const float *__restrict__ in, long long inStreamStride, long long inChannelStride,
		T *__restrict__ out, long long outStreamStride, long long outFrameStride, const int *__restrict__ counts, int C) {
	extern __shared__ __attribute__((aligned(16))) unsigned char smemRaw[];
	float *tile = reinterpret_cast<float *>(smemRaw);
	constexpr int V = PcmFormat<T>::V;
	const int s = blockIdx.y, tid = threadIdx.x;
	T *run = out + (size_t)s*outStreamStride;
	const bool dense = outFrameStride == C;
	long long e0;
	int count, head;
	if (!pcmTileRun<T>(run, (long long)counts[s]*C, dense, blockIdx.x, C, e0, count, head)) return;
	const long long f0 = e0/C;
	const int nFrames = int((e0 + count - 1)/C - f0) + 1;
	const float *src = in + (size_t)s*inStreamStride + f0;
	for (int c = 0; c < C; ++c) {
		const int first = int(f0*C + c - e0);
		for (int fl = tid; fl < nFrames; fl += 256) {
			const int i = first + fl*C;
			if (i >= 0 && i < count) tile[pcmSlot(i)] = src[(size_t)c*inChannelStride + fl];
		}
	}
	__syncthreads();
	if (dense) {
		T *p = run + e0;
		if (tid < head) p[tid] = PcmFormat<T>::encode(tile[pcmSlot(tid)]);
		const int nVec = (count - head)/V;
		for (int v = tid; v < nVec; v += 256) {
			const int e = head + v*V;
			float x[V];
			for (int k = 0; k < V; ++k) x[k] = tile[pcmSlot(e + k)];
			*reinterpret_cast<PcmWord4 *>(p + e) = PcmFormat<T>::pack(x);
		}
		const int done = head + nVec*V;
		if (tid < count - done) p[done + tid] = PcmFormat<T>::encode(tile[pcmSlot(done + tid)]);
	} else {
		for (int i = tid; i < count; i += 256) {
			const long long e = e0 + i, f = e/C;
			run[f*outFrameStride + (e - f*C)] = PcmFormat<T>::encode(tile[pcmSlot(i)]);
		}
	}
}

// format: 1 = int16, 2 = float32 (SMST_PCM_S16 / SMST_PCM_F32; the C ABI has checked it).  maxFrames: the largest of the streams' counts.
void launchPcmIn(int format, const void *in, long long inStreamStride, long long inFrameStride, float *out, long long outStreamStride, long long outChannelStride,
                 const int *counts, int S, int C, int maxFrames, hipStream_t st) {
	if (maxFrames < 1) return;
	const dim3 grid(divUp(maxFrames, kPcmTileFrames), S);
	if (format == 1) hipLaunchKernelGGL(kPcmIn<int16_t>, grid, dim3(256), pcmLdsBytes(C), st, static_cast<const int16_t *>(in), inStreamStride, inFrameStride, out, outStreamStride, outChannelStride, counts, C);
	else hipLaunchKernelGGL(kPcmIn<float>, grid, dim3(256), pcmLdsBytes(C), st, static_cast<const float *>(in), inStreamStride, inFrameStride, out, outStreamStride, outChannelStride, counts, C);
	countLaunch(LK_PCM_IN);
}
void launchPcmOut(int format, const float *in, long long inStreamStride, long long inChannelStride, void *out, long long outStreamStride, long long outFrameStride,
                  const int *counts, int S, int C, int maxFrames, hipStream_t st) {
	if (maxFrames < 1) return;
	const dim3 grid(divUp(maxFrames, kPcmTileFrames), S);
	if (format == 1) hipLaunchKernelGGL(kPcmOut<int16_t>, grid, dim3(256), pcmLdsBytes(C), st, in, inStreamStride, inChannelStride, static_cast<int16_t *>(out), outStreamStride, outFrameStride, counts, C);
	else hipLaunchKernelGGL(kPcmOut<float>, grid, dim3(256), pcmLdsBytes(C), st, in, inStreamStride, inChannelStride, static_cast<float *>(out), outStreamStride, outFrameStride, counts, C);
	countLaunch(LK_PCM_OUT);
}

} // namespace smst
