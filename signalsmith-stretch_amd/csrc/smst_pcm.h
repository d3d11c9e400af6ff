// Interleaved PCM at the batch API's boundary (include/smst.h: smst_batch_*_pcm): frames of int16, packed int24, int32, float16 or
// float32, channel-interleaved, to and from the dense planar fp32 image [S][C][maxLen] that the engine consumes and emits.  Included by
// smst_state.hip only.
//
// Conversion.  int16 -> float: float(v)/32768 (exact).  float -> int16: q = roundf(v*32768) -- ties away from zero --, clamped to
// [-32768, 32767], no dither unless a stream asks for it ("Dither" below): the rule tools/wav_io.h writes files with.  NaN gives 0; wav_io.h has no such case (its clamp turns a NaN
// into -32768): a NaN here is a fault of the signal path, and silence is the one code that is not a full-scale click.
// int24 (3 bytes, little-endian, packed) and int32: the same rule at full scale 2^23 and 2^31; an int32 above 2^24 is rounded to float32
// (nearest even) on the way in, and the way out clamps the FLOAT before it becomes an integer (2^31 and above give 2147483647).
// float16: widened exactly; narrowed round-to-nearest-even, subnormals kept, beyond 65520 to +-inf, NaN stays NaN.
//
// Shape.  A workgroup moves one tile of a stream's run -- kPcmTileFrames frames x C channels -- through LDS.  With frameStride == C the run
// is contiguous: it is read / written in GROUPS of G elements that fill W aligned 16-byte words (8 int16 / 4 floats in one word; 16 int24
// in three: 3 is invertible mod 16, so whatever the base address one sample boundary in every 16 lies on a 16-byte boundary), W 16-byte
// accesses per lane.  The pointers are aligned to the element only (int24: to the byte), so the run's first elements up to the first
// group boundary (tile 0, at most G - 1) and its last ones behind the last whole group (the last tile) go one by one; the tiles in
// between begin and end ON group boundaries (tile t > 0 begins `head` elements behind t*tile, in the middle of a frame if it has to: a
// tile is a whole number of groups for every C), so narrow accesses happen at a run's two ends only.  frameStride > C: every element goes
// by itself.  The planar side is rows of consecutive frames, one dword per lane.
//
// LDS image: element e of the tile (interleaved order) at dword e + e/32 (one pad dword per 32).  The group side touches it as G
// ds_*_b32 per lane, lane stride G = 4, 8 or 16 elements: lanes 4j..4j+3 (G = 8; 8j..8j+7 for G = 4, 2j and 2j+1 for G = 16) share a pad
// count and fill a residue class of banks, the next set is shifted by one -- 32 lanes, 32 banks, for every C.  The row side has lane
// stride C: conflict-free for C = 1, 2, 4, 8, 16 (the pad makes every 32/C-lane group start one bank further); for the other C one pad
// boundary inside the 32 lanes' span can put two lanes on a bank -- 2-way at the worst (brute force over C = 1..16, every channel and
// lane group), which a ds_write_b32 absorbs (kPcmOut) and which costs kPcmIn's ds_read_b32 one extra LDS cycle against ~100x that in
// memory time.
//
// Overs.  kPcmOut counts what the conversion could not represent: per lane one word, clamped (or, float16, turned +-inf from a finite
// value) in its low half and NaN inputs in its high half -- a lane converts some 35 elements of a tile at the most --, summed over the
// wavefront, and one atomicAdd per wavefront and non-zero counter into overs[2*s], overs[2*s + 1].
//
// Level.  The levelled forms of kPcmOut / kClipOut (a third template flag; PcmLevelIo of smst_device.h) multiply every element by its stream's
// gain in front of the rule above and keep, beside the overs word, one running maximum of |v| per lane -- the bits of the float, compared as
// integers: order-independent, so bit-reproducible --, maxed over the wavefront and, where it exceeds the stored one, into peaks[s].
#pragma once
#include <cstdint>
#include <stdexcept>
#include <type_traits>

namespace smst {

typedef unsigned PcmWord4 __attribute__((vector_size(16), may_alias)); // one 16-byte access
struct PcmS24 { unsigned char b[3]; };                                   // one packed sample, little-endian
typedef _Float16 PcmF16;
constexpr unsigned kPcmOverClamped = 1u, kPcmOverNan = 1u << 16;

// Per format: a group of G elements is W 16-byte words; lead(address) = the elements in front of the first group boundary.  The way out is
// one quantiser: t = scaled(v) is the value that is rounded (v*kScale for the integer formats, v itself for the float ones; a dithered
// element is v*kScale + d instead, NaN iff v is: d is finite), encode(t) its code, over(t) what encode(t) adds to a lane's overs word,
// pack(t, w) the codes of a group.
template <typename T> struct PcmFormat;
template <typename T, int G> __device__ inline int pcmLeadAligned(uintptr_t address) { return (G - int((address/sizeof(T))%G))%G; }
template <> struct PcmFormat<int16_t> {
	static constexpr int G = 8, W = 1;
	static constexpr float kScale = 32768.0f;
	static __device__ inline int lead(uintptr_t a) { return pcmLeadAligned<int16_t, G>(a); }
	static __device__ inline float decode(int16_t v) { return float(v)*(1.0f/32768.0f); }
	static __device__ inline float scaled(float v) { return v*kScale; }
	static __device__ inline unsigned code(float t) { // the 16 bits
		const float q = fminf(fmaxf(roundf(t), -32768.0f), 32767.0f);
		return (t != t) ? 0u : (unsigned(int(q)) & 0xffffu);
	}
	static __device__ inline int16_t encode(float t) { return int16_t(uint16_t(code(t))); }
	static __device__ inline unsigned over(float t) {
		const float r = roundf(t);
		return (t != t) ? kPcmOverNan : (r > 32767.0f || r < -32768.0f) ? kPcmOverClamped : 0u;
	}
	static __device__ inline void unpack(const PcmWord4 *w, float *x) {
		for (int k = 0; k < 4; ++k) {
			x[2*k] = decode(int16_t(w[0][k] & 0xffffu));
			x[2*k + 1] = decode(int16_t(w[0][k] >> 16));
		}
	}
	static __device__ inline void pack(const float *t, PcmWord4 *w) {
		for (int k = 0; k < 4; ++k) w[0][k] = code(t[2*k]) | (code(t[2*k + 1]) << 16);
	}
};
template <> struct PcmFormat<float> {
	static constexpr int G = 4, W = 1;
	static __device__ inline int lead(uintptr_t a) { return pcmLeadAligned<float, G>(a); }
	static __device__ inline float decode(float v) { return v; }
	static __device__ inline float scaled(float v) { return v; }
	static __device__ inline float encode(float t) { return t; }
	static __device__ inline unsigned over(float t) { return (t != t) ? kPcmOverNan : 0u; }
	static __device__ inline void unpack(const PcmWord4 *w, float *x) {
		for (int k = 0; k < 4; ++k) x[k] = __int_as_float(int(w[0][k]));
	}
	static __device__ inline void pack(const float *t, PcmWord4 *w) {
		for (int k = 0; k < 4; ++k) w[0][k] = unsigned(__float_as_int(t[k]));
	}
};
template <> struct PcmFormat<int32_t> {
	static constexpr int G = 4, W = 1;
	static constexpr float kScale = 2147483648.0f;
	static __device__ inline int lead(uintptr_t a) { return pcmLeadAligned<int32_t, G>(a); }
	static __device__ inline float decode(int32_t v) { return float(v)*(1.0f/2147483648.0f); }
	static __device__ inline float scaled(float v) { return v*kScale; }
	// the clamp acts on the float (2147483520 is the largest one below 2^31): no float outside int's range is ever converted
	static __device__ inline int32_t encode(float t) {
		const float r = roundf(t);
		const int32_t q = int32_t(fminf(fmaxf(r, -2147483648.0f), 2147483520.0f));
		return (t != t) ? 0 : (r >= 2147483648.0f ? 2147483647 : q);
	}
	static __device__ inline unsigned over(float t) {
		const float r = roundf(t);
		return (t != t) ? kPcmOverNan : (r >= 2147483648.0f || r < -2147483648.0f) ? kPcmOverClamped : 0u;
	}
	static __device__ inline void unpack(const PcmWord4 *w, float *x) {
		for (int k = 0; k < 4; ++k) x[k] = decode(int32_t(w[0][k]));
	}
	static __device__ inline void pack(const float *t, PcmWord4 *w) {
		for (int k = 0; k < 4; ++k) w[0][k] = unsigned(encode(t[k]));
	}
};
template <> struct PcmFormat<PcmF16> {
	static constexpr int G = 8, W = 1;
	static __device__ inline int lead(uintptr_t a) { return pcmLeadAligned<PcmF16, G>(a); }
	static __device__ inline float fromBits(unsigned bits) { const uint16_t b = uint16_t(bits); PcmF16 h; __builtin_memcpy(&h, &b, 2); return float(h); }
	static __device__ inline unsigned toBits(float v) { const PcmF16 h = PcmF16(v); uint16_t b; __builtin_memcpy(&b, &h, 2); return b; }
	static __device__ inline float decode(PcmF16 v) { return float(v); }
	static __device__ inline float scaled(float v) { return v; }
	static __device__ inline PcmF16 encode(float t) { return PcmF16(t); }
	// 65520 is the tie between 65504 and 2^16: to even, which is +-inf
	static __device__ inline unsigned over(float t) {
		const float a = fabsf(t);
		return (t != t) ? kPcmOverNan : (a >= 65520.0f && a <= 3.402823466e38f) ? kPcmOverClamped : 0u;
	}
	static __device__ inline void unpack(const PcmWord4 *w, float *x) {
		for (int k = 0; k < 4; ++k) {
			x[2*k] = fromBits(w[0][k] & 0xffffu);
			x[2*k + 1] = fromBits(w[0][k] >> 16);
		}
	}
	static __device__ inline void pack(const float *t, PcmWord4 *w) {
		for (int k = 0; k < 4; ++k) w[0][k] = toBits(t[2*k]) | (toBits(t[2*k + 1]) << 16);
	}
};
template <> struct PcmFormat<PcmS24> {
	static constexpr int G = 16, W = 3;
	static constexpr float kScale = 8388608.0f;
	// the k < 16 with address + 3k = 0 mod 16: k = -address*11, as 3*11 = 1 mod 16
	static __device__ inline int lead(uintptr_t a) { return int(((0 - a) & 15u)*11u & 15u); }
	static __device__ inline float fromLow24(unsigned v) { return float(int(v << 8) >> 8)*(1.0f/8388608.0f); } // (bits 24..31 of v are ignored)
	static __device__ inline float decode(PcmS24 v) { return fromLow24(unsigned(v.b[0]) | (unsigned(v.b[1]) << 8) | (unsigned(v.b[2]) << 16)); }
	static __device__ inline float scaled(float v) { return v*kScale; }
	static __device__ inline unsigned code(float t) { // the 24 bits
		const float q = fminf(fmaxf(roundf(t), -8388608.0f), 8388607.0f);
		return (t != t) ? 0u : (unsigned(int(q)) & 0xffffffu);
	}
	static __device__ inline PcmS24 encode(float t) {
		const unsigned q = code(t);
		PcmS24 r;
		r.b[0] = (unsigned char)(q & 0xffu); r.b[1] = (unsigned char)((q >> 8) & 0xffu); r.b[2] = (unsigned char)(q >> 16);
		return r;
	}
	static __device__ inline unsigned over(float t) {
		const float r = roundf(t);
		return (t != t) ? kPcmOverNan : (r > 8388607.0f || r < -8388608.0f) ? kPcmOverClamped : 0u;
	}
	// four samples are three dwords: a = d0[0:23], b = d0[24:31] d1[0:15], c = d1[16:31] d2[0:7], d = d2[8:31]
	static __device__ inline void unpack(const PcmWord4 *w, float *x) {
		unsigned d[12];
		for (int k = 0; k < 12; ++k) d[k] = w[k >> 2][k & 3];
		for (int q = 0; q < 4; ++q) {
			const unsigned d0 = d[3*q], d1 = d[3*q + 1], d2 = d[3*q + 2];
			x[4*q] = fromLow24(d0);
			x[4*q + 1] = fromLow24((d0 >> 24) | (d1 << 8));
			x[4*q + 2] = fromLow24((d1 >> 16) | (d2 << 16));
			x[4*q + 3] = fromLow24(d2 >> 8);
		}
	}
	static __device__ inline void pack(const float *t, PcmWord4 *w) {
		unsigned d[12];
		for (int q = 0; q < 4; ++q) {
			const unsigned a = code(t[4*q]), b = code(t[4*q + 1]), c = code(t[4*q + 2]), e = code(t[4*q + 3]);
			d[3*q] = a | (b << 24);
			d[3*q + 1] = (b >> 8) | (c << 16);
			d[3*q + 2] = (c >> 16) | (e << 8);
		}
		for (int k = 0; k < 12; ++k) w[k >> 2][k & 3] = d[k];
	}
};

__device__ inline int pcmSlot(int e) { return e + (e >> 5); }
inline __host__ __device__ int pcmLdsWords(int C) { const int most = kPcmTileFrames*C + 16; return most + most/32 + 1; } // (tile 0 is up to G - 1 = 15 elements longer)
inline size_t pcmLdsBytes(int C) { return size_t(pcmLdsWords(C))*sizeof(float); }
inline size_t pcmDitherLdsBytes(int C) { return pcmLdsBytes(C) + 16*sizeof(unsigned); } // behind the image: key(c) of the 16 channels at the most

// Dither (include/smst.h, "Dither": the definition; PcmDither of smst_device.h: a stream's entry).  Element i of a tile is channel c of the
// run's frame f -- from the tile's first element e0, wherever in a frame that lies --, and frame f of the run has the index n = first + f:
// the dither of an element is a function of (h, c, n) alone, whichever of the three paths below stores it and whichever tile, call or
// launch it falls into.  key(c) = pcmMix(h + 0x9E3779B9*(c + 1)) is computed once per workgroup, into LDS behind the tile image;
// per element there remain mix(key ^ lo32(n)) -- shared by the two words of the white form -- and one mix per word.
__device__ inline float pcmDitherUnit(unsigned word) { return float(word >> 8)*(1.0f/16777216.0f) - 0.5f; } // [-0.5, 0.5), exact
__device__ inline float pcmDitherValue(unsigned mode, unsigned key, unsigned long long n) {
	const unsigned hi = unsigned(n >> 32), a = pcmMix(key ^ unsigned(n)), step = 0x85EBCA6Bu*(2u*hi + 1u);
	const float u0 = pcmDitherUnit(pcmMix(a + step));
	if (mode == kPcmDitherTpdf) return u0 + pcmDitherUnit(pcmMix(a + step + 0x85EBCA6Bu));
	const unsigned long long m = n - 1; // (modulo 2^64)
	return u0 - pcmDitherUnit(pcmMix(pcmMix(key ^ unsigned(m)) + 0x85EBCA6Bu*(2u*unsigned(m >> 32) + 1u)));
}
// Where element i of a tile lies: frame `frame` behind the tile's first frame, channel c.  next(): the element behind it.
struct PcmPlace {
	unsigned frame, c;
	__device__ inline PcmPlace(int lag, int i, int C) : frame(unsigned(lag + i)/unsigned(C)), c(unsigned(lag + i) - frame*unsigned(C)) {}
	__device__ inline void next(int C) { if (++c == unsigned(C)) { c = 0; ++frame; } }
};

// The elements [e0, e0 + count) of a stream's run of `total` elements that tile `t` moves, and how many of them (tile 0 only) lie in
// front of the first group boundary.  false: the tile lies behind the run.
template <typename T> __device__ inline bool pcmTileRun(const T *run, long long total, bool dense, int t, int C, long long &e0, int &count, int &head) {
	const int tileElems = kPcmTileFrames*C; // whole groups: a multiple of 16 elements
	const int lead = dense ? PcmFormat<T>::lead(reinterpret_cast<uintptr_t>(run)) : 0;
	e0 = t ? (long long)t*tileElems + lead : 0;
	if (e0 >= total) return false;
	const long long e1 = (long long)(t + 1)*tileElems + lead;
	count = int((e1 < total ? e1 : total) - e0);
	head = t ? 0 : (lead < count ? lead : count);
	return true;
}

// The walk over those elements, in either direction (T may be const): with frameStride == C the `head` elements one by one, the whole groups
// of G, the elements behind the last group one by one; else every element by itself.  element(x, i, at): x is element i of the tile, at its
// PcmPlace; group(p, i, at): p points at the W aligned 16-byte words of the G elements from i on.  Every lane of the workgroup calls it.
template <typename T, typename Element, typename Group> __device__ inline void pcmWalk(T *run, long long frameStride, long long e0, int count, int head, int C, Element element, Group group) {
	constexpr int G = PcmFormat<typename std::remove_const<T>::type>::G;
	const int tid = threadIdx.x;
	const long long f0 = e0/C; // (a tile may begin and end inside a frame)
	const int lag = int(e0 - f0*C); // elements of the tile's first frame that lie in front of the tile
	if (frameStride == C) {
		T *p = run + e0;
		if (tid < head) element(p[tid], tid, PcmPlace(lag, tid, C));
		const int nGroups = (count - head)/G;
		for (int g = tid; g < nGroups; g += 256) {
			const int e = head + g*G;
			group(p + e, e, PcmPlace(lag, e, C));
		}
		const int done = head + nGroups*G;
		if (tid < count - done) element(p[done + tid], done + tid, PcmPlace(lag, done + tid, C));
	} else {
		for (int i = tid; i < count; i += 256) {
			const PcmPlace at(lag, i, C);
			element(run[(f0 + at.frame)*frameStride + at.c], i, at);
		}
	}
}

// One tile of a run of frames -> the rows of a planar fp32 image.  run: the run's first frame; dst: the sample of channel 0 that frame goes to.
// Every lane of the workgroup calls it (kPcmIn; kClipIn of smst_clip.h for a run that begins at a per-stream offset).
template <typename T> __device__ inline void pcmTileIn(const T *__restrict__ run, long long inFrameStride, long long frames, float *__restrict__ out, long long outChannelStride,
		int t, int C, float *tile) {
	typedef PcmFormat<T> F;
	const int tid = threadIdx.x;
	long long e0;
	int count, head;
	if (!pcmTileRun<T>(run, frames*C, inFrameStride == C, t, C, e0, count, head)) return;
	pcmWalk(run, inFrameStride, e0, count, head, C,
		[&](const T &x, int i, const PcmPlace &) { tile[pcmSlot(i)] = F::decode(x); },
		[&](const T *p, int i, const PcmPlace &) {
			PcmWord4 w[F::W];
			for (int k = 0; k < F::W; ++k) w[k] = reinterpret_cast<const PcmWord4 *>(p)[k];
			float x[F::G];
			F::unpack(w, x);
			for (int k = 0; k < F::G; ++k) tile[pcmSlot(i + k)] = x[k];
		});
	__syncthreads();
	const long long f0 = e0/C; // (each element is moved by the tile that holds it)
	const int nFrames = int((e0 + count - 1)/C - f0) + 1;
	float *dst = out + f0;
	for (int c = 0; c < C; ++c) {
		const int first = int(f0*C + c - e0);
		for (int fl = tid; fl < nFrames; fl += 256) {
			const int i = first + fl*C;
			if (i >= 0 && i < count) dst[(size_t)c*outChannelStride + fl] = tile[pcmSlot(i)];
		}
	}
}

// What an element adds to a peak meter: the bits of |v| -- non-negative floats order as their bit patterns do, +inf above every finite one --,
// 0 for a NaN
__device__ inline unsigned pcmPeakBits(float v) {
	const unsigned a = unsigned(__float_as_int(v)) & 0x7fffffffu;
	return a > 0x7f800000u ? 0u : a;
}
// the lanes' peaks into stream s's word (every lane of the workgroup arrives here): one vote, and a wavefront that holds nothing above the
// stored peak -- nearly every one, once a loud tile has been met -- issues no atomic at all, another one a single atomicMax
__device__ inline void pcmMaxPeak(int *__restrict__ peaks, int s, unsigned peak) {
	if (__any(int(peak) > peaks[s])) {
		const int tid = threadIdx.x;
		int most = int(peak);
		for (int m = 32; m; m >>= 1) most = max(most, __shfl(most, (tid & 63) ^ m));
		if ((tid & 63) == 0) atomicMax(peaks + s, most);
	}
}

// The reverse: one tile of the rows of a planar fp32 image -> a run of frames.  in: the sample of channel 0 that goes to the run's first frame,
// or null for a run of zeros (the code of 0.0).  false: the tile lies behind the run; else `over` has this lane's overs word (see "Overs").
// Dith (int16 / int24) decides how an element's rounded value is formed -- v*scale + d, d the dither of the stream's entry dp for the frame
// index first + f (a run of zeros and a stream of mode 0 get d = 0: the undithered codes), so that an element counts as clamped when the
// DITHERED value was -- and that the 16 key words behind the image are filled; nothing else.
// Level ("Level" of include/smst.h): the quantiser takes w = v*g -- one fp32 multiply of its own -- in place of v, and `peak` has the largest
// |v| of this lane's elements as its bits, NaN skipped; a run of zeros is not multiplied (0*inf would be a NaN).  Nothing else.
// Limit ("Limiter" of include/smst.h; the levelled form only): where `limit` is set -- r of the run's first frame, one float per frame --
// the quantiser takes u = w*r, one more fp32 multiply of its own; a stream whose `limit` is null gets the levelled form's bytes.
// Delayed ("Stream limiter" of include/smst.h; the limited form only): where `line` is set -- the last lineFrames of the stream's carried
// frames, rows of linePitch floats, one per channel -- frame i of the run is frame i of the line for i < lineFrames and frame i - lineFrames
// of the image behind it: the loader of the delayed stream, and nothing else; a stream whose `line` is null is loaded as ever.
template <typename T, bool Dith, bool Level = false, bool Limit = false, bool Delayed = false> __device__ inline bool pcmTileOut(const float *__restrict__ in, long long inChannelStride, T *__restrict__ run, long long outFrameStride, long long frames,
		int t, int C, float *tile, unsigned &over, PcmDither dp, float gain = 1.0f, unsigned *peak = nullptr, const float *__restrict__ limit = nullptr,
		const float *__restrict__ line = nullptr, int lineFrames = 0, int linePitch = 0) {
	typedef PcmFormat<T> F;
	const int tid = threadIdx.x;
	long long e0;
	int count, head;
	if (!pcmTileRun<T>(run, frames*C, outFrameStride == C, t, C, e0, count, head)) return false;
	const long long f0 = e0/C;
	const int nFrames = int((e0 + count - 1)/C - f0) + 1;
	const float *src = in ? in + f0 : nullptr;
	for (int c = 0; c < C; ++c) {
		const int first = int(f0*C + c - e0);
		for (int fl = tid; fl < nFrames; fl += 256) {
			const int i = first + fl*C;
			if (i < 0 || i >= count) continue;
			if constexpr (Delayed) if (line) {
				const long long f = f0 + fl;
				tile[pcmSlot(i)] = f < lineFrames ? line[(size_t)c*linePitch + f] : in[(size_t)c*inChannelStride + (f - lineFrames)];
				continue;
			}
			tile[pcmSlot(i)] = src ? src[(size_t)c*inChannelStride + fl] : 0.0f;
		}
	}
	const unsigned mode = Dith && src ? dp.mode : 0u;
	unsigned *keys = reinterpret_cast<unsigned *>(tile) + pcmLdsWords(C);
	if (mode && tid < C) keys[tid] = pcmMix(dp.h + 0x9E3779B9u*unsigned(tid + 1));
	__syncthreads();
	over = 0;
	const unsigned long long n0 = (((unsigned long long)dp.nHi << 32) | dp.nLo) + (unsigned long long)f0;
	const float g = src ? gain : 1.0f;
	unsigned most = 0u;
	auto rounded = [&](int i, const PcmPlace &at) { // element i of the tile as the quantiser takes it
		float v = tile[pcmSlot(i)];
		if constexpr (Level) {
			most = max(most, pcmPeakBits(v));
			v = __fmul_rn(v, g);
#if defined(__HIP_DEVICE_COMPILE__)
			// float16 writes the fp32 product narrowed: two roundings.  Left alone, the compiler folds the multiply into the conversion
			// (v_fma_mixlo_f16, which rounds the exact product once); an empty statement that "reads and writes" w keeps it a value of its own
			if constexpr (std::is_same<T, PcmF16>::value) asm("" : "+v"(v));
#endif
			if constexpr (Limit) if (limit && src) {
				v = __fmul_rn(v, limit[f0 + at.frame]);
#if defined(__HIP_DEVICE_COMPILE__)
				if constexpr (std::is_same<T, PcmF16>::value) asm("" : "+v"(v));
#endif
			}
		}
		if constexpr (Dith) return mode ? v*F::kScale + pcmDitherValue(mode, keys[at.c], n0 + at.frame) : v*F::kScale;
		else return F::scaled(v);
	};
	pcmWalk(run, outFrameStride, e0, count, head, C,
		[&](T &x, int i, const PcmPlace &at) { const float q = rounded(i, at); x = F::encode(q); over += F::over(q); },
		[&](T *p, int i, PcmPlace at) {
			float x[F::G];
			for (int k = 0; k < F::G; ++k) { x[k] = rounded(i + k, at); over += F::over(x[k]); at.next(C); }
			PcmWord4 w[F::W];
			F::pack(x, w);
			for (int k = 0; k < F::W; ++k) reinterpret_cast<PcmWord4 *>(p)[k] = w[k];
		});
	if constexpr (Level) *peak = most;
	return true;
}
// the lanes' overs words into stream s's counters (every lane of the workgroup arrives here; the vote keeps the clean wavefront, which is
// nearly every one, to one instruction)
__device__ inline void pcmAddOvers(unsigned *__restrict__ overs, int s, unsigned over) {
	if (overs && __any(over != 0)) {
		const int tid = threadIdx.x;
		int sum = int(over);
		for (int m = 32; m; m >>= 1) sum += __shfl(sum, (tid & 63) ^ m);
		if ((tid & 63) == 0) {
			int *words = reinterpret_cast<int *>(overs) + 2*s; // (the words wrap as unsigned ones do)
			if (sum & 0xffff) atomicAdd(words, sum & 0xffff);
			if (sum >> 16) atomicAdd(words + 1, sum >> 16);
		}
	}
}

// interleaved frames -> planar fp32.  grid (tiles, S), 256 threads; in[s*inStreamStride + i*inFrameStride + c] -> out[s*outStreamStride + c*outChannelStride + i], i < counts[s]
template <typename T> __global__ __launch_bounds__(256) void kPcmIn(const T *__restrict__ in, long long inStreamStride, long long inFrameStride,
		float *__restrict__ out, long long outStreamStride, long long outChannelStride, const int *__restrict__ counts, int C) {
	extern __shared__ __attribute__((aligned(16))) unsigned char smemRaw[];
	const int s = blockIdx.y;
	pcmTileIn<T>(in + (size_t)s*inStreamStride, inFrameStride, counts[s], out + (size_t)s*outStreamStride, outChannelStride, blockIdx.x, C, reinterpret_cast<float *>(smemRaw));
}

// planar fp32 -> interleaved frames: the reverse.  overs (may be null): [S][2] counters, see "Overs" above.  Dith (int16 / int24): dither[s] is
// stream s's entry, the index of the run's first frame in it; else dither is not read.  Level: the stream's fixed gain of level.table[s] (the
// host refuses a whole-clip mode here) is applied and reported -- by the workgroup of the run's first tile --, its peak metered; else level is not read
template <typename T, bool Dith, bool Level> __global__ __launch_bounds__(256) void kPcmOut(const float *__restrict__ in, long long inStreamStride, long long inChannelStride,
		T *__restrict__ out, long long outStreamStride, long long outFrameStride, const int *__restrict__ counts, int C, unsigned *__restrict__ overs, const PcmDither *__restrict__ dither,
		PcmLevelIo level) {
	extern __shared__ __attribute__((aligned(16))) unsigned char smemRaw[];
	const int s = blockIdx.y;
	PcmDither dp{0u, 0u, 0u, 0u};
	if constexpr (Dith) dp = dither[s];
	unsigned over;
	if constexpr (Level) {
		const float g = level.table[s].gain;
		unsigned peak;
		if (!pcmTileOut<T, Dith, true>(in + (size_t)s*inStreamStride, inChannelStride, out + (size_t)s*outStreamStride, outFrameStride, counts[s], blockIdx.x, C, reinterpret_cast<float *>(smemRaw), over, dp, g, &peak)) return;
		if (blockIdx.x == 0 && threadIdx.x == 0) level.applied[s] = g;
		pcmMaxPeak(level.peaks, s, peak);
	} else {
		if (!pcmTileOut<T, Dith>(in + (size_t)s*inStreamStride, inChannelStride, out + (size_t)s*outStreamStride, outFrameStride, counts[s], blockIdx.x, C, reinterpret_cast<float *>(smemRaw), over, dp)) return;
	}
	pcmAddOvers(overs, s, over);
}

// A runtime format (SMST_PCM_* of include/smst.h; the C ABI has checked it) -> its element type: f(PcmTag<T>(), dithered), `dithered` a
// std::true_type where the caller has dither entries AND the format has a step to dither (int16 / int24), else a std::false_type
template <typename T> struct PcmTag { typedef T type; };
template <typename T, typename F> static void pcmDispatchDithered(bool dither, F &f) {
	if (dither) f(PcmTag<T>(), std::true_type());
	else f(PcmTag<T>(), std::false_type());
}
template <typename F> static void pcmDispatch(int format, bool dither, F f) {
	switch (format) {
	case kPcmS16: pcmDispatchDithered<int16_t>(dither, f); break;
	case kPcmS24: pcmDispatchDithered<PcmS24>(dither, f); break;
	case kPcmF32: f(PcmTag<float>(), std::false_type()); break;
	case kPcmS32: f(PcmTag<int32_t>(), std::false_type()); break;
	case kPcmF16: f(PcmTag<PcmF16>(), std::false_type()); break;
	default: throw std::invalid_argument("unknown PCM format");
	}
}

// maxFrames: the largest of the streams' counts
void launchPcmIn(int format, const void *in, long long inStreamStride, long long inFrameStride, float *out, long long outStreamStride, long long outChannelStride,
                 const int *counts, int S, int C, int maxFrames, hipStream_t st) {
	if (maxFrames < 1) return;
	const dim3 grid(divUp(maxFrames, kPcmTileFrames), S);
	pcmDispatch(format, false, [&](auto tag, auto) {
		typedef typename decltype(tag)::type T;
		hipLaunchKernelGGL(kPcmIn<T>, grid, dim3(256), pcmLdsBytes(C), st, static_cast<const T *>(in), inStreamStride, inFrameStride, out, outStreamStride, outChannelStride, counts, C);
	});
	countLaunch(LK_PCM_IN);
}
void launchPcmOut(int format, const float *in, long long inStreamStride, long long inChannelStride, void *out, long long outStreamStride, long long outFrameStride,
                  const int *counts, int S, int C, int maxFrames, unsigned *overs, hipStream_t st, const PcmDither *dither, const PcmLevelIo &level) {
	if (maxFrames < 1) return;
	const dim3 grid(divUp(maxFrames, kPcmTileFrames), S);
	pcmDispatch(format, dither != nullptr, [&](auto tag, auto dithered) {
		typedef typename decltype(tag)::type T;
		constexpr bool Dith = decltype(dithered)::value;
		const size_t lds = Dith ? pcmDitherLdsBytes(C) : pcmLdsBytes(C);
		if (level.table) {
			hipLaunchKernelGGL((kPcmOut<T, Dith, true>), grid, dim3(256), lds, st, in, inStreamStride, inChannelStride, static_cast<T *>(out), outStreamStride, outFrameStride, counts, C, overs, dither, level);
			countLaunch(LK_PCM_OUT_LEVELLED);
		} else {
			hipLaunchKernelGGL((kPcmOut<T, Dith, false>), grid, dim3(256), lds, st, in, inStreamStride, inChannelStride, static_cast<T *>(out), outStreamStride, outFrameStride, counts, C, overs, dither, level);
			countLaunch(Dith ? LK_PCM_OUT_DITHERED : LK_PCM_OUT);
		}
	});
}

} // namespace smst
