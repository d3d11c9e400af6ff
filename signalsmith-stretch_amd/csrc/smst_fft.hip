// Analysis and synthesis transforms, overlap-add and emission (K1, K4a, K4b, K5) and their launchers.  See smst_kernels_common.h.
#include "smst_kernels_common.h"
#include <type_traits>

namespace smst {

// ------------------------------------------------------------------------------------------------------
// In-LDS Stockham FFT (decimation in frequency, natural order in and out), H = 2^k * {1,3,5}.
// Radix-4 passes (+ one radix-2) come first so the stride `s` stays a power of two; the single odd-radix
// pass comes last, where all its twiddles are 1.  src/dst ping-pong; returns the buffer holding the result.
// SIGN = -1: forward (e^{-i...}), +1: inverse (unnormalised).
// ------------------------------------------------------------------------------------------------------
// Complex values are fc (smst_fft_complex.h): a register pair from load to store; conjugation, +-i and negation of an operand are folded into
// the instruction that uses it.  The stage twiddles are stored for the forward transform: the inverse one conjugates them in the product.
template <int SIGN> __device__ __forceinline__ fc mulTwiddle(fc v, fc w) { return fmul<(SIGN > 0)>(v, w); } // v * w (forward), v * conj(w) (inverse)
template <int SIGN> __device__ __forceinline__ fc addJ(fc a, fc b) { return (SIGN < 0) ? fsubI(a, b) : faddI(a, b); } // a + j b, j = -i (forward), +i (inverse)
template <int SIGN> __device__ __forceinline__ fc subJ(fc a, fc b) { return (SIGN < 0) ? faddI(a, b) : fsubI(a, b); } // a - j b
template <int SIGN> __device__ __forceinline__ fc mulJ(fc a) { return (SIGN < 0) ? fmake(a.y, -a.x) : fmake(-a.y, a.x); } // j a (where no sum takes it)

// the radix-4, -3 and -5 butterflies, in place, outputs in natural order (the generic ladder's and the register-blocked stages')
template <int SIGN>
__device__ __forceinline__ void dft4(fc &a, fc &b, fc &c, fc &d) {
	const fc apc = fadd(a, c), amc = fsub(a, c), bpd = fadd(b, d), bmd = fsub(b, d);
	a = fadd(apc, bpd);
	b = addJ<SIGN>(amc, bmd);
	c = fsub(apc, bpd);
	d = subJ<SIGN>(amc, bmd);
}
// the same with j*c in the place of c (the w16^4 and w8^2 twiddles of the radix-16 and radix-8 butterflies: no instruction of their own)
template <int SIGN>
__device__ __forceinline__ void dft4J(fc &a, fc &b, fc &c, fc &d) {
	const fc apc = addJ<SIGN>(a, c), amc = subJ<SIGN>(a, c), bpd = fadd(b, d), bmd = fsub(b, d);
	a = fadd(apc, bpd);
	b = addJ<SIGN>(amc, bmd);
	c = fsub(apc, bpd);
	d = subJ<SIGN>(amc, bmd);
}
template <int SIGN>
__device__ __forceinline__ void dft3(fc &a, fc &b, fc &c) {
	const float s3 = 0.86602540378443864676f;
	const fc bpc = fadd(b, c), bmc = fsub(b, c);
	const fc t = fmake(a.x - 0.5f*bpc.x, a.y - 0.5f*bpc.y);
	const fc jb = mulJ<SIGN>(bmc);
	const fc u = fmake(jb.x*s3, jb.y*s3);
	a = fadd(a, bpc);
	b = fadd(t, u);
	c = fsub(t, u);
}
template <int SIGN>
__device__ __forceinline__ void dft5(fc &a, fc &b, fc &c, fc &d, fc &e) {
	const float c1 = 0.30901699437494742410f, c2 = -0.80901699437494742410f;
	const float s1 = 0.95105651629515357212f, s2 = 0.58778525229247312917f;
	const fc bpe = fadd(b, e), bme = fsub(b, e), cpd = fadd(c, d), cmd = fsub(c, d);
	const fc t1 = fmake(a.x + c1*bpe.x + c2*cpd.x, a.y + c1*bpe.y + c2*cpd.y);
	const fc t2 = fmake(a.x + c2*bpe.x + c1*cpd.x, a.y + c2*bpe.y + c1*cpd.y);
	const fc u1 = fmake(s1*bme.x + s2*cmd.x, s1*bme.y + s2*cmd.y);
	const fc u2 = fmake(s2*bme.x - s1*cmd.x, s2*bme.y - s1*cmd.y);
	a = fadd(a, fadd(bpe, cpd));
	b = addJ<SIGN>(t1, u1);
	c = addJ<SIGN>(t2, u2);
	d = subJ<SIGN>(t2, u2);
	e = subJ<SIGN>(t1, u1);
}
template <int SIGN>
__device__ float2 *fftLds(float2 *src2, float2 *dst2, const FftPlan &plan, const float2 *__restrict__ tw2) {
	fc *src = reinterpret_cast<fc *>(src2), *dst = reinterpret_cast<fc *>(dst2);
	const fc *__restrict__ tw = reinterpret_cast<const fc *>(tw2);
	const int H = plan.H;
	int nCur = H;
	int shift = 0; // s = 1 << shift while radices are powers of two
	for (int pass = 0; pass < plan.npass; ++pass) {
		const int r = plan.radix[pass];
		const int m = nCur/r;
		const int nb = H/r;
		const int twScale = H/nCur;
		if (r == 4) {
			const int s = 1 << shift;
			for (int t = threadIdx.x; t < nb; t += blockDim.x) {
				const int p = t >> shift, q0 = t & (s - 1);
				const fc *in = src + q0 + (p << shift);
				const int inStride = m << shift;
				fc *out = dst + q0 + ((4*p) << shift);
				fc a = in[0], b = in[inStride], c = in[2*inStride], e = in[3*inStride];
				dft4<SIGN>(a, b, c, e);
				const int ti = p*twScale;
				out[0] = a;
				out[s] = mulTwiddle<SIGN>(b, tw[ti]);
				out[2*s] = mulTwiddle<SIGN>(c, tw[2*ti]);
				out[3*s] = mulTwiddle<SIGN>(e, tw[3*ti]);
			}
			shift += 2;
		} else if (r == 2) {
			const int s = 1 << shift;
			for (int t = threadIdx.x; t < nb; t += blockDim.x) {
				const int p = t >> shift, q0 = t & (s - 1);
				const fc *in = src + q0 + (p << shift);
				const int inStride = m << shift;
				fc *out = dst + q0 + ((2*p) << shift);
				const fc a = in[0], b = in[inStride];
				out[0] = fadd(a, b);
				out[s] = mulTwiddle<SIGN>(fsub(a, b), tw[p*twScale]);
			}
			shift += 1;
		} else if (r == 3) { // last pass: m == 1, p == 0, all twiddles are 1
			const int s = nb;
			for (int t = threadIdx.x; t < nb; t += blockDim.x) {
				fc a = src[t], b = src[t + s], c = src[t + 2*s];
				dft3<SIGN>(a, b, c);
				dst[t] = a;
				dst[t + s] = b;
				dst[t + 2*s] = c;
			}
		} else { // r == 5, last pass
			const int s = nb;
			for (int t = threadIdx.x; t < nb; t += blockDim.x) {
				fc a = src[t], b = src[t + s], c = src[t + 2*s], e = src[t + 3*s], f = src[t + 4*s];
				dft5<SIGN>(a, b, c, e, f);
				dst[t] = a;
				dst[t + s] = b;
				dst[t + 2*s] = c;
				dst[t + 3*s] = e;
				dst[t + 4*s] = f;
			}
		}
		__syncthreads();
		fc *tmp = src; src = dst; dst = tmp;
		nCur = m;
	}
	return reinterpret_cast<float2 *>(src);
}

// ------------------------------------------------------------------------------------------------------
// Register-blocked FFT for H = 256*R3: three Stockham stages 16 x 16 x R3, each butterfly held in registers, so the data
// (R3 = 10: 2560 bins = presetCheaper at 44.1/48 kHz; 12: 3072 = presetDefault at 44.1/48 kHz; 20: 5120 = presetCheaper at 88.2/96 kHz;
// 24: 6144 = presetDefault at 88.2/96 kHz -- every size signalsmith-stretch.h:63-68 produces up to 96 kHz; R3 = {2,4,8} x {3,5})
// crosses LDS only twice (vs. six times in the generic radix-4 ladder) and the stage-A output is padded by one
// element per 16 so that neither the 128-byte-strided writes nor the stage-B reads conflict on LDS banks.
// Twiddles come from per-stage tables laid out [n][p] (coalesced across the threads of a stage).
// ------------------------------------------------------------------------------------------------------
template <int SIGN>
__device__ __forceinline__ fc mulConst(fc v, float re, float im) { // v * (re, SIGN<0 ? -im : +im)
	const float s = (SIGN < 0) ? -im : im;
	return fmake(v.x*re - v.y*s, v.x*s + v.y*re);
}
// 16-point DFT in place; on return X[e + 4c] sits at v[c + 4e]
template <int SIGN>
__device__ __forceinline__ void dft16(fc (&v)[16]) {
#pragma unroll
	for (int i = 0; i < 4; ++i) dft4<SIGN>(v[i], v[i + 4], v[i + 8], v[i + 12]);
	const float c1 = 0.92387953251128675613f, s1 = 0.38268343236508977173f, h = 0.70710678118654752440f;
	// t_i[e] (at v[i + 4e]) *= w16^(i e)
	v[1 + 4] = mulConst<SIGN>(v[1 + 4], c1, s1);   // w^1
	v[1 + 8] = mulConst<SIGN>(v[1 + 8], h, h);     // w^2
	v[1 + 12] = mulConst<SIGN>(v[1 + 12], s1, c1); // w^3
	v[2 + 4] = mulConst<SIGN>(v[2 + 4], h, h);     // w^2
	// v[2 + 8] *= w^4 = j: taken by the butterfly that reads it (dft4J)
	v[2 + 12] = mulConst<SIGN>(v[2 + 12], -h, h);  // w^6
	v[3 + 4] = mulConst<SIGN>(v[3 + 4], s1, c1);   // w^3
	v[3 + 8] = mulConst<SIGN>(v[3 + 8], -h, h);    // w^6
	v[3 + 12] = mulConst<SIGN>(v[3 + 12], -c1, -s1); // w^9
#pragma unroll
	for (int e = 0; e < 4; ++e) {
		if (e == 2) dft4J<SIGN>(v[4*e], v[4*e + 1], v[4*e + 2], v[4*e + 3]);
		else dft4<SIGN>(v[4*e], v[4*e + 1], v[4*e + 2], v[4*e + 3]);
	}
}
// RA-point DFT over v[base + stride*j], j < RA (RA = 2, 4 or 8), in place, outputs in natural order
template <int SIGN, int RA, int N>
__device__ __forceinline__ void dftPow2(fc (&v)[N], int base, int stride) {
	if constexpr (RA == 2) {
		const fc a = v[base], b = v[base + stride];
		v[base] = fadd(a, b);
		v[base + stride] = fsub(a, b);
	} else if constexpr (RA == 4) {
		dft4<SIGN>(v[base], v[base + stride], v[base + 2*stride], v[base + 3*stride]);
	} else {
		static_assert(RA == 8, "radix 2, 4 or 8");
		// even / odd halves (each a natural-order 4-point DFT), then X[k] = E[k] + w8^k O[k], X[k+4] = E[k] - w8^k O[k]
		fc e0 = v[base], e1 = v[base + 2*stride], e2 = v[base + 4*stride], e3 = v[base + 6*stride];
		fc o0 = v[base + stride], o1 = v[base + 3*stride], o2 = v[base + 5*stride], o3 = v[base + 7*stride];
		dft4<SIGN>(e0, e1, e2, e3);
		dft4<SIGN>(o0, o1, o2, o3);
		const float h = 0.70710678118654752440f;
		o1 = mulConst<SIGN>(o1, h, h);
		o3 = mulConst<SIGN>(o3, -h, h);
		v[base] = fadd(e0, o0); v[base + 4*stride] = fsub(e0, o0);
		v[base + stride] = fadd(e1, o1); v[base + 5*stride] = fsub(e1, o1);
		v[base + 2*stride] = addJ<SIGN>(e2, o2); v[base + 6*stride] = subJ<SIGN>(e2, o2); // w8^2 = j
		v[base + 3*stride] = fadd(e3, o3); v[base + 7*stride] = fsub(e3, o3);
	}
}
// R3-point DFT (R3 = RA*G: RA = 2, 4 or 8 and G = 3 or 5) in place; on return X[e + RA*c] sits at v[c + G*e]
template <int R3> struct LastStage {
	static constexpr int G = (R3%3 == 0) ? 3 : 5;
	static constexpr int RA = R3/G;
	static_assert(R3%G == 0 && (RA == 2 || RA == 4 || RA == 8), "last stage: {2,4,8} x {3,5} points");
};
template <int SIGN, int R3>
__device__ __forceinline__ void dftLast(fc (&v)[R3]) {
	constexpr int G = LastStage<R3>::G, RA = LastStage<R3>::RA;
#pragma unroll
	for (int i = 0; i < G; ++i) dftPow2<SIGN, RA>(v, i, G);
	// t_i[e] (at v[i + G e]) *= w_R3^(i e)
#pragma unroll
	for (int i = 1; i < G; ++i) {
#pragma unroll
		for (int e = 1; e < RA; ++e) {
			// compile-time constant after unrolling
			const float ang = 6.28318530717958647692f*float(i*e)/float(R3);
			v[i + G*e] = mulConst<SIGN>(v[i + G*e], __builtin_cosf(ang), __builtin_sinf(ang));
		}
	}
#pragma unroll
	for (int e = 0; e < RA; ++e) {
		if constexpr (G == 3) dft3<SIGN>(v[G*e], v[G*e + 1], v[G*e + 2]);
		else dft5<SIGN>(v[G*e], v[G*e + 1], v[G*e + 2], v[G*e + 3 < R3 ? G*e + 3 : 0], v[G*e + 4 < R3 ? G*e + 4 : 0]);
	}
}

// load(idx) -> fc supplies the natural-order input, store(idx, value) receives the natural-order output (an fc).
// lds: H + H/16 float2.  All threads of the block must call this (it synchronises).
// prep(idx) -> any value: called for ALL outputs of a thread before the first store(idx, value, prepared), so whatever it
// loads is in flight together (a load placed inside `store` is not moved above the preceding stores by the compiler).
// LEAN: fewer table bytes per frame (the tables are L2-resident, but 73 KB of them per frame crossed the CU's 64-B/clk vector
// memory path beside 48 KB of data -- ablation in EXPERIMENTS.md: tables held constant took 0.9 ms per step off the analysis and 0.4 off
// the synthesis).  The 15 stage-A twiddles w^n come from six loaded ones (w^1..w^4, w^8, w^12: three 16-byte loads instead of
// eight) and nine products of two of them: one extra rounding each.
struct BlockSync { __device__ __forceinline__ void operator()() const { __syncthreads(); } };
struct NoHook { __device__ __forceinline__ void operator()() const {} };
struct NoArrival { __device__ __forceinline__ fc operator()(fc v, int) const { return v; } };
// t / sync: a workgroup may hold several TEAMS of 256 threads, each transforming its own frame in its own `lds` at its own pace;
// t is then the index within the team and sync() the team's barrier.  Hooks of kSynthEmitTeams: lastRead() is called once the last
// stage's operands have left `lds` (a barrier there lets `store` write into the same buffer); requested() once the frame's loads have
// been issued and before anything is written to `lds` (the previous frame's overlap-add runs under the loads' latency), firstWritten()
// after the first stage's writes
// FRAMES = 2 (kAnalyseTeamPairs): two frames in lockstep -- every stage runs for both between the same two barriers, frame f in its own buffer
// lds + f*(H + H/16), and every table value is read once and used for both.  The arithmetic of one frame is that of FRAMES = 1, the same helpers
// in the same order; the two frames' butterflies are independent chains.  load(idx, k) then returns a FrameSet<2> (both frames' element idx),
// arrived takes (value, idx, k, frame), prep and store take the frame as a last argument.
// TwRegs = StageTwiddles: the first-stage twiddles of thread t in registers (loaded once by the caller: they depend on t alone); twA is then unused.
template <int FRAMES> struct FrameSet { fc f[FRAMES]; };
struct StageTwiddles { float4 w[8]; }; // twA4[i*MA + t], i < 8
struct TwiddlesFromTable {};
template <int SIGN, int R3, bool LEAN, int ROUNDS = 0, int FRAMES = 1, typename Load, typename Prep, typename Store, typename Sync = BlockSync, typename LastRead = NoHook,
          typename Requested = NoHook, typename FirstWritten = NoHook, typename Arrived = NoArrival, typename TwRegs = TwiddlesFromTable>
__device__ __forceinline__ void fftFast(float2 *lds2, const float4 *__restrict__ twA, const float4 *__restrict__ twB, Load load, Prep prep, Store store,
                                        const int t = threadIdx.x, Sync sync = Sync(), LastRead lastRead = LastRead(), Requested requested = Requested(),
                                        FirstWritten firstWritten = FirstWritten(), Arrived arrived = Arrived(), TwRegs twRegs = TwRegs()) {
	static_assert(FRAMES == 1 || FRAMES == 2, "one frame, or two in lockstep");
	constexpr int MA = 16*R3, BUF = 17*MA; // BUF: a frame's padded buffer, H + H/16
	constexpr bool TW_REGS = std::is_same<TwRegs, StageTwiddles>::value;
	static_assert(!(TW_REGS && LEAN), "the lean tables have no register form");
	fc *lds = reinterpret_cast<fc *>(lds2);
	auto prepOf = [&](int j, int idx, int f) { if constexpr (FRAMES == 1) return prep(j, idx); else return prep(j, idx, f); };
	auto storeOf = [&](int j, fc u, auto r, int idx, int f) { if constexpr (FRAMES == 1) store(j, u, r, idx); else store(j, u, r, idx, f); };
	fc v[FRAMES][16];
	// stage A: radix 16, stride 1
	if (t < MA) {
#pragma unroll
		for (int k = 0; k < 16; ++k) {
			if constexpr (FRAMES == 1) v[0][k] = load(t + MA*k, k);
			else {
				const FrameSet<FRAMES> both = load(t + MA*k, k);
#pragma unroll
				for (int f = 0; f < FRAMES; ++f) v[f][k] = both.f[f];
			}
		}
	}
	requested();
	if (t < MA) {
#pragma unroll
		for (int f = 0; f < FRAMES; ++f) {
#pragma unroll
			for (int k = 0; k < 16; ++k) { // (anything `load` did to its value would be waited for in front of requested())
				if constexpr (FRAMES == 1) v[f][k] = arrived(v[f][k], t + MA*k);
				else v[f][k] = arrived(v[f][k], t + MA*k, k, f);
			}
		}
		fc w[16]; // w[n] = w_H^(n t) (the inverse transform conjugates it in the product: mulTwiddle)
		if constexpr (LEAN) {
			const float4 a = twA[t], b = twA[MA + t], c = twA[2*MA + t]; // (w1, w2) (w3, w4) (w8, w12)
			w[1] = fmake(a.x, a.y); w[2] = fmake(a.z, a.w); w[3] = fmake(b.x, b.y); w[4] = fmake(b.z, b.w);
			w[8] = fmake(c.x, c.y); w[12] = fmake(c.z, c.w);
#pragma unroll
			for (int hi = 4; hi <= 12; hi += 4) {
#pragma unroll
				for (int lo = 1; lo < 4; ++lo) w[hi + lo] = fmul<false>(w[hi], w[lo]); // (conj(a)*conj(b) = conj(a*b) bit for bit: smst_fft_complex.h)
			}
		} else {
			float4 wA[8]; // the 15 stage twiddles, two per 16-byte load, in flight during the butterflies
#pragma unroll
			for (int i = 0; i < 8; ++i) {
				if constexpr (TW_REGS) wA[i] = twRegs.w[i];
				else wA[i] = twA[i*MA + t];
			}
#pragma unroll
			for (int n = 1; n < 16; ++n) {
				const float4 pr = wA[(n - 1) >> 1];
				w[n] = ((n - 1) & 1) ? fmake(pr.z, pr.w) : fmake(pr.x, pr.y);
			}
		}
#pragma unroll
		for (int f = 0; f < FRAMES; ++f) dft16<SIGN>(v[f]);
#pragma unroll
		for (int f = 0; f < FRAMES; ++f) {
#pragma unroll
			for (int pos = 0; pos < 16; ++pos) {
				const int n = (pos >> 2) + 4*(pos & 3);
				lds[f*BUF + 17*t + n] = n > 0 ? mulTwiddle<SIGN>(v[f][pos], w[n]) : v[f][pos]; // padded index of 16 t + n
			}
		}
	}
	firstWritten();
	sync();
	// stage B: radix 16, stride 16
	const int p = t >> 4, q0 = t & 15;
	if (t < MA) {
#pragma unroll
		for (int f = 0; f < FRAMES; ++f) {
#pragma unroll
			for (int k = 0; k < 16; ++k) v[f][k] = lds[f*BUF + q0 + 17*(p + R3*k)];
		}
	}
	sync();
	if (t < MA) {
		float4 wB[8];
#pragma unroll
		for (int i = 0; i < 8; ++i) wB[i] = twB[i*R3 + p];
#pragma unroll
		for (int f = 0; f < FRAMES; ++f) dft16<SIGN>(v[f]);
#pragma unroll
		for (int f = 0; f < FRAMES; ++f) {
#pragma unroll
			for (int pos = 0; pos < 16; ++pos) {
				const int n = (pos >> 2) + 4*(pos & 3);
				fc val = v[f][pos];
				if (n > 0) {
					const float4 pr = wB[(n - 1) >> 1];
					val = mulTwiddle<SIGN>(val, ((n - 1) & 1) ? fmake(pr.z, pr.w) : fmake(pr.x, pr.y));
				}
				lds[f*BUF + q0 + 256*p + 16*n] = val;
			}
		}
	}
	sync();
	// stage C: radix R3, stride 256, no twiddles
	if (t < 256) {
		constexpr int G = LastStage<R3>::G, RA = LastStage<R3>::RA;
		fc u[FRAMES][R3];
#pragma unroll
		for (int f = 0; f < FRAMES; ++f) {
#pragma unroll
			for (int k = 0; k < R3; ++k) u[f][k] = lds[f*BUF + t + 256*k];
		}
		lastRead();
		constexpr int CHUNK = ROUNDS ? R3/ROUNDS : (R3 <= 12 ? R3 : (R3 == 24 ? 6 : 5)); // outputs prepared ahead of their stores (R3 = 20 / 24: four rounds, or the registers cost a wave of occupancy; ROUNDS: the caller's choice)
		decltype(prepOf(0, 0, 0)) ready[FRAMES][CHUNK];
#pragma unroll
		for (int f = 0; f < FRAMES; ++f) {
#pragma unroll
			for (int i = 0; i < CHUNK; ++i) { // the first round's loads fly during the butterflies
				const int e = i/G, c = i - G*e;
				ready[f][i] = prepOf(t + 256*(e + RA*c), e + RA*c, f);
			}
		}
#pragma unroll
		for (int f = 0; f < FRAMES; ++f) dftLast<SIGN, R3>(u[f]);
#pragma unroll
		for (int f = 0; f < FRAMES; ++f) {
#pragma unroll
			for (int p0 = 0; p0 < R3; p0 += CHUNK) {
				if (p0 > 0) {
#pragma unroll
					for (int i = 0; i < CHUNK; ++i) {
						const int pos = p0 + i, e = pos/G, c = pos - G*e;
						if (pos < R3) ready[f][i] = prepOf(t + 256*(e + RA*c), e + RA*c, f);
					}
				}
#pragma unroll
				for (int i = 0; i < CHUNK; ++i) {
					const int pos = p0 + i, e = pos/G, c = pos - G*e;
					if (pos < R3) storeOf(t + 256*(e + RA*c), u[f][pos], ready[f][i], e + RA*c, f);
				}
			}
		}
	}
}

// ------------------------------------------------------------------------------------------------------
// What the frame kernels share: each step of a frame's way through analysis or synthesis is defined once.
// ------------------------------------------------------------------------------------------------------
constexpr int fastBlockThreads(int R3) { return 16*R3 > 256 ? 16*R3 : 256; } // stages A and B take 16*R3 threads, stage C 256

// which hops a launch analyses: those with a new spectrum that no earlier call analysed; which = 1 (the window one interval earlier) only where asked for
__device__ __forceinline__ bool hopWantsAnalysis(const HopDesc &hd, int which) {
	return (hd.flags & HOP_ACTIVE) && (hd.flags & HOP_NEW_SPECTRUM) && !(hd.flags & HOP_PREANALYSED) && (!which || (hd.flags & HOP_REANALYSE_PREV));
}

// A spectrum row in half-bin order: element j of the H-point transform is bin 2j while that is below H, and the conjugate of bin N - 1 - 2j above
__device__ __forceinline__ int halfBinIndex(int j, int H, int N) {
	const int kk = 2*j;
	return kk >= H ? N - 1 - kk : kk;
}
__device__ __forceinline__ fc loadHalfBin(const float2 *X, int j, int H, int N) {
	// one load at a selected address, conjugated afterwards: with a load in each arm of the conditional the
	// compiler emitted 16 loads each followed by s_waitcnt vmcnt(0) -- sixteen memory round trips per FFT
	return fconjLoad(X + halfBinIndex(j, H, N), 2*j >= H);
}
__device__ __forceinline__ void storeHalfBin(float2 *dst, int j, fc u, int H, int N) {
	fconjStore(dst + halfBinIndex(j, H, N), u, 2*j >= H);
}

// The windowed analysis element m = t + MA*slot from the full table w = (winA[m], winB[m]), where the window's halves change validity at
// element-slot boundaries (slot 0 has no imaginary part, slot 15 no real part): the same roundings as kAnalyseFast's general path,
// round(xi*b + round(xr*a)), with the absent half an exact zero
__device__ __forceinline__ float2 analysisElement(float4 w, float xr, float xi, int slot) { // (an absent half is not read: its sample is no operand)
	float2 r = make_float2(0.f, 0.f);
	if (slot < 15) r = make_float2(xr*w.x, xr*w.y);
	if (slot > 0) r = make_float2(fmaf(xi, w.z, r.x), fmaf(xi, w.w, r.y));
	return r;
}
// the element's two samples, fetched apart from their window entry (kAnalyseTeamPairs: all of a pass's samples are requested before the table is read)
__device__ __forceinline__ float2 analysisSamples(const float *x0, const float *x1, int m, int slot) {
	return make_float2(slot < 15 ? x0[m] : 0.f, slot > 0 ? x1[m] : 0.f);
}
__device__ __forceinline__ float2 analysisElement(float4 w, const float *x0, const float *x1, int m, int slot) {
	const float2 x = analysisSamples(x0, x1, m, slot);
	return analysisElement(w, x.x, x.y, slot);
}
// The lean tables' generated modulation e^{-i pi m/N} of element m = t + stride*k, where e^{-i pi stride/N} = e^{-i pi/per}: hb = halfTw[t] times one
// of `per` constants (compile-time after unrolling).  Analysis: k = slot, per = 32; synthesis: k = j, per = 2*R3.
__device__ __forceinline__ fc leanModulation(float2 hb, int k, int per) {
	const float ang = 3.14159265358979323846f*float(k)/float(per);
	return fmulExpr(fpack(hb), fmake(__builtin_cosf(ang), -__builtin_sinf(ang)));
}
// Synthesis output m of a frame into dst (the frame in memory, or kSynthEmitTeams' copy in LDS): u * e^{+i pi m/N} (tw = e^{-i pi m/N}), its real
// part under the window at m + B/2, its imaginary part at m - H + B/2
__device__ __forceinline__ void storeWindowed(float *dst, int m, fc u, fc tw, float wRe, float wIm, int B, int H) {
	const int halfB = B/2;
	const fc v = fmulc(u, tw); // * e^{+i pi m / N}
	if (m < B - halfB) dst[m + halfB] = (2*v.x)*wRe;
	if (m >= H - halfB) dst[m - H + halfB] = (2*v.y)*wIm;
}
__device__ __forceinline__ void storeWindowed(float *dst, int m, fc u, float4 r, int B, int H) { // r: the output's synTab entry
	storeWindowed(dst, m, u, fmake(r.x, r.y), r.z, r.w, B, H);
}

// (windowPad / analysisWindowInCall: smst_device.h -- the host scheduler evaluates the same condition)
template <int R3, bool LEAN>
__global__ __launch_bounds__(fastBlockThreads(R3)) __attribute__((amdgpu_waves_per_eu(4, 4))) void kAnalyseFast(DevBatch d, IoArgs io, int sBase, int hopBase, int lateOnly) {
	extern __shared__ __attribute__((aligned(16))) unsigned char smemRaw[];
	float2 *lds = reinterpret_cast<float2 *>(smemRaw);
	const BlockCoord bc = xcdAwareBlock();
	const int k = bc.x;
	const int c = bc.y >> 1;
	const int which = bc.y & 1;
	const int s = bc.s;
	const HopDesc hd = d.hops[(size_t)(sBase + s)*d.hopStride + hopBase + k];
	if (!hopWantsAnalysis(hd, which)) return;
	if (lateOnly && analysisWindowInCall(d.B, d.M, d.I, hd.inputOffset, which, io.inSamples[sBase + s])) return; // kAnalyseTeams has taken this frame
	const int B = d.B, H = d.M, halfB = B/2, N = d.N;
	const int base = hd.inputOffset - (which ? d.I : 0) - B;
	const float *x = io.in + (size_t)(sBase + s)*io.inStreamStride + (size_t)c*io.inChannelStride;
	const float *hist = d.hist + ((size_t)(sBase + s)*d.C + c)*(size_t)d.histPitch + d.histBase[d.histCur][sBase + s] + d.histLen;
	const float2 *__restrict__ winA = d.winA, *__restrict__ winB = d.winB;
	float2 *dst = (which ? d.Xprev : d.Xcur) + rowOf(d, s, k, c);
	auto prep = [](int, int) { return 0; };
	auto store = [&](int j, fc u, int, int) { storeHalfBin(dst, j, u, H, N); };
	constexpr int MA = 16*R3;
	const float4 *__restrict__ twA = LEAN ? d.twA6 : d.twA4;
	// LEAN: the folded window (w_re, w_im)(m) * e^{-i pi m/N} as TWO floats per element and the modulation generated: element
	// m = t + MA*slot, and e^{-i pi MA/N} = e^{-i pi/32} whatever the size, so the modulation is halfTw[t] times one of
	// sixteen constants (8 bytes per element instead of 16; six more multiply-adds per element, one more rounding)
	const float2 *__restrict__ win2 = d.win2;
	const float2 hb = LEAN ? d.halfTw[min((int)threadIdx.x, MA - 1)] : make_float2(0.f, 0.f);
	if (base >= 0 && H - halfB == MA && B - halfB == 15*MA) {
		// the usual case (both presets): the whole window lies in this call's input, and the two halves of the packed
		// input change validity exactly at element-slot boundaries: slot 0 has no imaginary part, slot 15 no real part
		const float *x0 = x + base + halfB, *x1 = x + base - H + halfB;
		const float4 *__restrict__ win4 = d.win4;
		fftFast<-1, R3, LEAN>(lds, twA, d.twB4,
			[&](int m, int slot) {
				if constexpr (LEAN) {
					const float2 w = win2[m];
					float2 z = make_float2(0.f, 0.f);
					if (slot < 15) z.x = x0[m]*w.x;
					if (slot > 0) z.y = x1[m]*w.y;
					return fmul<false>(fpack(z), leanModulation(hb, slot, 32));
				} else {
					return fpack(analysisElement(win4[m], x0, x1, m, slot)); // (winA, winB) in one 16-byte load
				}
			}, prep, store);
		return;
	}
	// the general case (a window that reaches into the carried history, or a block size whose halves do not fall on slot boundaries):
	// bounds-checked sample fetches, THE SAME ARITHMETIC as the fast case above, element for element -- a hop analysed in a short
	// call (history) and the same hop inside one long call must give the same bits (chunking invariance)
	fftFast<-1, R3, LEAN>(lds, twA, d.twB4,
		[&](int m, int slot) {
			float xr = 0, xi = 0;
			if (m < B - halfB) { int src = base + m + halfB; xr = (src >= 0) ? x[src] : hist[src]; }
			if (m >= H - halfB) { int src = base + m - H + halfB; xi = (src >= 0) ? x[src] : hist[src]; }
			if constexpr (LEAN) {
				const float2 w = win2[m];
				return fmul<false>(fmake(xr*w.x, xi*w.y), leanModulation(hb, slot, 32));
			} else {
				const float2 a = winA[m], b = winB[m];
				return fmake(fmaf(xi, b.x, xr*a.x), fmaf(xi, b.y, xr*a.y));
			}
		}, prep, store);
}

// ------------------------------------------------------------------------------------------------------
// K1 by persistent TEAMS (the default for the 2560- and 3072-bin geometries; SMST_FFT_TEAMS=0: one frame per workgroup): one workgroup per CU, three teams of 256 threads, each team transforming
// frame after frame AT ITS OWN PACE -- the barriers of a transform are the team's (an LDS counter its four waves spin on), not the
// workgroup's.  The folded window and the stage twiddles (76 KB) are copied to LDS once per workgroup and shared by the teams, so
// per frame only the samples come in and the spectrum goes out (kAnalyseFast pulls 74 KB of tables through L1 per frame).
// Same table values, same operations in the same order: bit-identical to kAnalyseFast.
// ------------------------------------------------------------------------------------------------------
struct TeamSync { // LDS operations of a wave complete in order: a wave's counter increment is seen after its data writes / reads
	volatile int *word;
	int *generation;
	__device__ __forceinline__ void operator()() const {
		asm volatile("" ::: "memory");
		__builtin_amdgcn_wave_barrier(); // (the CPU stand-in runs a wave lane by lane: every lane reaches the barrier before lane 0 signals)
		if ((threadIdx.x & 63) == 0) (void)__hip_atomic_fetch_add(const_cast<int *>(word), 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
		*generation += 4;
		while (__hip_atomic_load(const_cast<int *>(word), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < *generation) __builtin_amdgcn_s_sleep(1);
		__builtin_amdgcn_wave_barrier();
		asm volatile("" ::: "memory");
	}
};
// A team workgroup's prologue (every thread of the workgroup constructs one): its LDS is the 16-byte table of the kernel's elements
// (`source`: d.win4 or d.synTab, [H]), the first- and second-stage twiddles ([8][MA], [8][R3]), a transform buffer per team and the teams'
// barrier words -- teamLdsBytes() on the host.  The tables are copied and the words cleared once per workgroup.
// FRAMES = 2 (kAnalyseTeamPairs): two transform buffers per team, one behind the other, and no first-stage twiddles in LDS (the threads hold
// theirs in registers: StageTwiddles) -- the table, [8][R3] second-stage twiddles, TEAMS x FRAMES buffers, the barrier words.
template <int R3, int TEAMS, int FRAMES = 1>
struct TeamWorkgroup {
	static_assert(16*R3 <= 256, "a team is 256 threads");
	static constexpr int MA = 16*R3, H = 256*R3;
	float4 *table, *twA, *twB;
	float2 *lds;         // this team's transform buffer(s), H + H/16 each
	int team, t;         // the team, the thread within it
	volatile int *word;  // the team's barrier word
	int generation = 0;
	__device__ __forceinline__ TeamWorkgroup(unsigned char *smem, const DevBatch &d, const float4 *__restrict__ source) {
		team = __builtin_amdgcn_readfirstlane(threadIdx.x >> 8);
		t = threadIdx.x & 255;
		table = reinterpret_cast<float4 *>(smem);
		twA = table + H;
		twB = twA + (FRAMES == 1 ? 8*MA : 0);
		lds = reinterpret_cast<float2 *>(twB + 8*R3) + (size_t)team*FRAMES*(H + H/16);
		volatile int *words = reinterpret_cast<volatile int *>(reinterpret_cast<float2 *>(twB + 8*R3) + (size_t)TEAMS*FRAMES*(H + H/16));
		for (int i = threadIdx.x; i < H; i += blockDim.x) table[i] = source[i];
		if constexpr (FRAMES == 1) {
			for (int i = threadIdx.x; i < 8*MA; i += blockDim.x) twA[i] = d.twA4[i];
		} else {
			twA = nullptr;
		}
		for (int i = threadIdx.x; i < 8*R3; i += blockDim.x) twB[i] = d.twB4[i];
		if (threadIdx.x < 16) words[threadIdx.x] = 0;
		__syncthreads();
		word = words + team;
	}
	TeamWorkgroup(const TeamWorkgroup &) = delete;
	__device__ __forceinline__ TeamSync sync() { return TeamSync{word, &generation}; } // the team's barrier (it counts in this object)
};

// EXACT: block = 15/16 of the FFT size (windowPad = 0: the geometry is then a compile-time constant); otherwise see windowPad.
// Either way the arithmetic is kAnalyseFast's, element for element (an absent half contributes a zero: sample x zero weight).
template <int R3, int TEAMS, bool EXACT>
__global__ __launch_bounds__(256*TEAMS) void kAnalyseTeams(DevBatch d, IoArgs io, const HopDesc *__restrict__ hopTable, int sBase, int hopBase, int tileHops, int nStreams) {
	extern __shared__ __attribute__((aligned(16))) unsigned char smemRaw[];
	constexpr int MA = 16*R3, H = 256*R3, N = 2*H;
	const int B = EXACT ? 480*R3 : d.B, halfB = B/2; // EXACT: the geometry this kernel is launched for
	const int total = tileHops*2*d.C*nStreams;
	TeamWorkgroup<R3, TEAMS> wg(smemRaw, d, d.win4); // table: (winA, winB) of all elements
	const TeamSync sync = wg.sync();
	const int t = wg.t, tA = t < MA ? t : 0;
	const int stride = gridDim.x*TEAMS;
	for (int lin = blockIdx.x + gridDim.x*wg.team; lin < total; lin += stride) { // the same residue mod 8 for all of a workgroup's teams
		const BlockCoord bc = xcdAwareCoord(lin, tileHops, 2*d.C, nStreams);
		const HopDesc hd = hopTable[(size_t)(sBase + bc.s)*d.hopStride + hopBase + bc.x];
		const int c = bc.y >> 1, which = bc.y & 1;
		if (!hopWantsAnalysis(hd, which) || !analysisWindowInCall(B, H, d.I, hd.inputOffset, which, io.inSamples[sBase + bc.s])) continue;
		const int base = hd.inputOffset - (which ? d.I : 0) - B;
		const float *x = io.in + (size_t)(sBase + bc.s)*io.inStreamStride + (size_t)c*io.inChannelStride;
		const float *x0 = x + base + halfB, *x1 = x + base - H + halfB;
		float2 *dst = (which ? d.Xprev : d.Xcur) + rowOf(d, bc.s, bc.x, c);
		fftFast<-1, R3, false>(wg.lds, wg.twA, wg.twB,
			[&](int m, int slot) { return fpack(analysisElement(wg.table[tA + MA*slot], x0, x1, m, slot)); },
			[](int, int) { return 0; },
			[&](int j, fc u, int, int) { storeHalfBin(dst, j, u, H, N); }, t, sync);
		sync(); // the last stage's LDS reads, before the next frame's first-stage writes
	}
}

// kAnalyseTeams, two frames per team pass (the default; SMST_ANALYSE_PAIRS=0: the single-frame teams above).  A frame of kAnalyseTeams is one
// serial chain per team -- 30 loads, a radix-16 stage on 3 of its 4 waves, a barrier, another, a barrier, the last stage, 12 stores -- and three
// such chains per SIMD left the vector ALUs idle two thirds of the time.  Here a workgroup is TWO teams, two waves per SIMD with 256 registers
// each, and a team takes two frames through the transform in lockstep (fftFast<FRAMES = 2>): the two frames' butterflies are independent work
// inside each wave, a pass has the four team barriers a single frame had, and every window entry and stage twiddle is read once for the two.
// The first-stage twiddles depend on the thread alone and live in registers for the whole launch.
// A pass is two consecutive positions of ONE stream's job order (xcdAwareCoord's: the hop fastest, then channel and window) -- hops x and
// x + 1 of one (channel, window) but where a row of the order ends --, so both frames stay on the stream's XCD.  Each frame has its own
// predicate, exactly kAnalyseTeams' (what this kernel leaves, kAnalyseFast's lateOnly pass takes): a pass with one wanted frame transforms
// that frame alone, a pass with none is skipped.  inSamples: io.inSamples as a pointer the compiler may read through the scalar cache, like
// hopTable -- a pass begins with three scalar loads issued together and then all of its sample loads.
// Same table values, same operations in the same order on each frame: bit-identical to kAnalyseTeams and kAnalyseFast.
// TWIST (a twisted tile, DESIGN.md section 4: every hop analyses both of its windows, launchAnalyse): a pass is the TWO WINDOWS of one (hop, channel)
// -- frame 0 the current one, frame 1 the one an interval earlier -- so in the store step a thread holds the same bins of both, and what goes
// to the Xprev row is not the earlier window's spectrum but the previous-hop twist of the bin, prevHopTwist(cur, prev, rot), formed from the
// two values as they land in the rows (after the conjugation of the upper half).  The thread's bins never change: their twelve (R3)
// rotation factors live in registers for the whole launch.  A pass with one window in the call's input stores that frame raw, as above;
// kAnalyseFast takes the other one and kTwistRows turns the row afterwards.
template <int R3, bool EXACT, bool TWIST>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void kAnalyseTeamPairs(DevBatch d, IoArgs io, const HopDesc *__restrict__ hopTable, const int *__restrict__ inSamples, int sBase, int hopBase, int tileHops, int nStreams) {
	extern __shared__ __attribute__((aligned(16))) unsigned char smemRaw[];
	constexpr int TEAMS = 2, MA = 16*R3, H = 256*R3, N = 2*H;
	const int B = EXACT ? 480*R3 : d.B, halfB = B/2; // EXACT: the geometry this kernel is launched for
	const int jobs = tileHops*2*d.C;                 // of one stream
	const int passes = (jobs + 1)/2, total = passes*nStreams; // (TWIST: exactly tileHops*C passes of two frames)
	static_assert((H + 8*R3)*sizeof(float4) + TEAMS*2*(H + H/16)*sizeof(float2) + 64 <= 160*1024, "the window, the second-stage twiddles, four transform buffers and the barrier words fit a CU's LDS (155,200 bytes at R3 = 12)");
	TeamWorkgroup<R3, TEAMS, 2> wg(smemRaw, d, d.win4); // table: (winA, winB) of all elements
	const TeamSync sync = wg.sync();
	const int t = wg.t, tA = t < MA ? t : 0;
	StageTwiddles twA;
#pragma unroll
	for (int i = 0; i < 8; ++i) twA.w[i] = d.twA4[i*MA + tA];
	float2 rotOf[TWIST ? R3 : 1]; // TWIST: the hop rotation of the bins this thread stores (element t + 256*i of the last stage)
	if constexpr (TWIST) {
#pragma unroll
		for (int i = 0; i < R3; ++i) rotOf[i] = d.rot[halfBinIndex(t + 256*i, H, N)];
	}
	// Round i deals the passes [i*stride, (i + 1)*stride) to the teams, each team keeping its residue mod 8 (its XCD).  With a fixed place in
	// every round a team would move on by stride/8 passes of a stream per round -- 64 on 256 CUs, two whole rows of a 64-hop tile, so it would
	// meet the SAME window of the same or the other channel every time, and at stretch 1.0, where no hop re-analyses its previous window, one
	// team of every workgroup would find all of its passes unwanted.  The teams' places therefore rotate by `turn` per round (a bijection of
	// the round's passes onto the teams all the same), chosen so that a team moves on by an odd number of rows.
	const int stride = gridDim.x*TEAMS, rowPasses = TWIST ? tileHops : (tileHops + 1)/2;
	const int turn = 8*((((rowPasses - stride/8)%(2*rowPasses)) + 2*rowPasses)%(2*rowPasses));
	const int place = blockIdx.x + gridDim.x*wg.team;
	for (int round = 0; round*stride < total; ++round) {
		const int lin = round*stride + (place + round*turn)%stride;
		if (lin >= total) continue; // (the last round)
		const BlockCoord pc = xcdAwareCoord(lin, passes, 1, nStreams); // x: the pass of stream s
		const int nIn = inSamples[sBase + pc.s];
		HopDesc hd[2];
		BlockCoord bc[2];
		bool have[2];
#pragma unroll
		for (int f = 0; f < 2; ++f) {
			const int job = 2*pc.x + f;
			have[f] = job < jobs; // (an odd job count: the last pass has one frame)
			const int j = have[f] ? job : 2*pc.x;
			if constexpr (TWIST) { // pass pc.x = (hop, channel), the hop fastest; frame f = window f
				const int c = pc.x/tileHops;
				have[f] = true;
				bc[f].y = 2*c + f;
				bc[f].x = pc.x - c*tileHops;
			} else {
				bc[f].y = j/tileHops;
				bc[f].x = j - bc[f].y*tileHops;
			}
			bc[f].s = pc.s;
			hd[f] = hopTable[(size_t)(sBase + pc.s)*d.hopStride + hopBase + bc[f].x];
		}
		const float *x0[2], *x1[2];
		float2 *dst[2];
		bool on[2];
#pragma unroll
		for (int f = 0; f < 2; ++f) {
			const int c = bc[f].y >> 1, which = bc[f].y & 1;
			// (no short cut between the conditions: both descriptors and the stream's length are requested before the first of them is looked at)
			const bool wanted = hopWantsAnalysis(hd[f], which), inCall = analysisWindowInCall(B, H, d.I, hd[f].inputOffset, which, nIn);
			on[f] = have[f] & wanted & inCall;
			const int base = hd[f].inputOffset - (which ? d.I : 0) - B;
			const float *x = io.in + (size_t)(sBase + pc.s)*io.inStreamStride + (size_t)c*io.inChannelStride;
			x0[f] = x + base + halfB;
			x1[f] = x + base - H + halfB;
			dst[f] = (which ? d.Xprev : d.Xcur) + rowOf(d, pc.s, bc[f].x, c);
		}
		if (!on[0] && !on[1]) continue;
		auto prep = [](int, int, int = 0) { return 0; };
		if (on[0] && on[1]) {
			float4 win[16]; // the window entries of the thread's elements: one read for the two frames
			[[maybe_unused]] fc landed[TWIST ? R3 : 1]; // TWIST: frame 0's values as they went into the Xcur row (frame 0 is stored first)
			fftFast<-1, R3, false, 0, 2>(wg.lds, nullptr, wg.twB,
				[&](int m, int slot) {
					FrameSet<2> r;
#pragma unroll
					for (int f = 0; f < 2; ++f) r.f[f] = fpack(analysisSamples(x0[f], x1[f], m, slot));
					return r;
				},
				prep, [&](int j, fc u, int, int idx, int f) {
					if constexpr (TWIST) {
						const fc landedValue = fconjIf(u, 2*j >= H); // what storeHalfBin puts into the row
						float2 *row = dst[f] + halfBinIndex(j, H, N);
						if (f == 0) { landed[idx] = landedValue; *reinterpret_cast<fc *>(row) = landedValue; }
						else *row = prevHopTwist(funpack(landed[idx]), funpack(landedValue), rotOf[idx]);
					} else {
						storeHalfBin(dst[f], j, u, H, N);
					}
				}, t, sync, NoHook(),
				[&]() { // all 60 samples are on their way: the table is read under their latency, and nothing below moves above this point
#pragma unroll
					for (int slot = 0; slot < 16; ++slot) win[slot] = wg.table[tA + MA*slot];
					asm volatile("" ::: "memory");
				},
				NoHook(), [&](fc x, int, int slot, int) { return fpack(analysisElement(win[slot], x.x, x.y, slot)); }, twA);
		} else {
			const int f = on[0] ? 0 : 1; // the other slot does nothing
			const float *xa = x0[f], *xb = x1[f];
			float2 *dstOne = dst[f];
			fftFast<-1, R3, false>(wg.lds, nullptr, wg.twB,
				[&](int m, int slot) { return fpack(analysisElement(wg.table[tA + MA*slot], xa, xb, m, slot)); },
				prep, [&](int j, fc u, int, int) { storeHalfBin(dstOne, j, u, H, N); }, t, sync, NoHook(), NoHook(), NoHook(), NoArrival(), twA);
		}
		sync(); // the last stage's LDS reads, before the next pass's first-stage writes
	}
}

// A twisted tile's rows that the pair teams did not turn (a window of the hop reaches into the carried history: the first hops of a call;
// kAnalyseFast has written both spectra raw): Xprev := prevHopTwist(Xcur, Xprev, rot) in place, the operation kAnalyseTeamPairs<TWIST> applies in its
// store step.  Grid (the tile's first `lateHops` hops, channels, streams); teams: the pair kernel ran, and took the rows with both windows in the call.
__global__ __launch_bounds__(256) void kTwistRows(DevBatch d, IoArgs io, int sBase, int hopBase, int teams) {
	const int k = blockIdx.x, c = blockIdx.y, s = blockIdx.z;
	const HopDesc hd = d.hops[(size_t)(sBase + s)*d.hopStride + hopBase + k];
	if (!hopWantsAnalysis(hd, 1)) return;
	const int nIn = io.inSamples[sBase + s];
	if (teams && analysisWindowInCall(d.B, d.M, d.I, hd.inputOffset, 0, nIn) && analysisWindowInCall(d.B, d.M, d.I, hd.inputOffset, 1, nIn)) return;
	const float2 *cur = d.Xcur + rowOf(d, s, k, c);
	float2 *prev = d.Xprev + rowOf(d, s, k, c);
	for (int b = threadIdx.x; b < d.M; b += blockDim.x) prev[b] = prevHopTwist(cur[b], prev[b], d.rot[b]);
}

template <int R3, bool LEAN>
__global__ __launch_bounds__(fastBlockThreads(R3)) void kSynthFast(DevBatch d, int sBase, int hopBase) {
	extern __shared__ __attribute__((aligned(16))) unsigned char smemRaw[];
	float2 *lds = reinterpret_cast<float2 *>(smemRaw);
	const int k = blockIdx.x, c = blockIdx.y, s = blockIdx.z;
	const HopDesc hd = d.hops[(size_t)(sBase + s)*d.hopStride + hopBase + k];
	if (!(hd.flags & HOP_ACTIVE)) return;
	const int B = d.B, H = d.M, N = d.N;
	const float2 *X = d.OUT + rowOf(d, s, k, c);
	float *__restrict__ frame = frameOf(d, s, k, c);
	auto loadBin = [&](int j, int) { return loadHalfBin(X, j, H, N); };
	if constexpr (LEAN) {
		// an output needs e^{+i pi m/N} and its two window samples: the windows as one 8-byte load, the modulation generated --
		// m = t + 256 j, so it is halfTw[t] times one of R3 constants e^{-i pi j/(2 R3)} (conjugated in the product of storeWindowed)
		const float2 *__restrict__ win2 = d.win2;
		const float2 hb = d.halfTw[min((int)threadIdx.x, 255)];
		fftFast<+1, R3, true>(lds, d.twA6, d.twB4, loadBin,
			[&](int m, int) { return win2[m]; },
			[&](int m, fc u, float2 w, int j) { storeWindowed(frame, m, u, leanModulation(hb, j, 2*R3), w.x, w.y, B, H); });
	} else {
		const float4 *__restrict__ synTab = d.synTab;
		fftFast<+1, R3, false>(lds, d.twA4, d.twB4, loadBin,
			[&](int m, int) { // everything an output needs from memory in ONE 16-byte load (twiddle + its two window samples),
				// requested for all of a thread's outputs before the first store
				return synTab[m];
			},
			[&](int m, fc u, float4 r, int) { storeWindowed(frame, m, u, r, B, H); });
	}
}

// K4a by persistent teams (see kAnalyseTeams): kSynthFast's transform with kAnalyseTeams' organisation -- the (twiddle, window) table of
// the outputs and the stage twiddles sit in LDS, a team synthesises frame after frame at its own pace.  Bit-identical to kSynthFast.
template <int R3, int TEAMS>
__global__ __launch_bounds__(256*TEAMS) void kSynthTeams(DevBatch d, const HopDesc *__restrict__ hopTable, int sBase, int hopBase, int tileHops, int nStreams) {
	extern __shared__ __attribute__((aligned(16))) unsigned char smemRaw[];
	constexpr int H = 256*R3, N = 2*H;
	const int B = d.B;
	const int total = tileHops*d.C*nStreams;
	TeamWorkgroup<R3, TEAMS> wg(smemRaw, d, d.synTab); // table: (e^{-i pi m/N}, the two window samples of output m)
	const TeamSync sync = wg.sync();
	const int stride = gridDim.x*TEAMS;
	for (int lin = blockIdx.x + gridDim.x*wg.team; lin < total; lin += stride) {
		const BlockCoord bc = xcdAwareCoord(lin, tileHops, d.C, nStreams); // x: hop, y: channel
		const HopDesc hd = hopTable[(size_t)(sBase + bc.s)*d.hopStride + hopBase + bc.x];
		if (!(hd.flags & HOP_ACTIVE)) continue;
		const float2 *X = d.OUT + rowOf(d, bc.s, bc.x, bc.y);
		float *__restrict__ frame = frameOf(d, bc.s, bc.x, bc.y);
		fftFast<+1, R3, false>(wg.lds, wg.twA, wg.twB,
			[&](int j, int) { return loadHalfBin(X, j, H, N); },
			[&](int m, int) { return wg.table[m]; },
			[&](int m, fc u, float4 r, int) { storeWindowed(frame, m, u, r, B, H); }, wg.t, sync);
		sync(); // the last stage's LDS reads, before the next frame's first-stage writes
	}
}

// The carried front of the overlap-add under sample i of a tile (counted from where the carry begins): what the previous tile left -- sums per
// channel (`row`: the index of the row's first carried entry), window products per stream -- and behind it what an empty ring position holds
__device__ __forceinline__ float carriedSumAt(const DevBatch &d, size_t row, int i) { return i < d.carryLen ? loadCarrySum(d, d.carryCur, row + i) : 0.0f; }
__device__ __forceinline__ float carriedProductAt(const DevBatch &d, const float *__restrict__ carryWpOld, int i) { return i < d.carryLen ? carryWpOld[i] : 1e-30f; }
// The frames q with pos_q <= n < pos_q + B, pos_q = firstHopPos + q*I + delta, that cover any of the samples relFirst .. relLast
// (rel = n - firstHopPos - delta) among a tile's hopCount frames: empty where hi < lo
struct FrameRange { int lo, hi; };
__device__ __forceinline__ FrameRange coveringFrames(int relFirst, int relLast, int B, int I, int hopCount) {
	FrameRange r;
	r.hi = (relLast >= 0) ? relLast/I : -1;
	r.lo = (relFirst - B + 1 > 0) ? (relFirst - B + 1 + I - 1)/I : 0;
	if (r.hi > hopCount - 1) r.hi = hopCount - 1;
	return r;
}
// The window-product sum under output sample i of a tile (i counted from the tile's first sample): what the carry holds there, then
// the covering frames' products oldest first -- kEmit's sum, term for term.
__device__ __forceinline__ float windowProductAt(const DevBatch &d, const EmitDesc &ed, const float *__restrict__ carryWpOld, int i) {
	float wp = carriedProductAt(d, carryWpOld, i);
	if (ed.hopCount > 0) {
		const int rel = ed.nLo + i - ed.firstHopPos - d.delta;
		const FrameRange q = coveringFrames(rel, rel, d.B, d.I, ed.hopCount);
		for (int k = q.lo; k <= q.hi; ++k) wp += d.wprod[rel - k*d.I];
	}
	return wp;
}
// kSynthEmitTeams' companion: the window products do not depend on the channel or on the data, and from the sample on that the carried
// sums no longer reach they repeat with the interval -- the teams keep that steady pattern in registers.  What is left is per stream: the
// products under the tile's first wpHeadLen samples (-> wpHead) and under what the next tile starts from (-> the new carry).
__global__ __launch_bounds__(256) void kEmitProducts(DevBatch d, int sBase, int tileIndex) {
	const int sg = sBase + blockIdx.y;
	const EmitDesc ed = d.emit[(size_t)sg*d.emitStride + tileIndex];
	const int span = ed.nHi - ed.nLo, CL = d.carryLen;
	const float *carryWpOld = d.carryWp[d.carryCur] + carryWpRow(d, sg) + d.carryBase[d.carryCur][sg];
	const int i = blockIdx.x*blockDim.x + threadIdx.x;
	if (i == 0) d.carryBase[d.carryCur ^ 1][sg] = 0; // the new carry is written from the front of its rows (here and by kSynthEmitTeams)
	if (i < d.wpHeadLen) d.wpHead[(size_t)sg*d.wpHeadLen + i] = windowProductAt(d, ed, carryWpOld, i);
	else if (i - d.wpHeadLen < CL) d.carryWp[d.carryCur ^ 1][carryWpRow(d, sg) + (i - d.wpHeadLen)] = windowProductAt(d, ed, carryWpOld, span + (i - d.wpHeadLen));
}

// K4a + K4b in one kernel: synthesis, overlap-add, window-product normalisation and emission (signalsmith-stretch.h:397-415) without
// the frames ever reaching HBM.  A team of 256 threads takes ONE (stream, channel) of the tile and synthesises its hops in order;
// the overlap-add ring (the carried partial sums in front, NI = QN + 1 intervals) lives in the team's registers -- thread t owns
// the positions r = t + 256*slot of every interval.  Per hop: kSynthTeams' transform; its windowed outputs go to the team's own
// transform buffer (free once the last stage has read it) instead of HBM; each thread adds its positions of the QN intervals the frame
// covers, oldest frame first as kEmit (and the reference's ring) sums them; the interval that no later frame reaches is divided by
// its window products (kEmitProducts) and stored; the ring moves on by one interval.  The previous frame's additions run while the
// next frame's spectrum is on its way in.  Two teams per workgroup (the ring takes NI*SLOTS registers on top of the transform's), one
// workgroup per CU.  Same operations in the same order on the same values as kSynthTeams + kEmit: bit-identical output and carry
// (test_synth_emit_equals_two_kernels; at the edges of a tile, every instantiation: test_synth_emit_hoploop).
// The hop loop carries only what every hop needs.  GI, GB: the interval and the block where the launcher knows them (launchSynthEmit; 0: read
// from the batch) -- thread t owns r = t + 256*slot, so with the interval a constant every slot below I/256 needs no predicate, one partial
// slot tests t alone, and `a*I + r < B` is decided per (a, slot) but for one partial slot at most.  What only the edges of a tile need --
// the samples in front of the first hop, a stream without hops, the call's last interval (which may end behind ed.nHi), SPLIT's trailing
// interval, the carry write, the fp16 form of the carry -- sits in front of the loop and behind it, and the scalars it takes (SynthEmitEdge)
// are formed again behind the loop instead of living through it.
// Why an interval emitted INSIDE the loop is final as a whole: interval q is emitted while hop q + 1 <= cnt - 1 is transformed; the hops of a
// tile lie I samples apart, so the interval ends where hop q + 1 begins, and a hop begins inside its call (scheduleStream: outPos < nOut;
// split computation: its whole interval does) and not behind the tile's nHi (the next tile's first hop, or the call's end).
struct SynthEmitEdge {
	EmitDesc ed;
	float *out;           // the (stream, channel)'s output row
	size_t carryRow;      // the new carry's row
	size_t carried;       // the old carry's first entry
	const float *wpOld;   // the old carry's window products
};
__device__ __forceinline__ SynthEmitEdge synthEmitEdge(const DevBatch &d, const IoArgs &io, int sg, int c, int tileIndex) {
	SynthEmitEdge e;
	e.ed = d.emit[(size_t)sg*d.emitStride + tileIndex];
	const int carryFrom = d.carryBase[d.carryCur][sg];
	e.carryRow = carrySumRow(d, sg, c);
	e.carried = e.carryRow + carryFrom;
	e.wpOld = d.carryWp[d.carryCur] + carryWpRow(d, sg) + carryFrom;
	e.out = io.out + (size_t)sg*io.outStreamStride + (size_t)c*io.outChannelStride;
	return e;
}
// output sample n of the call: final, or part of what the next tile starts from
__device__ __forceinline__ void synthEmitPlace(const DevBatch &d, const SynthEmitEdge &e, int n, float sum, float wp) {
	if (n < e.ed.nHi) e.out[n] = sum/wp;
	else if (n - e.ed.nHi < d.carryLen) storeCarrySum(d, d.carryCur ^ 1, e.carryRow + (n - e.ed.nHi), sum);
}
template <int R3, int QN, int SLOTS, bool SPLIT, int GI, int GB>
__global__ __launch_bounds__(512) void kSynthEmitTeams(DevBatch d, IoArgs io, int sBase, int tileIndex, int nStreams) {
	constexpr int TEAMS = 2, MA = 16*R3, H = 256*R3, N = 2*H, NI = QN + 1, DQ = SPLIT ? 1 : 0;
	static_assert(GI == 0 || (GI <= 256*SLOTS && GI > 256*(SLOTS - 1) && QN*GI >= GB && GB <= N), "the geometry this instantiation is for");
	extern __shared__ __attribute__((aligned(16))) unsigned char smemRaw[];
	const int B = GI ? GB : d.B, I = GI ? GI : d.I;
	TeamWorkgroup<R3, TEAMS> wg(smemRaw, d, d.synTab); // table: (e^{-i pi m/N}, the two window samples of output m)
	const TeamSync sync = wg.sync();
	const int team = wg.team, t = wg.t;
	float2 *lds = wg.lds;
	float *ex = reinterpret_cast<float *>(lds); // the frame, B floats, in the transform buffer
	// position r = t + 256*slot of an interval exists / frame sample a*I + r exists: decided at compile time wherever GI, GB and t < 256 decide it
	auto inInterval = [&](int slot) { return 256*slot + t < I; };
	auto inFrame = [&](int a, int slot) { return 256*slot + t < I && a*I + 256*slot + t < B; };
	float steady[SLOTS]; // the window products under a sample that only this tile's frames cover: oldest frame first, as the ring sums them
#pragma unroll
	for (int slot = 0; slot < SLOTS; ++slot) {
		steady[slot] = 1e-30f;
#pragma unroll
		for (int a = QN - 1; a >= 0; --a) {
			if (inFrame(a, slot)) steady[slot] += d.wprod[a*I + 256*slot + t];
		}
		keepUnconditional(steady[slot]);
	}
	const int C = d.C, items = nStreams*C;
	const unsigned hopPitch = (unsigned)C*(unsigned)d.Mp; // from one hop's row of OUT to the next, in elements (rowOf)
	for (int item = blockIdx.x*TEAMS + team; item < items; item += gridDim.x*TEAMS) {
		const int s = item/C, c = item - s*C, sg = sBase + s;
		int cnt, off, firstHopPos;
		float acc[NI][SLOTS];
		{
			const SynthEmitEdge e = synthEmitEdge(d, io, sg, c, tileIndex);
			const int CL = d.carryLen;
			cnt = e.ed.hopCount;
			if (cnt == 0) { // nothing synthesised for this stream in this tile: the carried sums are emitted / move up
				const int span = e.ed.nHi - e.ed.nLo;
				for (int i = t; i < span + CL; i += 256) synthEmitPlace(d, e, e.ed.nLo + i, carriedSumAt(d, e.carried, i), carriedProductAt(d, e.wpOld, i));
				continue;
			}
			firstHopPos = e.ed.firstHopPos;
			off = firstHopPos - e.ed.nLo; // samples in front of the tile's first hop (the first tile of a call only)
			for (int i = t; i < off; i += 256) synthEmitPlace(d, e, e.ed.nLo + i, carriedSumAt(d, e.carried, i), carriedProductAt(d, e.wpOld, i));
#pragma unroll
			for (int u = 0; u < NI; ++u) {
#pragma unroll
				for (int slot = 0; slot < SLOTS; ++slot) {
					const int i = off + u*I + 256*slot + t;
					acc[u][slot] = inInterval(slot) ? carriedSumAt(d, e.carried, i) : 0.0f;
				}
			}
		}
		// (waited for HERE: a register that is still "being loaded" when the hop loop is entered makes the compiler wait for ALL loads at
		// its first use inside the loop -- i.e. for the spectrum that was requested just before)
#pragma unroll
		for (int u = 0; u < NI; ++u) {
#pragma unroll
			for (int slot = 0; slot < SLOTS; ++slot) keepUnconditional(acc[u][slot]);
		}
		// what the loop addresses: one base per item, 32-bit offsets per hop
		const float2 *spectra = d.OUT + rowOf(d, s, 0, c);            // hop q: + q*hopPitch
		float *outHops = io.out + (size_t)sg*io.outStreamStride + (size_t)c*io.outChannelStride + firstHopPos; // interval q: + q*I
		const float *wpHead = d.wpHead + (size_t)sg*d.wpHeadLen + off; // (kEmitProducts; it also writes the new carry's products) interval q: + q*I
		// frame q - 1 is added to the ring while frame q's spectrum is on its way in, and its finished interval leaves after frame
		// q's first-stage writes (no store between a load and its use: vmcnt counts both)
		auto overlapAdd = [&]() {
			float e[QN][SLOTS]; // all reads in flight together, no branch around any of them
			int tt = t;
			keepUnconditional(tt); // (the addresses are formed here, per hop: held across the loop they cost the registers the next spectrum needs)
#pragma unroll
			for (int a = 0; a < QN; ++a) {
#pragma unroll
				for (int slot = 0; slot < SLOTS; ++slot) {
					if (GI && (256*slot >= GI || a*GI + 256*slot >= GB)) continue; // no lane has this sample
					e[a][slot] = ex[inFrame(a, slot) ? a*I + 256*slot + tt : 0];
				}
			}
#pragma unroll
			for (int a = 0; a < QN; ++a) {
#pragma unroll
				for (int slot = 0; slot < SLOTS; ++slot) {
					if (GI && (256*slot >= GI || a*GI + 256*slot >= GB)) continue;
					keepUnconditional(e[a][slot]);
					acc[a + DQ][slot] = inFrame(a, slot) ? acc[a + DQ][slot] + e[a][slot] : acc[a + DQ][slot];
				}
			}
		};
		auto moveRing = [&]() {
#pragma unroll
			for (int u = 0; u + 1 < NI; ++u) {
#pragma unroll
				for (int slot = 0; slot < SLOTS; ++slot) acc[u][slot] = acc[u + 1][slot];
			}
#pragma unroll
			for (int slot = 0; slot < SLOTS; ++slot) acc[NI - 1][slot] = 0.0f;
		};
		// the window products under interval q: the steady pattern, but in the first NI intervals the carried products may reach into them
		// (loads of the kernel's own here too: see `next`)
		auto productsOf = [&](int q, float (&wp)[SLOTS]) {
#pragma unroll
			for (int slot = 0; slot < SLOTS; ++slot) wp[slot] = steady[slot];
			if (q < NI) {
				Async4 head[SLOTS];
				const float *from = wpHead + q*I;
#pragma unroll
				for (int slot = 0; slot < SLOTS; ++slot) asyncLoad4(head[slot], from + (inInterval(slot) ? 256*slot + t : 0));
				asyncWait<0>();
#pragma unroll
				for (int slot = 0; slot < SLOTS; ++slot) {
					asyncArrived(head[slot]);
					if (inInterval(slot)) wp[slot] = asyncValue(head[slot]);
				}
			}
		};
		auto emitFinal = [&](int q) { // an interval in front of the tile's last: final as a whole (see above)
			float wp[SLOTS];
			productsOf(q, wp);
			float *to = outHops + q*I;
#pragma unroll
			for (int slot = 0; slot < SLOTS; ++slot) {
				if (inInterval(slot)) to[256*slot + t] = acc[0][slot]/wp[slot];
			}
			moveRing();
		};
		// frame q + 1's spectrum is requested as soon as frame q's first stage has taken its own out of the registers
		// (loads the kernel waits for itself, smst_async.h: a compiler-tracked load whose value crosses the loop's back-edge makes the
		// compiler wait for EVERYTHING at the next barrier's counter update, i.e. right behind the request)
		Async8 next[16];
#pragma unroll
		for (int k = 0; k < 16; ++k) asyncClear(next[k]);
		auto request = [&](int q) {
			const float2 *X = spectra + (unsigned)q*hopPitch;
			if (t < MA) {
#pragma unroll
				for (int k = 0; k < 16; ++k) asyncLoad8(next[k], X + halfBinIndex(t + MA*k, H, N)); // one load at a selected address (see loadHalfBin) ...
			}
		};
		auto landed = [&]() { // at the END of a hop, in front of the back-edge: nothing of the compiler's may touch a register in flight
			asyncWait<0>();
#pragma unroll
			for (int k = 0; k < 16; ++k) asyncArrived(next[k]);
		};
		request(0);
		landed();
		for (int q = 0; q < cnt; ++q) {
			fftFast<+1, R3, false, 2>(lds, wg.twA, wg.twB, // (two rounds of prepared outputs: the ring and the next spectrum need the registers)
				[&](int, int k) { return fpack(asyncValue(next[k])); },
				[&](int m, int) { return wg.table[m]; },
				[&](int m, fc u, float4 r, int) { storeWindowed(ex, m, u, r, B, H); }, t, sync, sync,
				[&]() {
					if (q > 0) overlapAdd();
					sync(); // the previous frame has been read (or the previous item's last one), before this transform's first-stage writes
				},
				[&]() {
					if (q > 0) emitFinal(q - 1);
					request(q + 1 < cnt ? q + 1 : q);
				},
				[&](fc v, int j) { return fconjIf(v, 2*j >= H); }); // ... conjugated once it is there
			sync(); // the frame is complete
			landed();
		}
		overlapAdd();
		sync();
		// the edge behind the loop: the item's scalars again, from values the compiler cannot trace back through the loop
		int sgE = sg, cE = c;
		keepUnconditional(sgE);
		keepUnconditional(cE);
		const SynthEmitEdge e = synthEmitEdge(d, io, __builtin_amdgcn_readfirstlane(sgE), __builtin_amdgcn_readfirstlane(cE), tileIndex);
		auto emitEdge = [&](int q) { // an interval that may end behind ed.nHi: sample by sample
			float wp[SLOTS];
			productsOf(q, wp);
			const int n0 = firstHopPos + q*I;
#pragma unroll
			for (int slot = 0; slot < SLOTS; ++slot) {
				if (inInterval(slot)) synthEmitPlace(d, e, n0 + 256*slot + t, acc[0][slot], wp[slot]);
			}
			moveRing();
		};
		emitEdge(cnt - 1);
		// split computation: only blocks whose interval is complete are in the tile (the one in flight runs with a later call), so a call's
		// last tile may end up to an interval behind its last hop's interval: those samples leave like any other interval
		const bool trailing = SPLIT && firstHopPos + cnt*I < e.ed.nHi;
		if (trailing) emitEdge(cnt);
		const int n0 = firstHopPos + (cnt + (trailing ? 1 : 0))*I; // what the ring still holds: the start of the next tile's sums
#pragma unroll
		for (int u = 0; u < NI; ++u) {
#pragma unroll
			for (int slot = 0; slot < SLOTS; ++slot) {
				if (inInterval(slot)) synthEmitPlace(d, e, n0 + u*I + 256*slot + t, acc[u][slot], 1.0f); // (all of it behind the call's last final sample)
			}
		}
	}
}

// ------------------------------------------------------------------------------------------------------
// K5: per-stream input energy (silence gate, signalsmith-stretch.h:231-238)
// ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void kEnergy(DevBatch d, IoArgs io, int sBase, float *__restrict__ energyOut) {
	// grid (stream, part): partial sums, the host adds the kEnergyParts partials of a stream (short inputs are launched with fewer parts:
	// the slots that are left hold zeros)
	const int s = blockIdx.x, part = blockIdx.y, parts = gridDim.y;
	if (part == 0 && (int)threadIdx.x >= parts && (int)threadIdx.x < kEnergyParts) energyOut[(size_t)(sBase + s)*kEnergyParts + threadIdx.x] = 0.0f;
	const int n = io.inSamples[sBase + s];
	const int lo = (int)((long long)n*part/parts), hi = (int)((long long)n*(part + 1)/parts);
	float acc = 0;
	for (int c = 0; c < d.C; ++c) {
		const float *x = io.in + (size_t)(sBase + s)*io.inStreamStride + (size_t)c*io.inChannelStride;
		for (int i = lo + threadIdx.x; i < hi; i += blockDim.x) {
			float v = x[i];
			acc += v*v;
		}
	}
	extern __shared__ __attribute__((aligned(16))) unsigned char smemRaw[];
	float *red = reinterpret_cast<float *>(smemRaw);
	red[threadIdx.x] = acc;
	__syncthreads();
	for (int w = 128; w > 0; w >>= 1) {
		if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
		__syncthreads();
	}
	if (threadIdx.x == 0) energyOut[(size_t)(sBase + s)*kEnergyParts + part] = red[0];
}

// ------------------------------------------------------------------------------------------------------
// K1: analysis.  One workgroup per (hop, channel x {current, previous}, stream):
// gather B samples ending at the hop's input offset from the contiguous per-channel sample block (or the
// carried history for negative indices), multiply by the analysis window, fold into the N/2-point complex
// sequence of the half-bin-shifted real FFT, Stockham FFT in LDS, write the M = N/2 bins.
// Replaces stft.analyseStep at signalsmith-stretch.h:337,:359 (+ the copies :344-350,:366-372).
// ------------------------------------------------------------------------------------------------------
// BIG (blocks whose two ping-pong buffers do not fit a CU's LDS: presetDefault / presetCheaper at 176.4 / 192 kHz, 12288 / 10240 bins): one buffer
// in LDS, the other in memory -- the frame's own output row, which nobody reads before the kernel has finished.  The Stockham passes then
// alternate between LDS and HBM (L2 in practice: 96 KB per workgroup): slower than the LDS-resident form, the same arithmetic in the same order.
template <bool BIG>
__global__ __launch_bounds__(256) void kAnalyse(DevBatch d, IoArgs io, int sBase, int hopBase) {
	extern __shared__ __attribute__((aligned(16))) unsigned char smemRaw[];
	float2 *bufA = reinterpret_cast<float2 *>(smemRaw);
	float2 *bufB = bufA + d.M;

	const BlockCoord bc = xcdAwareBlock();
	const int k = bc.x;
	const int c = bc.y >> 1;
	const int which = bc.y & 1; // 0: current window, 1: window one interval earlier
	const int s = bc.s;
	const HopDesc hd = d.hops[(size_t)(sBase + s)*d.hopStride + hopBase + k];
	if (!hopWantsAnalysis(hd, which)) return;

	const int B = d.B, H = d.M, halfB = B/2;
	const int base = hd.inputOffset - (which ? d.I : 0) - B; // index of block element 0 in the call's input
	const float *x = io.in + (size_t)(sBase + s)*io.inStreamStride + (size_t)c*io.inChannelStride;
	const float *hist = d.hist + ((size_t)(sBase + s)*d.C + c)*(size_t)d.histPitch + d.histBase[d.histCur][sBase + s];
	const float *__restrict__ win = d.window;
	float2 *dst = (which ? d.Xprev : d.Xcur) + rowOf(d, s, k, c);
	if (BIG) bufB = dst;

	for (int m = threadIdx.x; m < H; m += blockDim.x) {
		float re = 0, im = 0;
		if (m < B - halfB) {
			int i = m + halfB;
			int src = base + i;
			float v = (src >= 0) ? x[src] : hist[d.histLen + src];
			re = v*win[i];
		}
		if (m >= H - halfB) {
			int i = m - H + halfB;
			int src = base + i;
			float v = (src >= 0) ? x[src] : hist[d.histLen + src];
			im = v*win[i];
		}
		bufA[m] = funpack(fmul<false>(fmake(re, im), fpack(d.halfTw[m])));
	}
	__syncthreads();
	float2 *res = fftLds<-1>(bufA, bufB, d.plan, d.twH);
	if (BIG && res == dst) { // the last pass ended in the output row: through LDS once more, the final order is a permutation of it
		for (int j = threadIdx.x; j < H; j += blockDim.x) bufA[j] = dst[j];
		__syncthreads();
		res = bufA;
	}
	const int N = d.N;
	for (int j = threadIdx.x; j < H; j += blockDim.x) storeHalfBin(dst, j, fpack(res[j]), H, N);
}

// ------------------------------------------------------------------------------------------------------
// K4a: synthesis.  One workgroup per (hop, channel, stream): inverse half-bin-shifted real FFT (gain N),
// multiply by the synthesis window, store the B-sample frame.  Replaces the copy at
// signalsmith-stretch.h:384-394 + stft.synthesiseStep (:397-399).
// ------------------------------------------------------------------------------------------------------
template <bool BIG> // BIG: the second buffer in memory (DevBatch::fftScratch, a row per frame), see kAnalyse
__global__ __launch_bounds__(256) void kSynth(DevBatch d, int sBase, int hopBase) {
	extern __shared__ __attribute__((aligned(16))) unsigned char smemRaw[];
	float2 *bufA = reinterpret_cast<float2 *>(smemRaw);
	float2 *bufB = bufA + d.M;
	const int k = blockIdx.x, c = blockIdx.y, s = blockIdx.z;
	if (BIG) bufB = d.fftScratch + rowOf(d, s, k, c);
	const HopDesc hd = d.hops[(size_t)(sBase + s)*d.hopStride + hopBase + k];
	if (!(hd.flags & HOP_ACTIVE)) return;
	const int B = d.B, H = d.M, N = d.N, halfB = B/2;
	const float2 *X = d.OUT + rowOf(d, s, k, c);
	for (int j = threadIdx.x; j < H; j += blockDim.x) bufA[j] = funpack(loadHalfBin(X, j, H, N));
	__syncthreads();
	float2 *res = fftLds<+1>(bufA, bufB, d.plan, d.twH);
	float *frame = frameOf(d, s, k, c);
	const float *__restrict__ win = d.window;
	for (int m = threadIdx.x; m < H; m += blockDim.x) {
		const float wRe = (m < B - halfB) ? win[m + halfB] : 0.0f, wIm = (m >= H - halfB) ? win[m - H + halfB] : 0.0f; // (the absent halves are not stored)
		storeWindowed(frame, m, fpack(res[m]), fpack(d.halfTw[m]), wRe, wIm, B, H);
	}
}

// ------------------------------------------------------------------------------------------------------
// K4b: overlap-add as a gather + window-product normalisation + emission (stft.readOutput/moveOutput at
// signalsmith-stretch.h:406-415), and the new carry (the part of the ring that outlives the tile).
// Sums are formed oldest-frame-first, as the reference's ring accumulates them.
// ------------------------------------------------------------------------------------------------------
// KMAX = the frames whose loads are issued together: ceil((B + 3)/I) cover a group of four samples (3 for presetCheaper, 5 for presetDefault);
// a slot beyond that is a load instruction for nothing, and the kernel lives on the number of those (EXPERIMENTS.md 6.10).
template <int KMAX>
__global__ __launch_bounds__(256) void kEmit(DevBatch d, IoArgs io, int sBase, int tileIndex) {
	// four consecutive output samples per thread: the frame / window-product taps of a group are 16-byte loads
	// (dword alignment suffices on gfx9), and the two integer divisions are paid once per group
	const int s = blockIdx.z, sg = sBase + s, c = blockIdx.y;
	const EmitDesc ed = d.emit[(size_t)sg*d.emitStride + tileIndex];
	const int span = ed.nHi - ed.nLo;
	const int i0 = 4*(blockIdx.x*blockDim.x + threadIdx.x);
	const int CL = d.carryLen;
	const int total = span + CL;
	if (i0 >= total) return;
	const int B = d.B, I = d.I;
	const int carryFrom = d.carryBase[d.carryCur][sg];
	const size_t carryRow = carrySumRow(d, sg, c);
	const float *carryWpOld = d.carryWp[d.carryCur] + carryWpRow(d, sg) + carryFrom;
	if (i0 == 0 && c == 0) d.carryBase[d.carryCur ^ 1][sg] = 0; // the new carry is written from the front of its rows
	float sum[4], wp[4];
	if (i0 + 3 < CL && !d.halfState) {
		const float4 a = *reinterpret_cast<const float4 *>(d.carrySum[d.carryCur] + carryRow + carryFrom + i0), b = *reinterpret_cast<const float4 *>(carryWpOld + i0);
		sum[0] = a.x; sum[1] = a.y; sum[2] = a.z; sum[3] = a.w;
		wp[0] = b.x; wp[1] = b.y; wp[2] = b.z; wp[3] = b.w;
	} else {
#pragma unroll
		for (int j = 0; j < 4; ++j) {
			const int i = i0 + j;
			sum[j] = carriedSumAt(d, carryRow + carryFrom, i);
			wp[j] = carriedProductAt(d, carryWpOld, i);
		}
	}
	if (ed.hopCount > 0) {
		// frames q with pos_q <= n < pos_q + B, pos_q = firstHopPos + q*I + delta; summed in ascending q per sample
		const int rel0 = ed.nLo + i0 - ed.firstHopPos - d.delta;
		const FrameRange cover = coveringFrames(rel0, rel0 + 3, B, I, ed.hopCount);
		const int qLo = cover.lo, qHi = cover.hi;
		// all covering frames' loads are issued before the first addition (a loop with a load per iteration costs one
		// memory round trip per frame); the additions then run in ascending q, the order the reference sums in
		float4 f[KMAX], w[KMAX];
		bool fast[KMAX];
#pragma unroll
		for (int k = 0; k < KMAX; ++k) {
			const int q = qLo + k, idx0 = rel0 - q*I;
			fast[k] = q <= qHi && idx0 >= 0 && idx0 + 3 < B;
			const float *frame = frameOf(d, s, fast[k] ? q : 0, c);
			f[k] = *reinterpret_cast<const float4 *>(frame + (fast[k] ? idx0 : 0));
			w[k] = *reinterpret_cast<const float4 *>(d.wprod + (fast[k] ? idx0 : 0));
		}
#pragma unroll
		for (int k = 0; k < KMAX; ++k) {
			const int q = qLo + k, idx0 = rel0 - q*I;
			if (fast[k]) {
				sum[0] += f[k].x; sum[1] += f[k].y; sum[2] += f[k].z; sum[3] += f[k].w;
				wp[0] += w[k].x; wp[1] += w[k].y; wp[2] += w[k].z; wp[3] += w[k].w;
			} else if (q <= qHi) { // a group that straddles a frame edge
				const float *frame = frameOf(d, s, q, c);
#pragma unroll
				for (int j = 0; j < 4; ++j) {
					const int idx = idx0 + j;
					if (idx >= 0 && idx < B) { sum[j] += frame[idx]; wp[j] += d.wprod[idx]; }
				}
			}
		}
		for (int q = qLo + KMAX; q <= qHi; ++q) { // more than KMAX covering frames (block/interval > 5): plain loop
			const int idx0 = rel0 - q*I;
			const float *frame = frameOf(d, s, q, c);
#pragma unroll
			for (int j = 0; j < 4; ++j) {
				const int idx = idx0 + j;
				if (idx >= 0 && idx < B) { sum[j] += frame[idx]; wp[j] += d.wprod[idx]; }
			}
		}
	}
	float *out = io.out + (size_t)sg*io.outStreamStride + (size_t)c*io.outChannelStride + ed.nLo;
	if (i0 + 3 < span) {
		*reinterpret_cast<float4 *>(out + i0) = make_float4(sum[0]/wp[0], sum[1]/wp[1], sum[2]/wp[2], sum[3]/wp[3]);
	} else {
#pragma unroll
		for (int j = 0; j < 4; ++j) {
			const int i = i0 + j;
			if (i < span) {
				out[i] = sum[j]/wp[j];
			} else if (i < total) {
				storeCarrySum(d, d.carryCur ^ 1, carryRow + (i - span), sum[j]);
				if (c == 0) d.carryWp[d.carryCur ^ 1][carryWpRow(d, sg) + (i - span)] = wp[j];
			}
		}
	}
}

// A call in which no stream fires a hop (most quanta of the 128-frame real-time pattern): its output is the front of the carried sums over
// their window products -- kEmit's quotient -- and the carry that is left BEGINS LATER in the same rows instead of being copied
// (B+I entries per row and call otherwise).  One workgroup per stream, so nobody reads the window's beginning while it moves.
__global__ __launch_bounds__(256) void kEmitCarried(DevBatch d, IoArgs io) {
	const int sg = blockIdx.x;
	const EmitDesc ed = d.emit[(size_t)sg*d.emitStride];
	const int span = ed.nHi - ed.nLo, from = d.carryBase[d.carryCur][sg];
	const float *wpRow = d.carryWp[d.carryCur] + carryWpRow(d, sg) + from;
	for (int c = 0; c < d.C; ++c) {
		const size_t row = carrySumRow(d, sg, c) + from;
		float *out = io.out + (size_t)sg*io.outStreamStride + (size_t)c*io.outChannelStride + ed.nLo;
		for (int i = threadIdx.x; i < span; i += blockDim.x) {
			out[i] = carriedSumAt(d, row, i)/carriedProductAt(d, wpRow, i);
		}
	}
	__syncthreads();
	if (threadIdx.x == 0) d.carryBase[d.carryCur][sg] = from + span;
}

// ------------------------------------------------------------------------------------------------------
// host-side launchers
// ------------------------------------------------------------------------------------------------------
void launchEnergy(const DevBatch &d, const IoArgs &io, int sBase, int nStreams, int maxSamples, float *energyOut, hipStream_t st) {
	// a part per 1024 samples of the longest input: a 128-frame quantum of 4096 streams is 4096 workgroups, not 65536 (56 -> 8 us)
	const int parts = std::max(1, std::min(kEnergyParts, maxSamples/1024));
	hipLaunchKernelGGL(kEnergy, dim3(nStreams, parts), dim3(256), 256*sizeof(float), st, d, io, sBase, energyOut);
}
// f(R3 = M/256 as a compile-time constant) where M/256 is one of R3S; false, and f not called, at any other size
template <int... R3S, typename F>
static bool withR3(int M, F f) { return M%256 == 0 && withInt<R3S...>(M/256, f); }
// The register-blocked kernels exist at four sizes (isFastSize), the team kernels at the two whose stages A and B fit a team's 256 threads
template <typename F> static bool withFastR3(int M, F f) { return withR3<10, 12, 20, 24>(M, f); }
template <typename F> static bool withTeamR3(int M, F f) { return withR3<10, 12>(M, f); }
static size_t fastLdsBytes(int M) { return ((size_t)M + M/16)*sizeof(float2); } // fftFast's padded buffer
static size_t teamLdsBytes(int M, int teams, int frames = 1) { // TeamWorkgroup: element table, first- and second-stage twiddles, a buffer per team and frame, barrier words
	const size_t twA = frames == 1 ? M/2 : 0; // (two frames per pass: the first-stage twiddles are in registers)
	return ((size_t)M + twA + M/32)*sizeof(float4) + teams*frames*fastLdsBytes(M) + 64;
}
static bool fastApplies(const DevBatch &d) { return !d.noFastFft && isFastSize(d.M); }
// (asks withTeamR3 itself, so a launcher that finds the teams to apply always has a team kernel to launch)
static bool teamsAvailable(const DevBatch &d) { return fastApplies(d) && withTeamR3(d.M, [](auto) {}) && d.fftTeams && !d.fftLean; }
// persistent teams pay a 76-KB table copy per workgroup: only where every team gets a few frames
static bool teamsApply(const DevBatch &d, int jobs) { return teamsAvailable(d) && (d.fftTeams == 2 || jobs >= 6*d.teamsGrid); }
// the analysis teams take two frames per pass (kAnalyseTeamPairs) wherever they apply: both geometries measured ahead of the single-frame form
static bool analysePairsApply(const DevBatch &d) { return d.analysePairs != 0; }
static int pairWorkgroups(const DevBatch &d, int passes) { // two teams each, otherwise as teamsWorkgroups
	return std::max(8, std::min((passes + 1)/2/8*8, d.teamsGrid));
}
static int teamsWorkgroups(const DevBatch &d, int jobs) { // three teams each: one workgroup per CU, a multiple of 8 (one residue class of the job order per XCD)
	return std::max(8, std::min((jobs + 2)/3/8*8, d.teamsGrid));
}
// kSynthEmitTeams' shape: the presets' block / interval ratios (2.5 and 4)
constexpr int synthEmitQN(int R3) { return R3 == 10 ? 3 : 4; }
constexpr int synthEmitSlots(int R3) { return R3 == 10 ? 8 : 6; }

// what a twisted tile's analysis is built on: the pair teams take the tile (the frames they leave -- none in most tiles -- go through kTwistRows)
bool analyseTwistApplies(const DevBatch &d, int nStreams, int tileHops) { return teamsApply(d, tileHops*d.C*2*nStreams) && analysePairsApply(d); }

void launchAnalyse(const DevBatch &d, const IoArgs &io, int sBase, int nStreams, int hopBase, int tileHops, bool anyInCall, bool anyLate, hipStream_t st, bool twisted, int lateHops) {
	const dim3 grid(tileHops, d.C*2, nStreams);
	const int jobs = tileHops*d.C*2*nStreams;
	const bool teams = anyInCall && teamsApply(d, jobs);
	if (teams) {
		const WindowPad pad = windowPad(d.B, d.M);
		const bool pairs = analysePairsApply(d);
		const int passes = (tileHops*d.C*2 + 1)/2*nStreams;
		withTeamR3(d.M, [&](auto r3) { withFlag(pad.lo == 0 && pad.hi == 0, [&](auto exact) {
			if (pairs && twisted) hipLaunchKernelGGL((kAnalyseTeamPairs<r3.value, exact.value, true>), dim3(pairWorkgroups(d, passes)), dim3(512), teamLdsBytes(d.M, 2, 2), st, d, io, d.hops, io.inSamples, sBase, hopBase, tileHops, nStreams);
			else if (pairs) hipLaunchKernelGGL((kAnalyseTeamPairs<r3.value, exact.value, false>), dim3(pairWorkgroups(d, passes)), dim3(512), teamLdsBytes(d.M, 2, 2), st, d, io, d.hops, io.inSamples, sBase, hopBase, tileHops, nStreams);
			else hipLaunchKernelGGL((kAnalyseTeams<r3.value, 3, exact.value>), dim3(teamsWorkgroups(d, jobs)), dim3(768), teamLdsBytes(d.M, 3), st, d, io, d.hops, sBase, hopBase, tileHops, nStreams);
		}); });
		countLaunch(LK_ANALYSE_TEAMS); // (either form)
		if (pairs) countLaunch(LK_ANALYSE_PAIRS);
		if (pairs && twisted) countLaunch(LK_ANALYSE_TWIST);
		if (!anyLate) return;
	}
	auto twistRows = [&] { // behind the kernel that wrote the late frames, on the same stream
		if (!twisted || lateHops <= 0) return;
		hipLaunchKernelGGL(kTwistRows, dim3(std::min(lateHops, tileHops), d.C, nStreams), dim3(256), 0, st, d, io, sBase, hopBase, teams ? 1 : 0);
		countLaunch(LK_TWIST_ROWS);
	};
	const int lateOnly = teams ? 1 : 0; // the frames whose windows reach into the carried history
	countLaunch(fastApplies(d) ? LK_ANALYSE_FAST : LK_ANALYSE_GENERIC);
	// every preset: presetCheaper at 44.1 / 48 kHz, presetDefault at 44.1 / 48 kHz, presetCheaper at 88.2 / 96 kHz, presetDefault at 88.2 / 96 kHz
	if (!d.noFastFft && withFastR3(d.M, [&](auto r3) { withFlag(d.fftLean != 0, [&](auto lean) {
			hipLaunchKernelGGL((kAnalyseFast<r3.value, lean.value>), grid, dim3(fastBlockThreads(r3.value)), fastLdsBytes(d.M), st, d, io, sBase, hopBase, lateOnly);
		}); })) { twistRows(); return; }
	size_t lds = 2*(size_t)d.M*sizeof(float2);
	if (fftNeedsScratch(d.M)) hipLaunchKernelGGL(kAnalyse<true>, grid, dim3(256), lds/2, st, d, io, sBase, hopBase);
	else hipLaunchKernelGGL(kAnalyse<false>, grid, dim3(256), lds, st, d, io, sBase, hopBase);
	twistRows();
}
void launchSynth(const DevBatch &d, int sBase, int nStreams, int hopBase, int tileHops, hipStream_t st) {
	const dim3 grid(tileHops, d.C, nStreams);
	const int jobs = tileHops*d.C*nStreams;
	if (teamsApply(d, jobs)) {
		withTeamR3(d.M, [&](auto r3) {
			hipLaunchKernelGGL((kSynthTeams<r3.value, 3>), dim3(teamsWorkgroups(d, jobs)), dim3(768), teamLdsBytes(d.M, 3), st, d, d.hops, sBase, hopBase, tileHops, nStreams);
		});
		countLaunch(LK_SYNTH_TEAMS);
		return;
	}
	countLaunch(fastApplies(d) ? LK_SYNTH_FAST : LK_SYNTH_GENERIC);
	if (!d.noFastFft && withFastR3(d.M, [&](auto r3) { withFlag(d.fftLean != 0, [&](auto lean) {
			hipLaunchKernelGGL((kSynthFast<r3.value, lean.value>), grid, dim3(fastBlockThreads(r3.value)), fastLdsBytes(d.M), st, d, sBase, hopBase);
		}); })) return;
	size_t lds = 2*(size_t)d.M*sizeof(float2);
	if (fftNeedsScratch(d.M)) hipLaunchKernelGGL(kSynth<true>, grid, dim3(256), lds/2, st, d, sBase, hopBase);
	else hipLaunchKernelGGL(kSynth<false>, grid, dim3(256), lds, st, d, sBase, hopBase);
}
bool synthEmitApplies(const DevBatch &d, int nStreams, int tileHops) {
	if (!teamsAvailable(d) || !d.synthEmit) return false;
	if (!(d.delta == 0 || d.delta == d.I)) return false;
	const int QN = synthEmitQN(d.M/256), SLOTS = synthEmitSlots(d.M/256);
	if (QN*d.I < d.B || d.I > 256*SLOTS || d.B > d.N) return false;
	// the teams read wpHead[off + q*I + r] for q <= QN, r < I, with off = the samples in front of a tile's first hop (< I: a block begins at
	// the latest I - 1 samples into a call, smst_engine.cpp): inside the (ceil(B/I) + 2)*I floats per stream only if QN >= ceil(B/I) -- stated, not assumed
	if ((QN + 2)*d.I > d.wpHeadLen) return false;
	// one (stream, channel) per team, its hops in sequence.  Measured on 256 CUs (profiles/r4_synth_emit_sweep.txt): ahead of the two
	// kernels from 32 stereo streams on, at every batch size up to 1024 -- also where the last round of teams is mostly empty
	return d.synthEmit == 2 || (tileHops >= 8 && nStreams*d.C >= 64);
}
void launchEmitProducts(const DevBatch &d, int sBase, int nStreams, int tileIndex, hipStream_t st) {
	hipLaunchKernelGGL(kEmitProducts, dim3(divUp(d.wpHeadLen + d.carryLen, 256), nStreams), dim3(256), 0, st, d, sBase, tileIndex);
}
// kSynthEmitTeams with the interval and the block as constants (and as many slots as the interval takes): presetDefault and presetCheaper at
// 48 and 44.1 kHz.  Every other geometry that synthEmitApplies() accepts takes the instantiation that reads them from the batch.
template <int GI, int GB> struct SynthEmitGeometry { static constexpr int interval = GI, block = GB, slots = (GI + 255)/256; };
template <int R3, typename F>
static void withSynthEmitGeometry(const DevBatch &d, F f) { // f(geometry, slots)
	using Slots = std::integral_constant<int, synthEmitSlots(R3)>;
	auto is = [&](auto g) { return d.I == g.interval && d.B == g.block && (f(g, std::integral_constant<int, g.slots>()), true); };
	if constexpr (R3 == 12) { if (is(SynthEmitGeometry<1440, 5760>()) || is(SynthEmitGeometry<1323, 5292>())) return; }
	if constexpr (R3 == 10) { if (is(SynthEmitGeometry<1920, 4800>()) || is(SynthEmitGeometry<1764, 4410>())) return; }
	f(SynthEmitGeometry<0, 0>(), Slots());
}
void launchSynthEmit(const DevBatch &d, const IoArgs &io, int sBase, int nStreams, int tileIndex, hipStream_t st) {
	const int items = nStreams*d.C;
	const int wgs = std::min(divUp(items, 2), d.teamsGrid); // two teams each
	withTeamR3(d.M, [&](auto r3) { withFlag(d.delta != 0, [&](auto split) { withSynthEmitGeometry<r3.value>(d, [&](auto g, auto slots) {
		hipLaunchKernelGGL((kSynthEmitTeams<r3.value, synthEmitQN(r3.value), slots.value, split.value, g.interval, g.block>), dim3(wgs), dim3(512), teamLdsBytes(d.M, 2), st, d, io, sBase, tileIndex, nStreams);
	}); }); });
	countLaunch(LK_SYNTH_EMIT);
}
void launchEmit(const DevBatch &d, const IoArgs &io, int sBase, int nStreams, int tileIndex, int maxSpan, hipStream_t st) {
	const dim3 grid(divUp(divUp(maxSpan + d.carryLen, 4), 256), d.C, nStreams);
	const int covering = divUp(d.B + 3, d.I); // frames that can cover a group of four output samples
	if (covering <= 3) hipLaunchKernelGGL(kEmit<3>, grid, dim3(256), 0, st, d, io, sBase, tileIndex);
	else if (covering <= 4) hipLaunchKernelGGL(kEmit<4>, grid, dim3(256), 0, st, d, io, sBase, tileIndex);
	else if (covering <= 5) hipLaunchKernelGGL(kEmit<5>, grid, dim3(256), 0, st, d, io, sBase, tileIndex);
	else hipLaunchKernelGGL(kEmit<6>, grid, dim3(256), 0, st, d, io, sBase, tileIndex); // (more covering frames: the kernel's plain loop takes the rest)
}
void launchEmitCarried(const DevBatch &d, const IoArgs &io, hipStream_t st) {
	hipLaunchKernelGGL(kEmitCarried, dim3(d.S), dim3(256), 0, st, d, io);
	countLaunch(LK_EMIT_CARRIED);
}

} // namespace smst
