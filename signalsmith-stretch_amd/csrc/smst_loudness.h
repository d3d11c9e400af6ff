// Integrated loudness (ITU-R BS.1770-4) of whole clips at the batch API's boundary (include/smst.h, "Loudness", has the definition): Batch::exact
// measures the planar fp32 output image in front of the levelled kClipOut, which takes the stream's gain gL from the meters left here.
// Included by smst_state.hip only, behind smst_clip.h.  Everything up to gL is float64.
//
// The K-weighting is a fourth-order recurrence over each channel of each clip -- sequential in time.  It is cut, in CLIP ORDER (position p of
// a clip lies at seg0.src + p of its row for p < seg0.count, at seg1.src + p - seg0.count behind that), into chunks of kLoudChunk frames, one
// lane per chunk, and run as a linear system x' = A x + B u in the cascade's transposed direct form II (4 state values):
//   kLoudChunks<false>  every lane filters its chunk from zero state and keeps the state it ends in         -> ends[stream, channel, chunk]
//   kLoudCarry          per (stream, channel), in chunk order: x_in[k + 1] = A^chunk x_in[k] + ends[k]      -> ends[] now holds x_in[]
//   kLoudChunks<true>   every lane filters its chunk again from its true incoming state and sums y^2 into the one or two 100-ms
//                       sub-blocks the chunk overlaps (h >= kLoudChunk: the host refuses a lower rate)       -> partials[stream, channel, chunk][2]
//   kLoudGate           one workgroup per stream: sub-block sums from the partials in chunk order, block powers with the channel weights in
//                       channel order, the two gates with sums in block order                                -> Z, the two counts, gL
// Every sum has one fixed order and no pass uses a floating-point atomic, so a run is bit-reproducible whatever the scheduling.
//
// Staging.  The 64 lanes of a wavefront walk 64 different chunks, 1 KiB apart: read directly, every load instruction would touch 64 cache
// lines for 4 bytes each.  So a wavefront stages kLoudTile floats of each of its 64 chunks into LDS at a time, as the aligned 16-byte words
// that cover them (kClipPeak's scheme: a word that lies inside the segment's run is read whole, one at a run's end element by element; a
// tile that the join of the two segments cuts has two such runs, kLoudWords words at the most between them), consecutive lanes taking
// consecutive words of a row.  The LDS rows are kLoudTile + 1 floats apart: lane r reads float r*33 + i, bank (r + i) mod 32, so the 32
// lanes of a ds_read_b32 group hit 32 banks.
#pragma once
#include "smst_clip.h"

namespace smst {

constexpr int kLoudTile = 32;                  // floats of a chunk that a wavefront stages at a time
constexpr int kLoudPitch = kLoudTile + 1;      // floats between two LDS rows
constexpr int kLoudWords = kLoudTile/4 + 3;    // aligned words that cover a tile's two runs of n0 + n1 = 32 floats: (n0 + 6)/4 + (n1 + 6)/4 at the most
constexpr int kLoudWaves = 4;                  // wavefronts per workgroup of kLoudChunks
constexpr int kLoudCarryAhead = 8;             // chunk ends that kLoudCarry reads ahead of the one it folds in
static_assert(kLoudChunk%kLoudTile == 0 && kLoudTile%4 == 0, "a chunk is a whole number of tiles, a tile a whole number of words");
inline size_t loudLdsBytes() { return size_t(kLoudWaves)*64*kLoudPitch*sizeof(float); }

struct LoudState { double s1, s2, s3, s4; };
// one sample through the shelf and the high-pass: returns y
__device__ inline double loudStep(const LoudCoef &k, LoudState &x, double u) {
	const double y1 = k.b0*u + x.s1;
	x.s1 = k.b1*u - k.a1*y1 + x.s2;
	x.s2 = k.b2*u - k.a2*y1;
	const double y = y1 + x.s3;
	x.s3 = -2.0*y1 - k.d1*y + x.s4;
	x.s4 = y1 - k.d2*y;
	return y;
}
// ... and its square into the partial sum it belongs to.  One source form for every pass and for the stream meter (smst_stream_meter.h): the
// library is built with -ffp-contract=on, so the form decides the fusing
__device__ inline void loudEnergyStep(const LoudCoef &k, LoudState &x, double u, double &e) {
	const double y = loudStep(k, x, u);
	e += y*y;
}
// x_in of the next chunk: next = A^chunk x + end, end the state the chunk reaches from zero state (likewise one source form).
// Here and in loudSumStep both operands of an operation can be NaN -- A^chunk itself is not finite where the shelf is unstable --, and the
// hardware's result then has the sign of the operand that comes first.  The compiler orders the operands of a product or a sum as it
// likes, kernel by kernel, so on the device the order is written down: a product, three fused multiply-adds and a sum -- what
// -ffp-contract=on makes of the expression -- in the order kLoudCarry was compiled to before the step became a function: the state in front
// of the matrix element in the product, the matrix element in front in the multiply-adds, the products in front of `end`
__device__ inline void loudCarryStep(const double *A, const double *x, const double *end, double *next) {
#if defined(__HIP_DEVICE_COMPILE__)
	for (int i = 0; i < 4; ++i) {
		double t;
		asm("v_mul_f64 %0, %1, %2" : "=v"(t) : "v"(x[0]), "v"(A[4*i]));
		asm("v_fma_f64 %0, %1, %2, %0" : "+v"(t) : "v"(A[4*i + 1]), "v"(x[1]));
		asm("v_fma_f64 %0, %1, %2, %0" : "+v"(t) : "v"(A[4*i + 2]), "v"(x[2]));
		asm("v_fma_f64 %0, %1, %2, %0" : "+v"(t) : "v"(A[4*i + 3]), "v"(x[3]));
		asm("v_add_f64 %0, %1, %2" : "=v"(next[i]) : "v"(t), "v"(end[i]));
	}
#else
	for (int i = 0; i < 4; ++i) next[i] = A[4*i]*x[0] + A[4*i + 1]*x[1] + A[4*i + 2]*x[2] + A[4*i + 3]*x[3] + end[i];
#endif
}
// one addend of a sub-block's sum, the sum in front: kLoudGate's first stage, and the stream meter's running sum
__device__ inline void loudSumStep(double &sum, double part) {
#if defined(__HIP_DEVICE_COMPILE__)
	asm("v_add_f64 %0, %0, %1" : "+v"(sum) : "v"(part));
#else
	sum += part;
#endif
}

// Word `word` of the aligned 16-byte words that cover run[0, n): its floats inside the run go to dst[their index].  [lo, hi): the indices
// around run[0] that the segment owns (lo <= 0, n <= hi); a word inside them is read whole, another one element by element
__device__ inline void loudStageWord(const float *__restrict__ run, int n, int word, int lo, int hi, float *dst) {
	const int back = int((reinterpret_cast<uintptr_t>(run) >> 2) & 3u); // floats between the 16-byte boundary at or in front of run and it
	const int a = 4*word - back;
	if (a >= n) return;
	if (a >= lo && a + 4 <= hi) {
		const PcmWord4 v = *reinterpret_cast<const PcmWord4 *>(run + a);
		for (int k = 0; k < 4; ++k) if (a + k >= 0 && a + k < n) dst[a + k] = __int_as_float(int(v[k]));
	} else {
		for (int k = 0; k < 4; ++k) if (a + k >= 0 && a + k < n) dst[a + k] = run[a + k];
	}
}
__device__ inline int loudWordsOf(const float *run, int n) { return n > 0 ? (int((reinterpret_cast<uintptr_t>(run) >> 2) & 3u) + n + 3)/4 : 0; }

// grid (tiles of kLoudWaves*64 chunks, C, S), 256 threads: lane l of wavefront v of workgroup x has chunk (x*kLoudWaves + v)*64 + l
template <bool Energy> __global__ __launch_bounds__(256) void kLoudChunks(const float *__restrict__ image, long long imageStreamStride, long long imageChannelStride,
		const ClipSeg *__restrict__ segs, const LoudEntry *__restrict__ loud, LoudScratch w) {
	extern __shared__ __attribute__((aligned(16))) unsigned char smemRaw[];
	const int s = blockIdx.z, c = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
	const int h = loud[s].h;
	const ClipSeg g0 = segs[2*s], g1 = segs[2*s + 1];
	if (h == 0 || g0.zeros || g1.zeros) return;
	const int n0 = max(g0.count, 0), n1 = max(g1.count, 0), N = n0 + n1;
	const int nChunks = (N + kLoudChunk - 1)/kLoudChunk;
	if (int(blockIdx.x)*kLoudWaves*64 >= nChunks) return;
	const int kWave = (int(blockIdx.x)*kLoudWaves + (tid >> 6))*64, k = kWave + lane;
	const LoudCoef coef = loud[s].k;
	const size_t slot = ((size_t)s*gridDim.y + c)*w.maxChunks + k;
	LoudState x{0.0, 0.0, 0.0, 0.0};
	if (Energy && k < nChunks) x = LoudState{w.ends[4*slot], w.ends[4*slot + 1], w.ends[4*slot + 2], w.ends[4*slot + 3]};
	const long long p0 = (long long)k*kLoudChunk;                  // the chunk's first position in the clip
	const long long split = (p0/h + 1)*h;                           // ... and the first one of the second sub-block it reaches
	double e0 = 0.0, e1 = 0.0;
	float *rows = reinterpret_cast<float *>(smemRaw) + (size_t)(tid >> 6)*64*kLoudPitch;
	const float *row = image + (size_t)s*imageStreamStride + (size_t)c*imageChannelStride;
	for (int j = 0; j < kLoudChunk/kLoudTile; ++j) {
		for (int it = 0; it < kLoudWords; ++it) {
			const int i = it*64 + lane, r = i/kLoudWords, word = i%kLoudWords;
			const long long t0 = (long long)(kWave + r)*kLoudChunk + j*kLoudTile; // row r's tile begins here
			if (t0 >= N) continue;
			const int t = int(t0), n = min(kLoudTile, N - t);
			const int nA = min(max(n0 - t, 0), n), q = t + nA - n0;               // floats of the tile in segment 0; where the rest begins in segment 1
			const int wordsA = loudWordsOf(row + g0.src + t, nA);
			if (word < wordsA) loudStageWord(row + g0.src + t, nA, word, -t, n0 - t, rows + r*kLoudPitch);
			else if (nA < n) loudStageWord(row + g1.src + q, n - nA, word - wordsA, -q, n1 - q, rows + r*kLoudPitch + nA);
		}
		__syncthreads();
		const long long q0 = p0 + j*kLoudTile;
		const int n = q0 < N ? min(kLoudTile, N - int(q0)) : 0;
		const float *mine = rows + lane*kLoudPitch;
		if constexpr (Energy) {
			const int first = int(min(max(split - q0, 0ll), (long long)n));        // samples of the tile in the chunk's first sub-block
			for (int i = 0; i < first; ++i) loudEnergyStep(coef, x, double(mine[i]), e0);
			for (int i = first; i < n; ++i) loudEnergyStep(coef, x, double(mine[i]), e1);
		} else {
			for (int i = 0; i < n; ++i) loudStep(coef, x, double(mine[i]));
		}
		__syncthreads(); // (the next tile goes into the same rows)
	}
	if (k >= nChunks) return;
	if constexpr (Energy) {
		w.partials[2*slot] = e0; w.partials[2*slot + 1] = e1;
	} else {
		w.ends[4*slot] = x.s1; w.ends[4*slot + 1] = x.s2; w.ends[4*slot + 2] = x.s3; w.ends[4*slot + 3] = x.s4;
	}
}

// ends[k] := x_in[k], one lane per (stream, channel): grid (ceil(S*C/64)), 64 threads.  The chain is short -- a 4x4 product per chunk --
// but every step needs a chunk's end from memory, so the ends are read kLoudCarryAhead chunks ahead of the chain
__global__ __launch_bounds__(64) void kLoudCarry(const ClipSeg *__restrict__ segs, const LoudEntry *__restrict__ loud, int S, int C, LoudScratch w) {
	const int sc = blockIdx.x*64 + threadIdx.x;
	if (sc >= S*C) return;
	const int s = sc/C;
	const ClipSeg g0 = segs[2*s], g1 = segs[2*s + 1];
	if (loud[s].h == 0 || g0.zeros || g1.zeros) return;
	const int N = max(g0.count, 0) + max(g1.count, 0), nChunks = (N + kLoudChunk - 1)/kLoudChunk;
	double A[16];
	for (int i = 0; i < 16; ++i) A[i] = loud[s].Ac[i];
	double *p = w.ends + (size_t)sc*w.maxChunks*4;
	double x[4] = {0.0, 0.0, 0.0, 0.0}, ahead[kLoudCarryAhead][4], cur[kLoudCarryAhead][4];
	auto read = [&](int k0) {
		for (int u = 0; u < kLoudCarryAhead; ++u) for (int i = 0; i < 4; ++i) ahead[u][i] = k0 + u < nChunks ? p[(size_t)4*(k0 + u) + i] : 0.0;
	};
	read(0);
	for (int k0 = 0; k0 < nChunks; k0 += kLoudCarryAhead) {
		for (int u = 0; u < kLoudCarryAhead; ++u) for (int i = 0; i < 4; ++i) cur[u][i] = ahead[u][i];
		read(k0 + kLoudCarryAhead);
		for (int u = 0; u < kLoudCarryAhead && k0 + u < nChunks; ++u) {
			double *at = p + (size_t)4*(k0 + u);
			double next[4];
			for (int i = 0; i < 4; ++i) at[i] = x[i];
			loudCarryStep(A, x, cur[u], next);
			for (int i = 0; i < 4; ++i) x[i] = next[i];
		}
	}
}

// grid (S), 256 threads; LDS: 256 doubles.  Writes every stream's meters: one that is not measured (h == 0, a run of zeros, nothing) has no block.
// FromPartials false: the sub-block sums are in w.sub already (the stream meter's histories, smst_stream_meter.h) -- the first stage is left out
template <bool FromPartials> __global__ __launch_bounds__(256) void kLoudGate(const ClipSeg *__restrict__ segs, const LoudEntry *__restrict__ loud, const float *__restrict__ weights, int C, LoudScratch w) {
	extern __shared__ __attribute__((aligned(16))) unsigned char smemRaw[];
	double *tile = reinterpret_cast<double *>(smemRaw); // [256]
	const int s = blockIdx.x, tid = threadIdx.x;
	const int h = loud[s].h;
	const ClipSeg g0 = segs[2*s], g1 = segs[2*s + 1];
	const int N = (h == 0 || g0.zeros || g1.zeros) ? 0 : max(g0.count, 0) + max(g1.count, 0);
	const int nb = (h > 0 && N/4 >= h) ? (N - 4*h)/h + 1 : 0, nSub = nb ? nb + 3 : 0; // (block i: sub-blocks i ... i + 3)
	double *sub = w.sub + (size_t)s*C*w.maxSub, *z = w.z + (size_t)s*w.maxSub;
	if constexpr (FromPartials) for (int idx = tid; idx < C*nSub; idx += 256) {
		const int c = idx/nSub, j = idx%nSub;
		const int k0 = int((long long)j*h/kLoudChunk), k1 = int(((long long)(j + 1)*h - 1)/kLoudChunk);
		const double *part = w.partials + ((size_t)s*C + c)*w.maxChunks*2;
		double sum = 0.0;
		for (int k = k0; k <= k1; ++k) loudSumStep(sum, part[2*(size_t)k + ((long long)k*kLoudChunk/h == j ? 0 : 1)]);
		sub[(size_t)c*w.maxSub + j] = sum;
	}
	__syncthreads();
	for (int i = tid; i < nb; i += 256) {
		double acc = 0.0;
		for (int c = 0; c < C; ++c) {
			const double *q = sub + (size_t)c*w.maxSub + i;
			acc += double(weights[c])*(((q[0] + q[1]) + q[2]) + q[3]);
		}
		z[i] = acc/(4.0*h);
	}
	__syncthreads();
	// the gates, power domain.  The blocks go through LDS 256 at a time; lane 0 sums them in block order
	const double gate = loud[s].gate;
	double sum = 0.0, rel = 0.0;
	int passed[2] = {0, 0};
	for (int pass = 0; pass < 2; ++pass) {
		sum = 0.0;
		for (int base = 0; base < nb; base += 256) {
			if (base + tid < nb) tile[tid] = z[base + tid];
			__syncthreads();
			if (tid == 0) for (int i = 0; i < min(256, nb - base); ++i) if (tile[i] > gate && (pass == 0 || tile[i] > rel)) { sum += tile[i]; ++passed[pass]; }
			__syncthreads();
		}
		if (pass == 0 && passed[0]) rel = 0.1*(sum/passed[0]);
	}
	if (tid) return;
	const double Z = passed[1] ? sum/passed[1] : 0.0;
	w.Z[s] = Z;
	w.counts[2*s] = passed[0]; w.counts[2*s + 1] = passed[1];
	w.gain[s] = (passed[1] && Z > 0.0 && Z*0.5 < Z) ? float(sqrt(loud[s].P/Z)) : 1.0f; // (Z*0.5 < Z: finite)
}

bool loudEntryOf(double sampleRate, double targetLufs, LoudEntry &e) {
	e = LoudEntry{};
	const double hop = std::floor(sampleRate/10 + 0.5);
	if (!(hop >= kLoudChunk && hop <= double(1 << 27))) return false;
	const double pi = 3.14159265358979323846;
	{ // shelf
		const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
		const double K = std::tan(pi*f0/sampleRate), Vh = std::pow(10.0, G/20), Vb = std::pow(Vh, 0.4996667741545416), a0 = 1 + K/Q + K*K;
		e.k.b0 = (Vh + Vb*K/Q + K*K)/a0; e.k.b1 = 2*(K*K - Vh)/a0; e.k.b2 = (Vh - Vb*K/Q + K*K)/a0;
		e.k.a1 = 2*(K*K - 1)/a0; e.k.a2 = (1 - K/Q + K*K)/a0;
	}
	{ // high-pass
		const double f0 = 38.13547087602444, Q = 0.5003270373238773;
		const double K = std::tan(pi*f0/sampleRate), d = 1 + K/Q + K*K;
		e.k.d1 = 2*(K*K - 1)/d; e.k.d2 = (1 - K/Q + K*K)/d;
	}
	// x' = A x + B u of loudStep: A, then A^kLoudChunk by squaring
	static_assert((kLoudChunk & (kLoudChunk - 1)) == 0, "A^chunk is formed by squaring");
	double A[16] = {-e.k.a1, 1, 0, 0,  -e.k.a2, 0, 0, 0,  -2 - e.k.d1, 0, -e.k.d1, 1,  1 - e.k.d2, 0, -e.k.d2, 0};
	for (int n = kLoudChunk; n > 1; n >>= 1) {
		double B[16];
		for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) B[4*i + j] = A[4*i]*A[j] + A[4*i + 1]*A[4 + j] + A[4*i + 2]*A[8 + j] + A[4*i + 3]*A[12 + j];
		for (int i = 0; i < 16; ++i) A[i] = B[i];
	}
	for (int i = 0; i < 16; ++i) e.Ac[i] = A[i];
	e.P = std::pow(10.0, (targetLufs + 0.691)/10);
	e.gate = std::pow(10.0, (-70 + 0.691)/10);
	e.h = int(hop);
	e.Pm = e.Ps = __builtin_inf();
	return true;
}

void launchClipLoudness(const float *image, long long imageSS, long long imageCS, const ClipSeg *segs, int S, int C, const LoudEntry *loud, const float *weights, const LoudScratch &w, hipStream_t st) {
	const dim3 grid(divUp(w.maxChunks, kLoudWaves*64), C, S);
	hipLaunchKernelGGL(kLoudChunks<false>, grid, dim3(256), loudLdsBytes(), st, image, imageSS, imageCS, segs, loud, w);
	hipLaunchKernelGGL(kLoudCarry, dim3(divUp(S*C, 64)), dim3(64), 0, st, segs, loud, S, C, w);
	hipLaunchKernelGGL(kLoudChunks<true>, grid, dim3(256), loudLdsBytes(), st, image, imageSS, imageCS, segs, loud, w);
	hipLaunchKernelGGL(kLoudGate<true>, dim3(S), dim3(256), 256*sizeof(double), st, segs, loud, weights, C, w);
	countLaunch(LK_CLIP_LOUDNESS);
}

} // namespace smst
