// The R 128 meters' streaming form at the batch API's boundary (include/smst.h, "Stream meter", has the definition): smst_batch_process_pcm and
// smst_batch_flush_pcm measure the call's planar fp32 output image behind the output conversion.  Included by smst_state.hip only, behind
// smst_stream_limiter.h.  Every step is the clip meters' own (loudEnergyStep, loudStep, loudCarryStep of smst_loudness.h; truePeakFrameBits of
// smst_true_peak.h) in the clip meters' order, so the frames v[0, Tm) a stream has had metered give the bits that the clip meters give of
// the clip v[0, Tm), however they were cut into calls.
//
// What a stream carries (smst_device.h, PcmStreamMeter): per channel the chunk in progress -- x_in, the state run from it, the state run from
// zero, e0 and e1, the running sum of the sub-block in progress -- and Tm, the last 11 frames, the running true-peak and sample-peak words,
// its configuration and the closed sub-block sums.  ONE set of it: a lane of kPcmStreamMeter reads and writes the state of its own (stream,
// channel) only; kPcmStreamMeterPeak, launched in front of it on the same stream, only READS what is carried (Tm and the 11 frames) and maxes
// integers into the two words, whose order does not matter.  Everything is ordered by the batch's stream, the setter's clear included.
//
// kPcmStreamMeterPeak.  One lane per new frame f: |x| into both words, and the window that frame completes -- the one of frame Tm + f - 6,
// whose 12 taps end at frame f -- from the 11 carried frames and the image.  The six windows behind that, which the clip form closes against
// zeros, are never folded in: kPcmStreamMeterRead forms them from the carried frames for a reading.
//
// kPcmStreamMeter.  One lane per (stream, channel) continues the chunk in progress over the call's frames.  A wavefront's 64 lanes read 64
// different rows, so the rows are staged through LDS in tiles of kLoudTile floats, consecutive lanes reading consecutive floats of a row, the
// LDS rows kLoudPitch floats apart (kLoudChunks' banking).  Chunk ends and sub-block ends inside the call are handled in the lane: at a
// sub-block's end the chunk's e0 closes the running sum, which goes to the history; at a chunk's end e0 (the chunk lay inside one sub-block)
// or e1 (it straddled two) opens or continues the running sum -- kLoudGate's first stage, one addend at a time in chunk order -- and
// x_in' = A^chunk x_in + (the state run from zero), kLoudCarry's step.
//
// The chunk-scan form serves long calls, which one lane per row cannot: kPcmStreamMeterChunks<false> (zero-state runs of the call's chunks),
// kPcmStreamMeterCarry (the chain from the carried x_in), kPcmStreamMeterChunks<true> (the energy runs) and kPcmStreamMeterClose (the
// sub-block sums in chunk order, the new carried state) -- the clip meter's passes with a start position and a carried state, on a scratch
// of 6 doubles per chunk.  Both forms give the same bits; the host picks by the call's longest metered count (kStreamMeterScanFrames).
//
// A reading (launchPcmStreamMeterRead): kLoudGate from its second stage on and kLoudRange on the histories, with a one-segment table of
// count Tm, then kPcmStreamMeterRead for the true-peak edge and the newest momentary and short-term powers.
#pragma once
#include "smst_stream_limiter.h"
#include "smst_loudness_range.h"
#include "smst_true_peak.h"

namespace smst {

// the frames of stream s that a call of `count` frames has metered: the setting, and what the history still holds
__device__ inline int streamMeterFrames(const StreamMeterConfig &cfg, double done, int count) {
	if (!cfg.on || count < 1) return 0;
	const long long left = (long long)cfg.cap - (long long)done;
	return int(min((long long)count, max(left, 0ll)));
}

// grid (tiles of 256 frames of the call, C, S), 256 threads.  starts: null, or the column of each stream's first frame of the call
__global__ __launch_bounds__(256) void kPcmStreamMeterPeak(const float *__restrict__ image, long long imageStreamStride, long long imageChannelStride, const int *__restrict__ counts,
		const int *__restrict__ starts, int S, TruePeakTable taps, PcmStreamMeter m) {
	const int s = blockIdx.z, c = blockIdx.y, tid = threadIdx.x, C = gridDim.y;
	const size_t sc = (size_t)s*C + c;
	const double done = m.state[sc*kStreamMeterDoubles + kStreamMeterAt];
	const int n = streamMeterFrames(m.config[s], done, counts[s]);
	if ((long long)blockIdx.x*256 >= n) return;
	const int f = int(blockIdx.x)*256 + tid;
	unsigned sample = 0u, most = 0u;
	if (f < n) {
		const float *row = image + (size_t)s*imageStreamStride + (size_t)c*imageChannelStride + (starts ? starts[s] : 0);
		const float *line = m.frames + sc*kStreamMeterLine;
		sample = pcmPeakBits(row[f]);
		if ((long long)done + f >= kTruePeakTrail) { // (the window of frame Tm + f - 6: its taps are frames f - 11 ... f of the call)
			float at[kTruePeakTaps];
#pragma unroll
			for (int j = 0; j < kTruePeakTaps; ++j) at[j] = f + j < kStreamMeterLine ? line[f + j] : row[f + j - kStreamMeterLine];
			unsigned bits[1];
			truePeakFrameBits<1>(at, taps, bits);
			most = bits[0];
		}
		most = max(most, sample);
	}
	int a = int(sample), b = int(most);
	for (int k = 32; k; k >>= 1) { a = max(a, __shfl(a, (tid & 63) ^ k)); b = max(b, __shfl(b, (tid & 63) ^ k)); }
	if ((tid & 63) == 0) {
		if (b > 0) atomicMax(m.words + s, b);
		if (a > 0) atomicMax(m.words + S + s, a);
	}
}

// grid (ceil(S*C/64)), 64 threads; LDS: streamMeterLdsBytes().  Lane l of workgroup x has (stream, channel) number x*64 + l
inline size_t streamMeterLdsBytes() { return size_t(64)*kLoudPitch*sizeof(float) + 64*sizeof(long long) + 64*sizeof(int); }
__global__ __launch_bounds__(64) void kPcmStreamMeter(const float *__restrict__ image, long long imageStreamStride, long long imageChannelStride, const int *__restrict__ counts,
		const int *__restrict__ starts, int S, int C, PcmStreamMeter m) {
	extern __shared__ __attribute__((aligned(16))) unsigned char smemRaw[];
	float *rows = reinterpret_cast<float *>(smemRaw);                               // [64][kLoudPitch]
	long long *rowAt = reinterpret_cast<long long *>(rows + 64*kLoudPitch);         // [64]: where each row's first frame of the call lies in the image
	int *rowFrames = reinterpret_cast<int *>(rowAt + 64);                           // [64]: the frames of it that are metered
	const int lane = threadIdx.x;
	const long long sc = (long long)blockIdx.x*64 + lane;
	const bool mine = sc < (long long)S*C;
	const int s = mine ? int(sc/C) : 0, c = mine ? int(sc%C) : 0;
	double *st = m.state + (size_t)(mine ? sc : 0)*kStreamMeterDoubles;
	const double done = st[kStreamMeterAt];
	const int n = mine ? streamMeterFrames(m.config[s], done, counts[s]) : 0;
	rowAt[lane] = (long long)s*imageStreamStride + (long long)c*imageChannelStride + (starts ? starts[s] : 0);
	rowFrames[lane] = n;
	__syncthreads();
	int most = 0;
	for (int r = 0; r < 64; ++r) most = max(most, rowFrames[r]);
	if (most == 0) return; // (uniform: every lane has the same value)
	const StreamMeterConfig &cfg = m.config[s];
	const LoudCoef coef = cfg.k;
	const int h = cfg.h;
	LoudState xr{st[4], st[5], st[6], st[7]}, xz{st[8], st[9], st[10], st[11]};
	double xin[4] = {st[0], st[1], st[2], st[3]}, e0 = st[12], e1 = st[13], sub = st[14];
	double *history = m.sub + (size_t)(mine ? sc : 0)*m.maxSub;
	const float *own = rows + lane*kLoudPitch;
	for (int t0 = 0; t0 < most; t0 += kLoudTile) {
		for (int it = 0; it < kLoudTile; ++it) {
			const int idx = it*64 + lane, r = idx/kLoudTile, i = idx%kLoudTile;
			if (t0 + i < rowFrames[r]) rows[r*kLoudPitch + i] = image[rowAt[r] + t0 + i];
		}
		__syncthreads();
		const int cnt = min(max(n - t0, 0), kLoudTile);
		const long long p0 = (long long)done + t0; // the position of the tile's first frame in the programme
		for (int i = 0; i < cnt; ) {
			const long long p = p0 + i, chunk0 = p/kLoudChunk*kLoudChunk, chunkEnd = chunk0 + kLoudChunk;
			const long long split = (chunk0/h + 1)*h;               // the first position of the second sub-block the chunk reaches
			const bool first = p < split;
			const long long stop = min(min(p0 + cnt, chunkEnd), first ? split : chunkEnd);
			const int to = int(stop - p0);
			// (the two runs in loops of their own, each the loop of a kLoudChunks pass: the compiler orders the operands of an addition as it
			// likes, and where two NaNs of different sign meet the order decides the sign of the result)
			for (int k = i; k < to; ++k) loudStep(coef, xz, double(own[k]));
			if (first) for (; i < to; ++i) loudEnergyStep(coef, xr, double(own[i]), e0);
			else for (; i < to; ++i) loudEnergyStep(coef, xr, double(own[i]), e1);
			if (first && stop == split) { // the sub-block ends: the chunk's e0 is its last addend
				loudSumStep(sub, e0);
				history[split/h - 1] = sub;
				sub = 0.0;
			}
			if (stop == chunkEnd) {
				if (split > chunkEnd) loudSumStep(sub, e0);      // the chunk lay inside one sub-block, and did not end it
				else if (split < chunkEnd) loudSumStep(sub, e1); // it straddled two: e1 is the first addend of the second
				const double end[4] = {xz.s1, xz.s2, xz.s3, xz.s4};
				double next[4];
				loudCarryStep(cfg.Ac, xin, end, next);
				for (int k = 0; k < 4; ++k) xin[k] = next[k];
				xr = LoudState{xin[0], xin[1], xin[2], xin[3]};
				xz = LoudState{0.0, 0.0, 0.0, 0.0};
				e0 = e1 = 0.0;
			}
		}
		__syncthreads(); // (the next tile goes into the same rows)
	}
	if (n < 1) return;
	st[0] = xin[0]; st[1] = xin[1]; st[2] = xin[2]; st[3] = xin[3];
	st[4] = xr.s1; st[5] = xr.s2; st[6] = xr.s3; st[7] = xr.s4;
	st[8] = xz.s1; st[9] = xz.s2; st[10] = xz.s3; st[11] = xz.s4;
	st[12] = e0; st[13] = e1; st[14] = sub;
	st[kStreamMeterAt] = done + double(n);
	// the last 11 frames of [the carried ones, the call's]
	float *line = m.frames + (size_t)sc*kStreamMeterLine;
	const float *row = image + rowAt[lane];
	float keep[kStreamMeterLine];
	for (int i = 0; i < kStreamMeterLine; ++i) keep[i] = (long long)i + n < kStreamMeterLine ? line[i + n] : row[(long long)i + n - kStreamMeterLine];
	for (int i = 0; i < kStreamMeterLine; ++i) line[i] = keep[i];
}

// ---- the chunk-scan form: a long call's chunks side by side, the clip meter's three passes with a start position and a carried state ----
// The chunks of a call that meters n frames from position `done` on: chunk i of the call is chunk done/kLoudChunk + i of the programme, cut
// to [done, done + n) -- the first one may be under way, the last one may stay incomplete
struct StreamMeterSpan {
	long long done, end; // the call's positions [done, end)
	long long first;     // the programme's chunk that holds `done`
	int chunks;          // chunks the call touches
	__device__ long long from(int i) const { return max((first + i)*kLoudChunk, done); }
	__device__ long long to(int i) const { return min((first + i + 1)*kLoudChunk, end); }
	__device__ bool closes(int i) const { return (first + i + 1)*kLoudChunk <= end; }
};
__device__ inline StreamMeterSpan streamMeterSpan(double done, int n) {
	StreamMeterSpan a;
	a.done = (long long)done; a.end = a.done + n;
	a.first = a.done/kLoudChunk;
	a.chunks = int((a.end - 1)/kLoudChunk - a.first) + 1;
	return a;
}
// the scratch of (stream, channel) number sc: per chunk of the call its end from zero state (then its incoming state), 4 doubles, and its
// two partial sums; then the state in which the energy pass left the last chunk
__device__ inline double *streamMeterEnds(const PcmStreamMeter &m, size_t sc) { return m.scan + sc*((size_t)m.maxChunks*6 + 4); }
__device__ inline double *streamMeterPartials(const PcmStreamMeter &m, size_t sc) { return streamMeterEnds(m, sc) + (size_t)m.maxChunks*4; }
__device__ inline double *streamMeterLast(const PcmStreamMeter &m, size_t sc) { return streamMeterEnds(m, sc) + (size_t)m.maxChunks*6; }

// kLoudChunks' two passes over the call's chunks: grid (tiles of 64 chunks, C, S), 64 threads; LDS: 64 rows of kLoudPitch floats.  Lane l of
// workgroup x has chunk x*64 + l of the call.  Energy false: from zero state -- the first chunk resumes the carried zero-state run -- to the
// chunk's end state.  Energy true: from the chunk's incoming state, which kPcmStreamMeterCarry left in the place of its end -- the first
// chunk resumes the carried run and its two sums -- to the chunk's two partial sums
template <bool Energy> __global__ __launch_bounds__(64) void kPcmStreamMeterChunks(const float *__restrict__ image, long long imageStreamStride, long long imageChannelStride,
		const int *__restrict__ counts, const int *__restrict__ starts, PcmStreamMeter m) {
	extern __shared__ __attribute__((aligned(16))) unsigned char smemRaw[];
	float *rows = reinterpret_cast<float *>(smemRaw); // [64][kLoudPitch]
	const int s = blockIdx.z, c = blockIdx.y, C = gridDim.y, lane = threadIdx.x;
	const size_t sc = (size_t)s*C + c;
	const double *st = m.state + sc*kStreamMeterDoubles;
	const StreamMeterConfig &cfg = m.config[s];
	const int n = streamMeterFrames(cfg, st[kStreamMeterAt], counts[s]);
	if (n < 1) return;
	const StreamMeterSpan span = streamMeterSpan(st[kStreamMeterAt], n);
	const int iWave = int(blockIdx.x)*64, i = iWave + lane;
	if (iWave >= span.chunks) return;
	const bool mine = i < span.chunks;
	const LoudCoef coef = cfg.k;
	const int h = cfg.h;
	double *ends = streamMeterEnds(m, sc), *partials = streamMeterPartials(m, sc);
	LoudState x{0.0, 0.0, 0.0, 0.0};
	double e0 = 0.0, e1 = 0.0;
	if (mine) {
		if constexpr (Energy) {
			if (i == 0) { x = LoudState{st[4], st[5], st[6], st[7]}; e0 = st[12]; e1 = st[13]; }
			else x = LoudState{ends[4*(size_t)i], ends[4*(size_t)i + 1], ends[4*(size_t)i + 2], ends[4*(size_t)i + 3]};
		} else if (i == 0) {
			x = LoudState{st[8], st[9], st[10], st[11]};
		}
	}
	const long long from = mine ? span.from(i) : 0, split = mine ? ((span.first + i)*kLoudChunk/h + 1)*h : 0;
	const int len = mine ? int(span.to(i) - from) : 0;
	const float *row = image + (size_t)s*imageStreamStride + (size_t)c*imageChannelStride + (starts ? starts[s] : 0);
	const float *own = rows + lane*kLoudPitch;
	for (int t0 = 0; t0 < kLoudChunk; t0 += kLoudTile) {
		for (int it = 0; it < kLoudTile; ++it) {
			const int idx = it*64 + lane, r = idx/kLoudTile, k = idx%kLoudTile;
			if (iWave + r >= span.chunks) continue;
			const long long a = span.from(iWave + r) + t0 + k;  // (row r's chunk, its float k of this tile)
			if (a < span.to(iWave + r)) rows[r*kLoudPitch + k] = row[a - span.done];
		}
		__syncthreads();
		const int cnt = min(max(len - t0, 0), kLoudTile);
		if constexpr (Energy) {
			const int first = int(min(max(split - (from + t0), 0ll), (long long)cnt)); // samples of the tile in the chunk's first sub-block
			for (int k = 0; k < first; ++k) loudEnergyStep(coef, x, double(own[k]), e0);
			for (int k = first; k < cnt; ++k) loudEnergyStep(coef, x, double(own[k]), e1);
		} else {
			for (int k = 0; k < cnt; ++k) loudStep(coef, x, double(own[k]));
		}
		__syncthreads(); // (the next tile goes into the same rows)
	}
	if (!mine) return;
	if constexpr (Energy) {
		partials[2*(size_t)i] = e0; partials[2*(size_t)i + 1] = e1;
		if (i == span.chunks - 1) { double *last = streamMeterLast(m, sc); last[0] = x.s1; last[1] = x.s2; last[2] = x.s3; last[3] = x.s4; }
	} else {
		ends[4*(size_t)i] = x.s1; ends[4*(size_t)i + 1] = x.s2; ends[4*(size_t)i + 2] = x.s3; ends[4*(size_t)i + 3] = x.s4;
	}
}

// kLoudCarry's chain from the carried x_in: ends[i] := the incoming state of chunk i of the call; the carried x_in and zero-state run become
// those of the chunk that is under way behind the call.  One lane per (stream, channel): grid (ceil(S*C/64)), 64 threads
__global__ __launch_bounds__(64) void kPcmStreamMeterCarry(const int *__restrict__ counts, int S, int C, PcmStreamMeter m) {
	const long long sc = (long long)blockIdx.x*64 + threadIdx.x;
	if (sc >= (long long)S*C) return;
	const int s = int(sc/C);
	double *st = m.state + (size_t)sc*kStreamMeterDoubles;
	const StreamMeterConfig &cfg = m.config[s];
	const int n = streamMeterFrames(cfg, st[kStreamMeterAt], counts[s]);
	if (n < 1) return;
	const StreamMeterSpan span = streamMeterSpan(st[kStreamMeterAt], n);
	double A[16];
	for (int i = 0; i < 16; ++i) A[i] = cfg.Ac[i];
	double *ends = streamMeterEnds(m, (size_t)sc);
	double x[4] = {st[0], st[1], st[2], st[3]}, end[4] = {0.0, 0.0, 0.0, 0.0};
	for (int i = 0; i < span.chunks; ++i) {
		double *at = ends + 4*(size_t)i;
		for (int k = 0; k < 4; ++k) { end[k] = at[k]; at[k] = x[k]; }
		if (!span.closes(i)) break; // (the last chunk stays under way: x is its incoming state, end its zero-state run)
		double next[4];
		loudCarryStep(A, x, end, next);
		for (int k = 0; k < 4; ++k) { x[k] = next[k]; end[k] = 0.0; }
	}
	for (int k = 0; k < 4; ++k) { st[k] = x[k]; st[8 + k] = end[k]; }
}

// The sub-block sums that close in the call, in chunk order from the carried running sum -- kLoudGate's first stage, one addend at a time --,
// and the rest of the carried state: the run, the two sums, the running sum, the position, the last 11 frames.  One lane per (stream, channel)
__global__ __launch_bounds__(64) void kPcmStreamMeterClose(const float *__restrict__ image, long long imageStreamStride, long long imageChannelStride, const int *__restrict__ counts,
		const int *__restrict__ starts, int S, int C, PcmStreamMeter m) {
	const long long sc = (long long)blockIdx.x*64 + threadIdx.x;
	if (sc >= (long long)S*C) return;
	const int s = int(sc/C), c = int(sc%C);
	double *st = m.state + (size_t)sc*kStreamMeterDoubles;
	const StreamMeterConfig &cfg = m.config[s];
	const int n = streamMeterFrames(cfg, st[kStreamMeterAt], counts[s]);
	if (n < 1) return;
	const StreamMeterSpan span = streamMeterSpan(st[kStreamMeterAt], n);
	const int h = cfg.h;
	const double *partials = streamMeterPartials(m, (size_t)sc);
	double *history = m.sub + (size_t)sc*m.maxSub;
	double sub = st[14], e0 = 0.0, e1 = 0.0;
	for (int i = 0; i < span.chunks; ++i) {
		e0 = partials[2*(size_t)i]; e1 = partials[2*(size_t)i + 1];
		const long long chunkEnd = (span.first + i + 1)*kLoudChunk, split = ((span.first + i)*kLoudChunk/h + 1)*h;
		if (span.done < split && split <= min(span.end, chunkEnd)) { // the sub-block ends in this call: the chunk's e0 is its last addend
			loudSumStep(sub, e0);
			history[split/h - 1] = sub;
			sub = 0.0;
		}
		if (span.closes(i)) {
			if (split > chunkEnd) loudSumStep(sub, e0);
			else if (split < chunkEnd) loudSumStep(sub, e1);
			e0 = e1 = 0.0;
		}
	}
	if (span.closes(span.chunks - 1)) {
		for (int k = 0; k < 4; ++k) st[4 + k] = st[k]; // (the next chunk's run begins at its x_in, which kPcmStreamMeterCarry left)
	} else {
		const double *last = streamMeterLast(m, (size_t)sc);
		for (int k = 0; k < 4; ++k) st[4 + k] = last[k];
	}
	st[12] = e0; st[13] = e1; st[14] = sub;
	st[kStreamMeterAt] = double(span.end);
	float *line = m.frames + (size_t)sc*kStreamMeterLine;
	const float *row = image + (size_t)s*imageStreamStride + (size_t)c*imageChannelStride + (starts ? starts[s] : 0);
	float keep[kStreamMeterLine];
	for (int i = 0; i < kStreamMeterLine; ++i) keep[i] = (long long)i + n < kStreamMeterLine ? line[i + n] : row[(long long)i + n - kStreamMeterLine];
	for (int i = 0; i < kStreamMeterLine; ++i) line[i] = keep[i];
}

// grid (S or 1), 64 threads: the stream's (-1: every stream's) meter as the setter leaves it -- the configuration, nothing metered
__global__ __launch_bounds__(64) void kPcmStreamMeterClear(PcmStreamMeter m, int S, int C, int stream, StreamMeterConfig cfg, int setConfig) {
	const int s = stream < 0 ? int(blockIdx.x) : stream, tid = threadIdx.x;
	if (tid == 0) {
		if (setConfig) m.config[s] = cfg;
		m.words[s] = 0; m.words[S + s] = 0;
	}
	for (int i = tid; i < C*kStreamMeterDoubles; i += 64) m.state[(size_t)s*C*kStreamMeterDoubles + i] = 0.0;
	for (int i = tid; i < C*kStreamMeterLine; i += 64) m.frames[(size_t)s*C*kStreamMeterLine + i] = 0.0f;
}

// grid (S), 64 threads: a reading's words -- out.peaks[s] = max(running, the six windows against zeros), out.peaks[S + s] = the sample peak --
// and the newest block powers, out.newest[2s] = z[nb - 1], [2s + 1] = st[ns - 1] (0.0 where there is none)
__global__ __launch_bounds__(64) void kPcmStreamMeterRead(const ClipSeg *__restrict__ segs, const LoudEntry *__restrict__ loud, int S, int C, TruePeakTable taps, PcmStreamMeter m,
		LoudScratch w, LoudRangeScratch r, StreamMeterReading out) {
	const int s = blockIdx.x, tid = threadIdx.x;
	unsigned most = 0u;
	if (m.config[s].on) {
		for (int idx = tid; idx < C*kTruePeakTrail; idx += 64) {
			const int c = idx/kTruePeakTrail, i = idx%kTruePeakTrail; // the window of frame Tm - 6 + i: its taps begin at carried frame i
			const long long q = (long long)m.state[((size_t)s*C + c)*kStreamMeterDoubles + kStreamMeterAt] - kTruePeakTrail + i;
			if (q < 0) continue;
			const float *line = m.frames + ((size_t)s*C + c)*kStreamMeterLine;
			float at[kTruePeakTaps];
#pragma unroll
			for (int j = 0; j < kTruePeakTaps; ++j) at[j] = i + j < kStreamMeterLine ? line[i + j] : 0.0f;
			unsigned bits[1];
			truePeakFrameBits<1>(at, taps, bits);
			most = max(most, bits[0]);
		}
	}
	int b = int(most);
	for (int k = 32; k; k >>= 1) b = max(b, __shfl(b, tid ^ k));
	if (tid) return;
	out.peaks[s] = max(b, m.words[s]);
	out.peaks[S + s] = m.words[S + s];
	const int h = loud[s].h, N = max(segs[2*s].count, 0);
	const int nSub = (h > 0 && N/4 >= h) ? N/h : 0, nb = nSub ? nSub - 3 : 0, ns = nSub >= kLoudRangeWindow ? nSub - (kLoudRangeWindow - 1) : 0;
	out.newest[2*s] = nb ? w.z[(size_t)s*w.maxSub + nb - 1] : 0.0;
	out.newest[2*s + 1] = ns ? r.st[(size_t)s*r.maxSt + ns - 1] : 0.0;
}

void launchPcmStreamMeterClear(const PcmStreamMeter &m, int S, int C, int stream, const StreamMeterConfig *cfg, hipStream_t st) {
	hipLaunchKernelGGL(kPcmStreamMeterClear, dim3(stream < 0 ? S : 1), dim3(64), 0, st, m, S, C, stream, cfg ? *cfg : StreamMeterConfig{}, cfg ? 1 : 0);
}

void launchPcmStreamMeter(const float *image, long long imageSS, long long imageCS, const int *counts, const int *starts, int S, int C, int maxFrames, const PcmStreamMeter &m, int form, hipStream_t st) {
	if (maxFrames < 1) return;
	const bool scan = streamMeterScans(maxFrames, form);
	if (scan && (!m.scan || m.maxChunks < streamMeterChunksOf(maxFrames))) throw std::invalid_argument("the stream meter's chunk-scan form needs its scratch");
	hipLaunchKernelGGL(kPcmStreamMeterPeak, dim3(divUp(maxFrames, 256), C, S), dim3(256), 0, st, image, imageSS, imageCS, counts, starts, S, truePeakTable(), m);
	if (scan) {
		const dim3 grid(divUp(streamMeterChunksOf(maxFrames), 64), C, S), lanes(divUp(S*C, 64));
		const size_t lds = size_t(64)*kLoudPitch*sizeof(float);
		hipLaunchKernelGGL(kPcmStreamMeterChunks<false>, grid, dim3(64), lds, st, image, imageSS, imageCS, counts, starts, m);
		hipLaunchKernelGGL(kPcmStreamMeterCarry, lanes, dim3(64), 0, st, counts, S, C, m);
		hipLaunchKernelGGL(kPcmStreamMeterChunks<true>, grid, dim3(64), lds, st, image, imageSS, imageCS, counts, starts, m);
		hipLaunchKernelGGL(kPcmStreamMeterClose, lanes, dim3(64), 0, st, image, imageSS, imageCS, counts, starts, S, C, m);
		countLaunch(LK_PCM_STREAM_METER_SCAN);
	} else {
		hipLaunchKernelGGL(kPcmStreamMeter, dim3(divUp(S*C, 64)), dim3(64), streamMeterLdsBytes(), st, image, imageSS, imageCS, counts, starts, S, C, m);
	}
	countLaunch(LK_PCM_STREAM_METER);
}

void launchPcmStreamMeterRead(const ClipSeg *segs, const LoudEntry *loud, const float *weights, int S, int C, const PcmStreamMeter &m, const LoudScratch &w, const LoudRangeScratch &r,
                              const StreamMeterReading &out, hipStream_t st) {
	hipLaunchKernelGGL(kLoudGate<false>, dim3(S), dim3(256), 256*sizeof(double), st, segs, loud, weights, C, w);
	hipLaunchKernelGGL(kLoudRange, dim3(S), dim3(kLoudRangeThreads), loudRangeLdsBytes(), st, segs, loud, weights, C, w, r);
	hipLaunchKernelGGL(kPcmStreamMeterRead, dim3(S), dim3(64), 0, st, segs, loud, S, C, truePeakTable(), m, w, r, out);
	countLaunch(LK_PCM_STREAM_METER_READ);
}

} // namespace smst
