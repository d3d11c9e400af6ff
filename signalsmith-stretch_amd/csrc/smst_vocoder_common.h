// Shared by the two translation units of the fused mono / stereo recurrence (smst_vocoder.hip: the tile form and its launchers;
// smst_vocoder_cont.hip: the continuous wavefront across the tiles of a call): the geometry of the line-aligned producers' LDS
// buffers, the ring constants, the plain-tile record from operands parked in LDS (plainRecord), the eight steps of a block of the
// register-history wavefront (wavefrontBlock).
#pragma once
#include "smst_recurrence.h"

namespace smst {

template <int CH, int L>
struct AlignGeom {
	static constexpr int RING = 32;                   // bins per (row, array): two lines
	static constexpr int ROWLEN = 2*CH*RING;          // float2 per row: CH input buffers, then CH previous-input buffers
	static constexpr int XLEN = CH*16;                // the row above the wave's first row: 16 bins per channel
	static constexpr int PER_PRODUCER = 8*ROWLEN + XLEN;
	static constexpr int LOADS = CH;                  // (4 rows x 2*CH arrays x 8 pieces) / 64 lanes
};

constexpr int kVocBlockSteps = 8, kVocBlocks = 3, kVocBlocksStaged = 2, kVocStagedProducers = 8, kVocOutBlocks = 4; // (kVocWaves: smst_recurrence.h)
constexpr int kVocOutBlocksAligned = 3; // lag 8: a row's 16-bin line lies in exactly two result blocks
// results ring: [block][step][channel][kVocOutPitch] -- 66, not 64: the writer reads a row's values of steps 2 apart in adjacent
// lane groups, and 2*CH*64 float2 is a multiple of the 32 banks (an 8-way conflict on every writer read with the first layout)
constexpr int kVocOutPitch = 66;

// The INTERIOR blocks of a line-aligned producer wave (vocoderProduceAligned has the derivation): blocks mw = n - 8*it, counted from the wave's first
// row, in [kVocInteriorFirst, vocInteriorLast(M)].  The launcher evaluates the same rule for its counter.
constexpr int kVocInteriorFirst = 8;
__host__ __device__ inline int vocInteriorLast(int M) { return (M >> 3) - 5; }

__device__ __forceinline__ float2 selectPair(bool pick, float2 a, float2 b) { return make_float2(pick ? a.x : b.x, pick ? a.y : b.y); }
__device__ __forceinline__ float2 fromLaneBelow(float2 v, float2 lane0) { // lane k receives lane k-1's v; lane 0 keeps its `lane0`
	// DPP wave_shr:1 without bound_ctrl: a lane with no source lane keeps the old value of the destination register
	return make_float2(__int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(lane0.x), __float_as_int(v.x), 0x138, 0xf, 0xf, false)),
	                   __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(lane0.y), __float_as_int(v.y), 0x138, 0xf, 0xf, false)));
}

// ------------------------------------------------------------------------------------------------------
// The record of a PLAIN tile (identity map, no random time factors) whose operands a producer has parked in LDS: the same operands and the
// same operations in the same order as computeRecord<CH, true, ...> (smst_recurrence.h, whose operands come from memory with a load
// schedule of their own) -- bit-identical records; the parity tests compare the forms.  `View` says where the operands lie, relative to
// the record's bin b:
//   in(c, off), prev(c, off)   Band.input / Band.prevInput of channel c at bin b + off
//   rot(off)                   hop rotation factor of bin b + off (off = 1, L: the two previous-hop twists)
//   above(c, off)              the row above (the hop before) at bin b + off: its input, or -- aboveIsEnergy() -- (Prediction.energy, -) of the carried state
// StageView (smst_vocoder.hip) reads StageGeom windows, AlignView the line buffers of AlignGeom.
// FOLD (FOLD0, see computeRecord): the record of the tile's first hop carries  Cc := prevOut[b+1]*Cc + prevOut[b+L]*Dc, Dc := 0  with the
// carried Band.output taps car1 / carL per channel; foldWave: this wave owns that row (uniform: the others skip the arithmetic),
// foldLane: this lane's record is in it.
// TWISTED (kVocoder ALIGNED on a twisted tile): prev(c, off) is not Band.prevInput but the finished twist of bin b + off
// (prevHopTwist, formed by the analysis pass); rot() and `rotate` are then unused.
// INTERIOR (the line-aligned producers' interior blocks): the caller guarantees L <= b < M - L, so the clamp of b + off and the four zeroings at the
// spectrum's edges cannot act and are left out; every floating-point operation and its order stay.
// ------------------------------------------------------------------------------------------------------
template <int CH, int L, bool FOLD, bool TWISTED = false, bool INTERIOR = false, typename View, int NFLOATS>
__device__ __forceinline__ void plainRecord(const View &v, int b, int M, float tf, bool rotate, bool foldWave, bool foldLane,
                                            const float2 (&car1)[CH], const float2 (&carL)[CH], float (&f)[NFLOATS]) {
	auto lerpIN = [&](int c, LerpIndex li) { // li.lo is an absolute bin
		const float2 low = v.in(c, li.lo - b), high = v.in(c, li.lo - b + 1);
		return clerp(low, high, li.fr);
	};
	float2 p[CH];
	float e[CH];
#pragma unroll
	for (int c = 0; c < CH; ++c) { p[c] = v.in(c, 0); e[c] = cnorm(p[c]); }
	int mc = 0; // maximum-energy channel, first maximum wins (:729-737)
	float eMax = e[0];
#pragma unroll
	for (int c = 1; c < CH; ++c) if (e[c] > eMax) { mc = c; eMax = e[c]; }
	float2 Pm = p[0];
#pragma unroll
	for (int c = 1; c < CH; ++c) if (c == mc) Pm = p[c];
	const float fb = float(b);
	float2 A = cmulc(Pm, lerpIN(mc, lerpIndex(fb - tf)));
	float2 B = cmulc(Pm, lerpIN(mc, lerpIndex(fb - L*tf)));
	auto twist = [&](int off, float stepMul) { // the coefficient of the previous hop's output at bin b + off
		const int bc = INTERIOR ? b + off : min(b + off, M - 1);
		const float2 Px = v.in(mc, off);
		float2 TW;
		if constexpr (TWISTED) TW = v.prev(mc, off); // the analysis pass has formed it
		else TW = prevHopTwist(Px, v.prev(mc, off), rotate ? v.rot(off) : make_float2(1.f, 0.f));
		const float eNow = cnorm(Px);
		const float2 up = v.above(mc, off);
		const float ePrev = v.aboveIsEnergy() ? up.x : cnorm(up); // Prediction.energy of the previous hop
		const float den = fmaxf(ePrev, eNow) + 1e-15f;
		const float2 down = cmulc(Px, lerpIN(mc, lerpIndex(float(bc) - stepMul*tf)));
		const float2 rr = cmulc(TW, down);
		const float inv = __builtin_amdgcn_rcpf(den); // 1-ulp hardware reciprocal, as twistFinish
		return make_float2(rr.x*inv, rr.y*inv);
	};
	float2 Cc = twist(1, 1.0f), Dc = twist(L, float(L));
	const float2 zero = make_float2(0.f, 0.f);
	if constexpr (!INTERIOR) {
		if (!(b > 0)) A = zero;
		if (!(b >= L)) B = zero;
		if (!(b < M - 1)) Cc = zero;
		if (!(b < M - L)) Dc = zero;
	}
	if constexpr (FOLD) {
		if (foldWave) {
			float2 c1 = car1[0], cL = carL[0];
#pragma unroll
			for (int c = 1; c < CH; ++c) if (c == mc) { c1 = car1[c]; cL = carL[c]; }
			const float2 K = prevHopTerms(c1, Cc, cL, Dc);
			if (foldLane) { Cc = K; Dc = zero; }
		}
	}
	f[0] = A.x; f[1] = A.y; f[2] = B.x; f[3] = B.y; f[4] = Cc.x; f[5] = Cc.y; f[6] = Dc.x; f[7] = Dc.y;
	f[8] = __int_as_float(mc);
	recordChannelFields<CH>(f, p, e, mc);
}

// Operands in the line buffers of the line-aligned producers (kVocoder ALIGNED, kVocoderCont), for the lane of local row r and step st.  The
// row's buffer holds the lines (j-1, j) in its even blocks (b0 = 16j) and (j, j+1) in its odd ones, so bin b sits at 16 + st resp. 8 + st;
// the row above runs 8 bins ahead (opposite parity): its buffer holds (j, j+1) either way, bin b at st resp. 8 + st.  Above the wave's first
// row: the 16 bins staged in xbuf, which start at b0.  The rotation factors of the lane's two previous-hop bins travel in registers.
template <int CH, int L>
struct AlignView {
	using G = AlignGeom<CH, L>;
	const float2 *mine, *up; // bin b of channel 0: this row's input, the row above
	int upPitch;             // channel pitch of `up`
	bool upIsEnergy;
	float2 rot1, rotL;
	__device__ __forceinline__ AlignView(const float2 *sbuf, const float2 *xbuf, int r, int st, bool odd, bool upIsEnergy_, float2 rot1_, float2 rotL_)
		: mine(sbuf + r*G::ROWLEN + (odd ? 8 : 16) + st), up((r > 0) ? sbuf + (r - 1)*G::ROWLEN + (odd ? 8 : 0) + st : xbuf + st),
		  upPitch((r > 0) ? G::RING : 16), upIsEnergy(upIsEnergy_), rot1(rot1_), rotL(rotL_) {}
	__device__ __forceinline__ float2 in(int c, int off) const { return mine[c*G::RING + off]; }
	__device__ __forceinline__ float2 prev(int c, int off) const { return mine[(CH + c)*G::RING + off]; }
	__device__ __forceinline__ float2 rot(int off) const { return off == 1 ? rot1 : rotL; }
	__device__ __forceinline__ float2 above(int c, int off) const { return up[c*upPitch + off]; }
	__device__ __forceinline__ bool aboveIsEnergy() const { return upIsEnergy; }
};

// ------------------------------------------------------------------------------------------------------
// The eight steps of one block of the register-history wavefront (the recurrence wave of kVocoder and kVocoderCont).  Lane k holds its last
// 8 outputs per channel in h[step & 7], so its own taps out[b-1], out[b-L] are h[(i+7)&7], h[(i+8-L)&7], and the previous hop's taps are
// registers of lane k-1 (it runs LAG bins ahead), fetched with one DPP wave_shr:1 each into tap1 / tapL -- whose lane-0 values nothing
// overwrites: the constants (1, 0) and (0, 0) that FOLD0 records expect.  ACROSS: every lane is a first hop, no lane reads another one's.
// blockRecs: the block's records; blockOut: its place in the result ring, this lane's column.  The records of step i+1 are read during step
// i into the other of two register sets; in the last step, where there is nothing to read ahead, peekNext() looks at the hand-off words
// the NEXT block waits for (an LDS round trip each, 200 clock cycles, sat on the serial path at every block boundary -- cycle trace).
// ------------------------------------------------------------------------------------------------------
template <int CH, int L, int LAG, bool ACROSS, int NCH, typename PeekNext>
__device__ __forceinline__ void wavefrontBlock(const float4 *blockRecs, float2 *blockOut, int k, float2 (&h)[8][CH], float2 (&tap1)[CH], float2 (&tapL)[CH],
                                               bool onlyAcknowledge, PeekNext peekNext) {
	constexpr int BS = kVocBlockSteps;
	float4 q[2][NCH]; // two register sets alternate, so the next step's record loads never overwrite live values
#pragma unroll
	for (int j = 0; j < NCH; ++j) q[0][j] = blockRecs[j*64 + k];
#pragma unroll
	for (int i = 0; i < BS; ++i) {
		if (onlyAcknowledge) break; // experiment builds only
		if (i + 1 < BS) {
#pragma unroll
			for (int j = 0; j < NCH; ++j) q[(i + 1) & 1][j] = blockRecs[((i + 1)*NCH + j)*64 + ((k + (i + 1)) & 63)];
		} else {
			peekNext();
		}
		float f[NCH*4];
		unpackRecord(q[i & 1], f);
		// (not recordMaxChannel: records of 1 or 2 channels carry the bare index, and every record of the ring was written by a producer -- all-zero outside the tile)
		const int mc = __float_as_int(f[8]);
		if constexpr (!ACROSS) {
#pragma unroll
			for (int c = 0; c < CH; ++c) { // lane k-1 finished its bin b+x (x = 1, L) LAG - x steps ago
				tap1[c] = fromLaneBelow(h[(i + 17 - LAG) & 7][c], tap1[c]);
				tapL[c] = fromLaneBelow(h[(i + 16 + L - LAG) & 7][c], tapL[c]);
			}
		}
		// the maximum channel's taps: explicit per-component selects (v_cndmask) -- written as an `if` the compiler makes a branch of
		// it, with a register copy in front of every tap that must survive (14 moves against 8 selects)
		float2 o1 = h[(i + 7) & 7][0], oL = h[(i + 8 - L) & 7][0], p1 = tap1[0], pL = tapL[0];
#pragma unroll
		for (int c = 1; c < CH; ++c) {
			const bool pick = c == mc;
			o1 = selectPair(pick, h[(i + 7) & 7][c], o1);
			oL = selectPair(pick, h[(i + 8 - L) & 7][c], oL);
			p1 = selectPair(pick, tap1[c], p1);
			pL = selectPair(pick, tapL[c], pL);
		}
		float2 out[CH];
		recurrenceOutputs<CH>(f, mc, o1, oL, p1, pL, out);
#pragma unroll
		for (int c = 0; c < CH; ++c) {
			h[i][c] = out[c];
			blockOut[(i*CH + c)*kVocOutPitch] = out[c];
		}
	}
}

} // namespace smst
