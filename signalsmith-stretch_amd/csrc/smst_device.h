// Device-side view of a batch (plain pointers, passed to kernels by value) and the kernel launchers.
#pragma once
#include <hip/hip_runtime.h>
#include "smst_types.h"

namespace smst {

struct DevBatch {
	// geometry (signalsmith-stretch.h:71-94; fftSamples/bands from the L1 contract)
	int S, C, B, I, M, N, L, T;
	int Mp;                       // row pitch (elements) of the per-tile [.][C][M] arrays: M + 32 rounded up to 16
	int recPitch;                 // float4 per wavefront step in REC: chunks*64 + 16
	int histLen, carryLen, delta; // B+I, B+I, split ? I : 0
	int carryPitch;               // B+I + 2*I: behind the window the rows hold what an empty ring position holds (sum 0, product 1e-30) -- written once, by kResetStreams
	int histPitch;                // 2*(B+I): a call's input is appended behind the window until the row is full, then the window moves back to the front
	int lag, ringSlots;           // wavefront skew (>= L+1) and LDS ring depth (power of two > lag)
	int recSteps;                 // record rows per stream: M + lag*(T-1) rounded up to 64, plus prefetch slack
	int hopStride, emitStride;    // row pitch of the per-call hop / emit tables
	int mapTableLen;
	int histCur, carryCur;        // which half of the double buffers is current
	int debugMode;                // always 0 in the product; builds with -DSMST_EXPERIMENTS read SMST_DEBUG_MODE (timing experiments)
	int noFeedFusion;             // SMST_NO_FEED_FUSION=1: pass A stays its own kernel (kPredictA) -- cross-check of the folded forms; =2: formant tiles in two passes over the spectra
	                              // (kFeedScanA + kFeedFreq + kFeedScanC with pass A folded) even where the one-pass form applies
	int feedSerial;               // SMST_FEED_SERIAL: bin-by-bin feed recurrences (kFeedSerial) instead of the scan form
	int halfState;                // carried Band.output / Prediction.energy / overlap-add sums stored in fp16 (BASELINE config 5 "fp16 internal")
	int fftLean;                  // SMST_FFT_TABLES=lean: register-blocked FFT kernels with the smaller tables (opt-in experiment, see smst_engine.cpp)
	int noFastFft;                // SMST_NO_FAST_FFT: the generic radix-4/2/3/5 ladder even where a register-blocked FFT exists (cross-check)
	int fftTeams;                 // analysis / synthesis by persistent workgroups of three free-running teams, tables in LDS (default; SMST_FFT_TEAMS=0: one frame per workgroup; =2: teams even for tiles with few frames per team -- tests)
	int vocTwist;                 // tiles that qualify keep the previous-hop twist, formed by the analysis pass, in Xprev (default 1; SMST_VOC_TWIST=0: Band.prevInput, the twist per record -- the cross-check)
	int analysePairs;             // the analysis teams take two frames per pass (kAnalyseTeamPairs; default 1; SMST_ANALYSE_PAIRS=0: kAnalyseTeams, one frame per pass -- the cross-check)
	int teamsGrid;                // their grid: one workgroup per CU, a multiple of 8
	int synthEmit;                // synthesis + overlap-add + emission in one kernel (kSynthEmitTeams) where it applies (default 1; SMST_SYNTH_EMIT=0: kSynthTeams + kEmit; =2: also for small tiles -- tests)
	int vocNWide;                 // 3-8 channels: producer passes of 8 rows x 8 steps instead of 16 rows x 4 (SMST_VOCN_WIDE, smst_switches.h)
	int vocWide;                  // mono / stereo, gathering producers (mapped tiles): passes of 4 rows x 16 steps instead of 8 x 8 (SMST_VOC_WIDE=0: the first form)
	int vocNHalfLines;            // 3-8 channels: the writer wave stores aligned 64-byte half lines (1) or whole 128-byte lines (2) instead of 32-byte sectors (SMST_VOCN_HALF_LINES=0: the first form)
	int noStage;                  // SMST_NO_STAGE: producers of the fused kernel gather from HBM even where staging applies
	int alignAll;                 // SMST_ALIGN_ALL: the line-aligned producers for every geometry they are valid for (default: L = 4 only)
	int noAlign;                  // SMST_NO_ALIGN: staged producers with per-row windows and lag L+1 (round 3) instead of the line-aligned form
	FftPlan plan;
	// constant tables
	const float2 *twH;     // e^{-2 pi i j / H}
	const float2 *halfTw;  // e^{-i pi m / N}
	const float2 *rot;     // per-bin hop rotation (signalsmith-stretch.h:647-655)
	const float2 *winA, *winB; // analysis window folded with e^{-i pi m/N}: u[m] = x[m+B/2]*winA[m] + x[m-H+B/2]*winB[m]
	const float4 *win4;        // (winA[m], winB[m]) interleaved: one 16-byte load per element in the fast analysis kernel
	const float4 *synTab;      // (halfTw[m], window[m+B/2] or 0, window[m-M+B/2] or 0): one 16-byte load per synthesis output
	const float4 *twA4, *twB4; // stage twiddles of the register-blocked FFT, rows (2i, 2i+1) paired: [8][16*R3], [8][R3]
	const unsigned *lcgPow;    // 16807^(j+1) mod (2^31 - 1), j < 2M: jump-ahead factors of the reference's random engine (smst_kernels_common.h: engineDraw)
	const float4 *twA6;        // lean form of twA4: (w^1, w^2), (w^3, w^4), (w^8, w^12) per thread, [3][16*R3]
	const float2 *win2;        // lean form of win4 and of synTab: the two window samples of an element only, [M]
	const float *window;   // analysis == synthesis window (Kaiser, perfect reconstruction)
	const float *wprod;    // window[i]^2 * N
	// per-stream state
	float2 *stInput, *stPrev, *stOut; // Band.input / .prevInput / .output   [S][C][M]
	float *stEnergy;                  // Prediction.energy                   [S][C][M]
	float *hist;                      // input history, a sliding window of B+I samples per row        [S][C][histPitch]
	int *histBase[2];                 // where each stream's window begins in its rows (double-buffered with histCur: kHistory reads one, writes the other)  [S]
	float *carrySum[2];               // overlap-add partial sums: a window of B+I per row    [S][C][carryPitch]
	float *carryWp[2];                // window products                                      [S][carryPitch]
	int *carryBase[2];                // where each stream's window begins in the rows of that half: a call without a hop emits from the front of the window
	                                  // and moves its beginning on (kEmitCarried) instead of copying what is left; everything else writes a window at 0.  [S]
	float *wpHead;                    // kSynthEmitTeams: the window products of a tile's first samples (those the carry reaches into), [S][wpHeadLen], written by kEmitProducts
	int wpHeadLen;                    // (ceil(B/I) + 2)*I
	float *stFreq;                    // freqEstimateWeighted / Weight       [S][2]
	const StreamParams *params;       // [S]
	// split computation spreads a block's steps over its interval (signalsmith-stretch.h:321-325) and the steps read the LIVE parameters:
	// findPeaks (:874), updateFormants step 0 (:982-983) and step 2 (:1020-1021) of the block in flight may each see other values.  In every
	// other launch the three point at `params`.
	const StreamParams *paramsPeaks, *paramsForm0, *paramsForm2;
	const float *mapTable;            // [S][kMapSlots][mapTableLen] custom frequency maps (table form of setFreqMap; StreamParams.mapSlot selects the row)
	// per-call tables
	const HopDesc *hops;   // [S][hopStride]
	const EmitDesc *emit;  // [S][emitStride]
	// per-tile workspace, [subS][T][C][M] unless noted
	float2 *Xcur, *Xprev, *OUT;
	PredEntry *PE;  // (Prediction.input, Prediction.energy) per (hop, channel, bin), 12 bytes: [subS][T][C][Mp]
	float2 *dump;   // [subS][C][64] parking lot for the recurrence kernel's out-of-range lanes
	float4 *REC;    // skewed per-step records of the bin recurrence [subS][recSteps][chunks][64 lanes]
	float2 *map;    // [subS][T][M]
	float *ratio;   // [subS][T][M]
	float *envelope; // [subS][T][M] test hook: the formant envelope (formantMetric after its eight passes, :984-1006) of every hop -- written only by the
	                 // separate envelope kernel (SMST_NO_FEED_FUSION=1), null otherwise (smst_batch_debug_get_formants)
	float *energyT, *smoothT; // [subS][M][64 hops]: feed scratch, hop index fastest
	float2 *peaksT;           // [subS][M/2 + 2][64 hops]
	float *est;     // [subS][T][2]
	float *freqEst; // [subS][T]: pitch estimate (in bins) each hop's formant envelope uses
	float *frames;  // [subS][T][C][B]
	float2 *fftScratch; // [subS][T][C][Mp]: second FFT buffer of the synthesis frames where two buffers do not fit LDS (fftNeedsScratch); null otherwise
	const int *nHops;      // [subS] hops of this tile
	const int *lastNewHop; // [subS] tile-local index of the last hop with a new spectrum, or -1
	// (behind everything else: the fields above keep the places every other kernel reads them from)
	int vocInterior;       // the line-aligned producers run the interior form of a block between a row's edges (default 1; SMST_VOC_INTERIOR=0: the general form in every block -- the cross-check)
};

// The continuous wavefront of the fused mono / stereo recurrence (kVocoderCont, smst_vocoder_cont.hip): launch `tile` covers the global
// blocks [n0, n1) of a wavefront that runs through ALL tiles of a call without draining -- the rows (lanes) finish tile - 1 and begin
// `tile` in it.  `[0]` = the workspace of tile - 1, `[1]` = the workspace of `tile`.
struct ContArgs {
	float2 *Xcur[2], *Xprev[2], *OUT[2];
	const int *tileInfo; // [tile][2][subS]: hops per stream and tile (row 0 of each pair), as the tile kernels' DevBatch::nHops
	int tileStride;      // 2*subS
	int nTiles;          // tiles of the call
	int tile;            // the tile that BEGINS in this launch (its row 0 starts at block n0 = tile*period), counted from the wavefront's first tile
	int hopBase;         // index of that first tile's first hop in the rows of the call's hop table
	int n0, n1;          // global block range; both even
	int period;          // blocks per tile and row: M/8 + 2 (a zero line between two hops of a row: see the kernel)
	float2 *save;        // [S][8*C*64]: the recurrence wave's last eight outputs per lane, from one launch to the next
	int writerWave;      // which wave drains the results: 4 (the recurrence wave's SIMD, as in kVocoder) or 11 (the SIMD that holds two producers)
};

struct IoArgs {
	const float *in;
	float *out;
	long long inStreamStride, inChannelStride, outStreamStride, outChannelStride;
	const int *inSamples;  // [S] device
	const int *outSamples; // [S] device
};

// Moving the carried state of whole streams between two batches of one geometry (Batch::moveStreamsFrom): one segment per state
// array, rows = streams.  Pair p copies `rowBytes` from src + pairs[2p]*srcPitch to dst + pairs[2p + 1]*dstPitch.
struct MoveSeg {
	const char *src;
	char *dst;
	unsigned long long srcPitch, dstPitch; // bytes from one stream's row to the next (the two batches differ in nothing else)
	unsigned long long rowBytes;
};
constexpr int kMoveSegs = 16;
struct MoveArgs {
	MoveSeg seg[kMoveSegs];
	int nSeg, nPairs;
	const int *pairs; // [nPairs][2] device: (source stream, destination stream)
};

// The packed input of a frame: element m = (x[base + halfB + m] w[halfB + m], x[base + halfB - M + m] w[halfB - M + m]), the real part
// present for m < B - halfB, the imaginary part for m >= M - halfB.  At 48 / 96 kHz (block = 15/16 of the FFT size) those edges are
// element-slot boundaries: slot 0 has no imaginary part, slot 15 no real part, and kAnalyseTeams fetches exactly the window.  Other
// block sizes (44.1 kHz: 5292 of 6144) end inside a slot; the team kernel then still fetches WHOLE slots 0..14 / 1..15 -- up to
// `windowPad` samples on either side of the window, which the table's zero weights cancel -- so a frame is its to take only if
// that wider span lies in this call's input too.  (First form: one compare + select per element and half: analysis 4.4 -> 6.8 ms per
// step at 44.1 kHz, slower than the per-frame kernel it was to replace.)
// The generic FFT kernels ping-pong between two buffers of `bands` complex values: in LDS while both fit (150 KiB), else one of them in memory
// (kAnalyse<true> / kSynth<true>: presetDefault / presetCheaper at 176.4 / 192 kHz).  One buffer must still fit.
__host__ __device__ inline bool fftNeedsScratch(int bands) { return (size_t)bands*16 > (size_t)150*1024; }
// The register-blocked FFT's band counts, 256*R3 (smst_fft.hip)
__host__ __device__ inline bool isFastSize(int bands) { return bands == 256*10 || bands == 256*12 || bands == 256*20 || bands == 256*24; }
constexpr size_t kLdsBytesPerCU = 160*1024;
// kChain's LDS (smst_vocoder_n.hip), one array of float2: a ring [C][ringSlots][64] of the last outputs per channel and lane, then the stage [C][128].
// Its size depends on the geometry alone; a batch whose ring does not fit is refused when it is created (Batch::Batch).
constexpr size_t chainLdsBytes(int channels, int ringSlots) { return ((size_t)channels*ringSlots*64 + (size_t)channels*128)*sizeof(float2); }
constexpr int kMaxBands = 150*1024/8; // 19200 bins of LDS; the largest band count {1,2,3,4,5,6,8}*2^k reaches below it is 16384

struct WindowPad { int lo, hi; };
__host__ __device__ inline WindowPad windowPad(int B, int M) {
	const int halfB = B/2, MA = M/16;
	WindowPad p;
	p.lo = (M - halfB) - MA;          // samples in front of the window that slot 1's imaginary parts reach
	p.hi = 15*MA - (B - halfB);       // samples behind it that slot 14's real parts reach
	return p;
}
// The frames that kAnalyseTeams takes (the others reach into the carried history, or too close to the end of the input, and go to the
// per-frame kernel's bounds-checked path).  The host evaluates the same condition (smst_engine.cpp).
__host__ __device__ inline bool analysisWindowInCall(int B, int M, int I, int inputOffset, int which, int inSamples) {
	const WindowPad p = windowPad(B, M);
	const int end = inputOffset - (which ? I : 0);
	return p.lo >= 0 && p.hi >= 0 && end - B - p.lo >= 0 && end + p.hi <= inSamples;
}

// Which kernel variant a launcher chose, counted per process (test hook: smst_debug_launch_count).  "Bit-identical to the other
// form" tests assert through these that BOTH forms really ran.
enum LaunchKind {
	LK_VOC_ALIGNED, LK_VOC_TWISTED, LK_VOC_INTERIOR, LK_VOC_STAGED, LK_VOC_GATHER, LK_VOC_N, LK_VOC_ONE, LK_VOC_ACROSS, LK_VOC_CONT, LK_CHAIN_UNFUSED,
	LK_ANALYSE_TEAMS, LK_ANALYSE_PAIRS, LK_ANALYSE_TWIST, LK_TWIST_ROWS, LK_ANALYSE_FAST, LK_ANALYSE_GENERIC, LK_SYNTH_TEAMS, LK_SYNTH_FAST, LK_SYNTH_GENERIC, LK_SYNTH_EMIT, LK_EMIT_CARRIED, LK_FEED_ONE_PASS, LK_PCM_IN, LK_PCM_OUT, LK_CLIP_IN, LK_CLIP_OUT, LK_PCM_OUT_DITHERED, LK_CLIP_OUT_DITHERED, LK_PCM_OUT_LEVELLED, LK_CLIP_OUT_LEVELLED, LK_CLIP_PEAK, LK_CLIP_LOUDNESS, LK_CLIP_TRUE_PEAK, LK_CLIP_LIMIT_NEED, LK_CLIP_LIMIT_GAIN, LK_CLIP_OUT_LIMITED, LK_CLIP_LOUDNESS_RANGE, LK_CLIP_RESAMPLE, LK_PCM_LIMIT_FEED, LK_PCM_LIMIT_GAIN, LK_PCM_OUT_LIMITED, LK_PCM_STREAM_RESAMPLE, LK_PCM_STREAM_METER, LK_PCM_STREAM_METER_READ, LK_PCM_STREAM_METER_SCAN, LK_CLIP_RESAMPLE_OUT, LK_PCM_STREAM_RESAMPLE_OUT, LK_PCM_STREAM_RESAMPLE_OUT_COPY, LK_PCM_LIMIT_FEED_TRUE_PEAK, LK_COUNT
};
long long launchCount(const char *name); // -1: unknown name

void launchEnergy(const DevBatch &d, const IoArgs &io, int sBase, int nStreams, int maxSamples, float *energyOut, hipStream_t st);
// twisted: the tile's Xprev rows take the finished previous-hop twists instead of Band.prevInput (RecurrenceForm::twisted; lateHops: the tile's first hops,
// those with a window that reaches into the history -- kTwistRows turns their rows)
void launchAnalyse(const DevBatch &d, const IoArgs &io, int sBase, int nStreams, int hopBase, int tileHops, bool anyInCall, bool anyLate, hipStream_t st, bool twisted = false, int lateHops = 0);
bool analyseTwistApplies(const DevBatch &d, int nStreams, int tileHops); // the pair teams take this tile (what a twisted tile's analysis is built on)
bool launchFeed(const DevBatch &d, int sBase, int nStreams, int hopBase, int tileHops, bool anyFormants, bool anyEstimatedBase, hipStream_t st); // true: pass A done too
void launchPredict(const DevBatch &d, bool fused, int sBase, int nStreams, int hopBase, int tileHops, bool plain, bool passADone, hipStream_t st); // fused: RecurrenceForm::fused()
// (the recurrence of a tile: recurrenceForm / launchRecurrence, smst_recurrence_form.h)
int continuousPeriod(const DevBatch &d);     // blocks per tile of the continuous wavefront
void launchVocoderContinuous(const DevBatch &d, const ContArgs &a, int sBase, int nStreams, hipStream_t st);
void launchSynth(const DevBatch &d, int sBase, int nStreams, int hopBase, int tileHops, hipStream_t st);
void launchEmit(const DevBatch &d, const IoArgs &io, int sBase, int nStreams, int tileIndex, int maxSpan, hipStream_t st);
void launchEmitCarried(const DevBatch &d, const IoArgs &io, hipStream_t st); // a call without hops, every stream (emit table row 0)
// synthesis + overlap-add + emission in one kernel: whether it applies to a tile; its window products (needs nothing of the tile's
// spectra: launched ahead of the recurrence's completion); the kernel itself
bool synthEmitApplies(const DevBatch &d, int nStreams, int tileHops);
void launchEmitProducts(const DevBatch &d, int sBase, int nStreams, int tileIndex, hipStream_t st);
void launchSynthEmit(const DevBatch &d, const IoArgs &io, int sBase, int nStreams, int tileIndex, hipStream_t st);
void launchCarryFeed(const DevBatch &d, int sBase, int nStreams, int hopBase, bool anyFormants, hipStream_t st);
void launchCarryOut(const DevBatch &d, int sBase, int nStreams, hipStream_t st);
void launchHistory(const DevBatch &d, const IoArgs &io, int span, hipStream_t st);
void launchPassThrough(const DevBatch &d, const IoArgs &io, const int *passFlags, int maxOut, hipStream_t st);
// flags: per-stream bit masks or null = allBits for every stream.  keep (may be null): per stream, the first samples of the overlap-add ring that
// stft.reset() does NOT reach -- split computation reads the rest of the interval from its stashed copy of the ring (signalsmith-stretch.h:407-415)
void launchResetStreams(const DevBatch &d, const int *flags, int allBits, const float *seedWp, hipStream_t st, const int *keep = nullptr);
// split computation: the spectra of the block in flight (analysed at the block's start, :293,:356-373) -> row 0 of the tile that runs the block
void launchPendingToTile(const DevBatch &d, int sBase, int nStreams, const float2 *pendIn, const float2 *pendPrev, hipStream_t st);
// ... and a flush() that fell between two synthesis steps (:397-399): channels from synthChannels[stream] on contribute no frame (negative: all do)
void launchMaskOutRows(const DevBatch &d, int sBase, int nStreams, const int *synthChannels, hipStream_t st);
void launchSeekHistory(const DevBatch &d, const IoArgs &io, const int *seekFlags, hipStream_t st);
void launchAddPreRoll(const DevBatch &d, const float *preRoll, int length, const int *offsets, hipStream_t st);
void launchComplexSelfTest(const float *in, float *out, int n, hipStream_t st); // smst_complex.h against its documented formulas (test hook)
void launchFftComplexSelfTest(const float *in, float *out, int n, hipStream_t st); // smst_fft_complex.h likewise: [n][4] -> [n][20]
void launchFlushTail(const DevBatch &d, const IoArgs &io, const int *tailOffset, const int *outOffset, hipStream_t st);
void launchMoveStreams(const MoveArgs &a, hipStream_t st); // every segment of every pair in one launch
// Interleaved PCM frames <-> the planar fp32 image (smst_pcm.h).  format: the SMST_PCM_* codes of include/smst.h; strides in elements (packed
// int24: of 3 bytes); counts: [S] device, frames per stream; maxFrames: the largest of them (sizes the grid; nothing is launched for 0);
// overs (may be null): [S][2] device counters that the output conversion adds its clamped / NaN elements to
constexpr int kPcmTileFrames = 512; // frames one workgroup moves
constexpr int kPcmS16 = 1, kPcmF32 = 2, kPcmS24 = 4, kPcmS32 = 5, kPcmF16 = 6;
void launchPcmIn(int format, const void *in, long long inStreamStride, long long inFrameStride, float *out, long long outStreamStride, long long outChannelStride,
                 const int *counts, int S, int C, int maxFrames, hipStream_t st);
// Dither of the int16 / int24 output conversions (include/smst.h, "Dither", has the definition; all of it is wrapping 32-bit arithmetic).
// One entry per stream, device: the mode (0: none -- today's rule), the stream's hash h of its seed (pcmDitherHash, computed by the host) and
// the frame index n of the run's first frame (kPcmOut; kClipOut takes its segment's destination frame instead).  dither == null, or a
// format other than int16 / int24: the undithered kernels, as before.
struct PcmDither { unsigned mode, h, nLo, nHi; };
constexpr unsigned kPcmDitherTpdf = 1u, kPcmDitherHp = 2u;
inline __host__ __device__ unsigned pcmMix(unsigned x) { x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16; return x; }
inline unsigned pcmDitherHash(long long seed) {
	const unsigned long long d = (unsigned long long)seed;
	return pcmMix(pcmMix(unsigned(d) ^ 0x736d7374u) ^ unsigned(d >> 32));
}
// Level of the output conversions (include/smst.h, "Level", has the definition).  One entry per stream, device: the mode (kPcmLevel*), the
// gain and -- the two whole-clip modes -- the ceiling.  A launch is a levelled one when `table` is set: every element is w = v*g before the
// rule above runs on w, peaks[s] (the bits of a non-negative float, which order as ints) takes the largest |v| the launch met in stream s,
// NaN skipped, and applied[s] the gain g it used.  kPcmOut knows the fixed gain only; kClipOut derives a whole-clip gain from clipPeak[s],
// the peak of the stream's clip that kClipPeak left there.  table == null: the unlevelled kernels, as before; nothing else is read.
// flags, a bit set.  kPcmFlagTruePeak: the stream's true-peak flag (include/smst.h, "True peak") -- kClipTruePeak measures the stream, and
// kClipOut forms its whole-clip gain from truePeak[s] of the PcmLevelIo, which that pass left there, in the place of clipPeak[s].
// kPcmFlagLimiter: the stream's limiter flag (include/smst.h, "Limiter"), which acts in the PROTECT and LOUDNESS modes only (pcmLimited):
// the whole-clip gain is formed without the ceiling's quotient, and kClipOut multiplies every frame by its r of PcmLevelIo::limit as well
struct PcmLevel { unsigned mode; float gain, ceiling; unsigned flags; };
constexpr unsigned kPcmFlagTruePeak = 1u, kPcmFlagLimiter = 2u;
// kPcmFlagStreamLimiter: the stream limiter's setting (include/smst.h, "Stream limiter"), which acts in the streaming calls on a FIXED stream;
// the entry's ceiling word -- a FIXED entry has no use for it otherwise -- then holds the stream limiter's ceiling.  kPcmFlagStreamLimitSet:
// which of the stream's two carried lines the call reads (it writes the other one)
constexpr unsigned kPcmFlagStreamLimiter = 4u, kPcmFlagStreamLimitSet = 8u;
// kPcmFlagStreamLimitTruePeak: the stream limiter's true-peak flag (include/smst.h, "Stream limiter"), inert without kPcmFlagStreamLimiter:
// the detector sees the three inter-sample phases as well (kPcmLimitFeedTruePeak), and the output is 6 frames later still
constexpr unsigned kPcmFlagStreamLimitTruePeak = 16u;
// kClipOut takes the loudness mode's gain gL from loudGain[s], which kLoudGate (smst_loudness.h) left there, and limits it by ceiling/peak.
constexpr unsigned kPcmLevelFixed = 0u, kPcmLevelProtect = 1u, kPcmLevelNormalise = 2u, kPcmLevelLoudness = 3u;
struct PcmLevelIo { const PcmLevel *table = nullptr; int *peaks = nullptr; float *applied = nullptr; int *clipPeak = nullptr; const float *loudGain = nullptr;
	const int *truePeak = nullptr;   // (null: no stream of the call was measured -- every stream's gain comes from its clip peak)
	const float *limit = nullptr; long long limitPitch = 0; }; // r of the limited streams, [S][limitPitch] in clip order (null: no stream of the call is limited)
inline __host__ __device__ bool pcmLimited(const PcmLevel &l) { return (l.flags & kPcmFlagLimiter) && (l.mode == kPcmLevelProtect || l.mode == kPcmLevelLoudness); }
void launchPcmOut(int format, const float *in, long long inStreamStride, long long inChannelStride, void *out, long long outStreamStride, long long outFrameStride,
                  const int *counts, int S, int C, int maxFrames, unsigned *overs, hipStream_t st, const PcmDither *dither = nullptr, const PcmLevelIo &level = PcmLevelIo());
// Whole clips of ragged lengths (smst_clip.h; Batch::exact): each stream moves two segments of frames between the caller's buffer and a planar
// fp32 image -- `count` frames from frame `src` of its row(s) on the source side to frame `dst` on the destination side; zeros != 0: no
// source, the destination gets 0.0 (its code, in a frame format).  segs: [S][2] device.  format: an SMST_PCM_* code, or 0 for a caller's
// buffer that is planar fp32 itself (inner stride = channel stride instead of frame stride; the copy is then plain in both directions).
// maxCount: the largest count of any segment (sizes the grid; nothing is launched for 0).
struct ClipSeg { int src, dst, count, zeros; };
void launchClipIn(int format, const void *in, long long inStreamStride, long long inInnerStride, float *image, long long imageStreamStride, long long imageChannelStride,
                  const ClipSeg *segs, int S, int C, int maxCount, hipStream_t st);
void launchClipOut(int format, const float *image, long long imageStreamStride, long long imageChannelStride, void *out, long long outStreamStride, long long outInnerStride,
                   const ClipSeg *segs, int S, int C, int maxCount, unsigned *overs, hipStream_t st, const PcmDither *dither = nullptr, const PcmLevelIo &level = PcmLevelIo());
// The peak of every stream's clip -- the largest |v| of the image's samples that the segments cover, NaN skipped -- maxed into clipPeak[s]
// (the caller zeroes the words in front of it): the pass of a levelled clip call in which a stream has a whole-clip mode
void launchClipPeak(const float *image, long long imageStreamStride, long long imageChannelStride, const ClipSeg *segs, int S, int C, int maxCount, int *clipPeak, hipStream_t st);
// Integrated loudness of every stream's clip (include/smst.h, "Loudness", has the definition; smst_loudness.h the kernels).  One entry per
// stream, device: the two biquads' coefficients, the cascade's transition matrix to the power of the chunk length, the target power P, the
// absolute gate and the hop h of the 100-ms sub-blocks; h == 0: the stream is not measured.  All of it float64, computed by the host
// (loudEntryOf; false: the sample rate gives h < kLoudChunk).
constexpr int kLoudChunk = 256; // frames of a channel's clip, in clip order, that one lane filters
struct LoudCoef { double b0, b1, b2, a1, a2, d1, d2; }; // shelf: b0 b1 b2 / 1 a1 a2; high-pass: 1 -2 1 / 1 d1 d2
// meter != 0: kLoudRange (smst_loudness_range.h) measures the stream too; Pm, Ps: the powers of its momentary and short-term caps (+inf: none)
struct LoudEntry { LoudCoef k; double Ac[16], P, gate; int h, meter; double Pm, Ps; };
bool loudEntryOf(double sampleRate, double targetLufs, LoudEntry &e); // (meter 0, no caps)
// The passes' scratch, all float64 but the meters' last two: per stream the meters -- Z, the two block counts, gL --, per (stream, channel,
// chunk) the chunk's end state (then its incoming state) and its two partial sums, per (stream, channel) the sub-block sums, per stream the
// block powers.  maxChunks / maxSub: of the longest measured clip (loudScratchAt lays out `base`, which holds loudScratchDoubles)
struct LoudScratch { double *Z; int *counts; float *gain; double *ends, *partials, *sub, *z; int maxChunks, maxSub; };
inline size_t loudScratchDoubles(int S, int C, int maxChunks, int maxSub) { return (size_t)2*S + (S + 1)/2 + (size_t)S*C*maxChunks*6 + (size_t)S*C*maxSub + (size_t)S*maxSub; }
inline LoudScratch loudScratchAt(double *base, int S, int C, int maxChunks, int maxSub) {
	LoudScratch w;
	double *p = base;
	w.Z = p; p += S;
	w.counts = reinterpret_cast<int *>(p); p += S;
	w.gain = reinterpret_cast<float *>(p); p += (S + 1)/2;
	w.ends = p; p += (size_t)S*C*maxChunks*4;
	w.partials = p; p += (size_t)S*C*maxChunks*2;
	w.sub = p; p += (size_t)S*C*maxSub;
	w.z = p;
	w.maxChunks = maxChunks; w.maxSub = maxSub;
	return w;
}
// the four passes, on `st`: every stream's meters are written (a stream that is not measured: Z 0, no blocks, gL 1)
void launchClipLoudness(const float *image, long long imageStreamStride, long long imageChannelStride, const ClipSeg *segs, int S, int C,
                        const LoudEntry *loud, const float *weights, const LoudScratch &w, hipStream_t st);
// Loudness range and the two maxima of every metered stream's clip (include/smst.h, "Loudness range", has the definition;
// smst_loudness_range.h the kernel), from the sub-block sums and the block powers that the four passes left in `w`.  Per stream the meters --
// M, ST, lo, hi as powers, then ns and n -- and the short-term powers st[s*maxSt + i]; a stream that is not metered: zeros.  Where a cap of
// the stream's entry is finite, w.gain[s] is lowered to min(gL, gm, gs) in place.  maxSt >= ns of every metered stream
struct LoudRangeScratch { double *meters; int *counts; double *st; int maxSt; };
inline size_t loudRangeDoubles(int S, int maxSt) { return (size_t)5*S + (size_t)S*maxSt; }
inline LoudRangeScratch loudRangeAt(double *base, int S, int maxSt) {
	LoudRangeScratch r;
	r.meters = base;
	r.counts = reinterpret_cast<int *>(base + (size_t)4*S);
	r.st = base + (size_t)5*S;
	r.maxSt = maxSt;
	return r;
}
void launchClipLoudnessRange(const ClipSeg *segs, int S, int C, const LoudEntry *loud, const float *weights, const LoudScratch &w, const LoudRangeScratch &r, hipStream_t st);
// True peak of every flagged stream's clip (include/smst.h, "True peak", has the definition; smst_true_peak.h the kernel): a 4x polyphase
// interpolation in float64 of every channel, in clip order across the join of the two segments, maxed with the samples themselves into
// truePeak[s] as float bits (the caller zeroes the words in front of it).  level: the call's level entries, whose fourth word is the flag.
// maxFrames: the longest measured clip (sizes the grid; nothing is launched for 0).  The taps travel by value, as a kernel argument
constexpr int kTruePeakTile = 1024;                                        // frames of a channel's clip, in clip order, that one workgroup measures
constexpr int kTruePeakTaps = 12, kTruePeakLead = 5, kTruePeakTrail = 6;   // tap j of a frame weighs the sample j - 5 frames from it
struct TruePeakTable { float c[3][kTruePeakTaps]; };                       // phase p = 1, 2, 3 at [p - 1]
const TruePeakTable &truePeakTable();
void launchClipTruePeak(const float *image, long long imageStreamStride, long long imageChannelStride, const ClipSeg *segs, int S, int C, int maxFrames,
                        const PcmLevel *level, int *truePeak, hipStream_t st);
// Lookahead limiter of whole clips (include/smst.h, "Limiter", has the definition; smst_limiter.h the kernels), for the streams that
// pcmLimited() names.  Two passes on `st`, over the image and the segments of the passes above:
//   need   per frame, in clip order: all channels folded into need(n) = ceiling/(m(n)*g) where that is below 1   -> need[s*pitch + n]
//   gain   hold (the minimum of need over 2H + 1 frames), smoothed by the window of 2H + 1 floats, min'ed with need -> r[s*pitch + n],
//          and the stream's two meter words: meters[s] = max of bits(1.0f) - bits(r), meters[S + s] = frames with r < 1 (zeroed by the caller)
// level: the call's view (table, and loudGain where a stream is in the loudness mode).  maxFrames: the longest limited clip, <= pitch (sizes
// the grids; nothing is launched for 0).  H: the lookahead in frames, 1 ... kLimitMaxLookahead; window: device, limitWindow()'s floats
constexpr int kLimitTile = kTruePeakTile;       // frames of a clip, in clip order, that one workgroup of either pass takes
constexpr int kLimitMaxLookahead = 1024, kLimitDefaultLookahead = 72;
void limitWindow(int H, float *win);            // win[k + H] = float32(h_k/sum h), k = -H ... H: in double, one rounding
void launchClipLimit(const float *image, long long imageStreamStride, long long imageChannelStride, const ClipSeg *segs, int S, int C, int maxFrames,
                     const PcmLevelIo &level, int H, const float *window, float *need, float *r, long long pitch, int *meters, hipStream_t st);
// The limiter's streaming form (include/smst.h, "Stream limiter", has the definition; smst_stream_limiter.h the kernels), for the streams whose
// level entry has kPcmFlagStreamLimiter: the output of smst_batch_process_pcm / _flush_pcm 2H frames late, limited by the curve of the clip
// [2H zeros, every frame emitted so far].  What a batch carries, device: per stream two LINES -- need of the last 4H frames, [S][4H], and the
// last 2H frames of every channel before the gain, [S][C][2H] --, of which a call reads the one its entry's kPcmFlagStreamLimitSet names and
// writes the other, and the two meter words of kClipLimitGain, [2][S], which accumulate until they are taken.  What a call works in: the
// need row [S][needPitch >= 4H + longest limited count] and the r row [S][rPitch >= that count], stream-ordered scratch as the images are.
// A stream with kPcmFlagStreamLimitTruePeak is 2H + 6 frames late: need of a frame waits for the 6 frames its taps reach ahead.  Its need
// line is the one above -- need of the last 4H frames whose taps are complete --; its frames are carried in lines of their own, the last
// pcmStreamLimitTruePeakLine(H) = 2H + 11 frames of every channel, [S][C][2H + 11], two sets as above (null until a stream first gets the
// flag): the first 5 are the reach of the oldest missing need's taps, the 2H + 6 behind them what the output is late by
struct PcmStreamLimit {
	float *need[2] = {nullptr, nullptr};
	float *frames[2] = {nullptr, nullptr};
	float *truePeakFrames[2] = {nullptr, nullptr};
	int *meters = nullptr;
	float *needRow = nullptr, *rRow = nullptr;
	long long needPitch = 0, rPitch = 0;
	const float *window = nullptr; // limitWindow(H)'s floats, device
	int H = 0;
};
inline size_t pcmStreamLimitSetFloats(int S, int C, int H) { return (size_t)S*4*H + (size_t)S*C*2*H; } // one set of lines: need, then the frames
constexpr int kStreamLimitTruePeakDelay = kTruePeakTrail;                                                // SMST_STREAM_LIMITER_TRUE_PEAK_DELAY
inline __host__ __device__ int pcmStreamLimitTruePeakLine(int H) { return 2*H + kTruePeakLead + kTruePeakTrail; }
inline size_t pcmStreamLimitTruePeakSetFloats(int S, int C, int H) { return (size_t)S*C*pcmStreamLimitTruePeakLine(H); } // one set of the flag's lines
// need <- 1, frames <- +0.0 in both sets of `stream` (-1: of every stream), the flag's lines included where they exist, on `st`
void launchPcmLimitClear(const PcmStreamLimit &lim, int S, int C, int stream, hipStream_t st);
// launchPcmOut's levelled form for a call in which a limited stream has frames (maxLimited: the largest count of such a stream without the
// true-peak flag, maxTruePeak: of one with it; one of them >= 1): the two passes, then the conversion -- a kernel of its own -- that takes
// a limited stream's frame i from its line (i < 2H, or 2H + 6) or from the image behind it and multiplies it by r as well; a stream without
// the setting gets the levelled form's bytes.  Three launches on `st` -- with maxTruePeak < 1 exactly those of a batch that has no flag --,
// four where streams of both kinds have frames: each feed kernel takes its own kind
void launchPcmOutLimited(int format, const float *in, long long inStreamStride, long long inChannelStride, void *out, long long outStreamStride, long long outFrameStride,
                         const int *counts, int S, int C, int maxFrames, int maxLimited, int maxTruePeak, unsigned *overs, hipStream_t st, const PcmDither *dither,
                         const PcmLevelIo &level, const PcmStreamLimit &lim);
// Sample-rate conversion of whole clips in front of the engine (include/smst.h, "Resample", has the definition; smst_resample.h the kernel).
// A ratio L/M, reduced, the batch's rate over the clip's: N frames become Nr = ceil(N*L/M), frame n at input position n*M/L, formed by the T = 2H
// taps of its phase's row of a Kaiser-windowed sinc in float64, rounded once.  ResampleShape: what a ratio fixes -- H, T and the pitch of a
// row of its table ([L][pitch] floats, T rounded up to a multiple of 4, the padding 0.0); resampleTaps fills such a table (host, in double).
// ResampleEntry: one per stream, device -- L == 0: the stream is not resampled, the kernel leaves its rows alone.
// The kernel reads a raw image in which each resampled stream's clip lies from column 0 of its rows and writes resampled frame n where the
// stream's two segments put it (their counts add up to Nr; src is not read).  maxFrames: the largest Nr (sizes the grid; nothing is
// launched for 0); maxSpanPitch: the largest resampleSpanPitch of the launch's entries (sizes the LDS)
constexpr int kResampleTile = 1024;                      // resampled frames of a stream that one workgroup forms
constexpr int kResampleMaxTerm = 640, kResampleMaxRatios = 8;
constexpr int kResampleLdsFloats = 15360;                // 60 KB: the most a launch asks for
struct ResampleShape { int L, M, H, T, pitch; };
inline ResampleShape resampleShapeOf(int L, int M) { // (reduced, within the limits)
	ResampleShape g{L, M, 32, 64, 64};
	if (M > L) g.H = (32*M + L - 1)/L;
	g.T = 2*g.H;
	g.pitch = (g.T + 3)/4*4;
	return g;
}
struct ResampleEntry { const float *taps; int N, Nr, L, M, H, T, pitch, pad; };
// floats of one channel's LDS image of a tile: the span, at most ceil((kResampleTile - 1)*M/L) + T, in whole 16-byte words
inline __host__ __device__ int resampleSpanPitch(int L, int M, int T) { return (((kResampleTile - 1)*M + L - 1)/L + T + 3)/4*4; }
// ... and of a launch: up to 4 channels side by side where they fit the most a launch asks for, at least one
inline int resampleLdsFloats(int C, int maxSpanPitch) {
	int group = C < 4 ? C : 4;
	while (group > 1 && group*maxSpanPitch > kResampleLdsFloats) --group;
	return group*maxSpanPitch;
}
inline long long resampledLength(long long N, int L, int M) { return (N*L + M - 1)/M; }
void resampleTaps(const ResampleShape &g, float *out);
void launchClipResample(const float *raw, long long rawStreamStride, long long rawChannelStride, float *image, long long imageStreamStride, long long imageChannelStride,
                        const ClipSeg *segs, const ResampleEntry *entries, int S, int C, int maxFrames, int maxSpanPitch, hipStream_t st);

// The converter BEHIND the engine (include/smst.h, "Output resample", has the definition; smst_resample_out.h the kernel): a stream's ratio L/M is
// the delivery rate over the batch's; for Nd delivered frames the engine renders E = resampleRenderLength(Nd) frames, the smallest count that
// holds the centre (n*M)/L of every delivered frame.  ResampleOutEntry: one per stream, device -- L == 0: no ratio, the kernel leaves the
// stream's rows alone.  The kernel reads the E rendered frames where srcSegs puts them (src and count of the two segments: frames [0, k) and
// [k, E); dst is not read) and writes delivered frame n where dstSegs puts it (dst and count; the counts add up to Nd; src is not read).
// maxFrames: the largest Nd; maxSpanPitch: the largest resampleSpanPitch of the launch's entries
struct ResampleOutEntry { const float *taps; int E, Nd, L, M, H, T, pitch, pad; };
inline long long resampleRenderLength(long long Nd, int L, int M) { return Nd < 1 ? 0 : ((Nd - 1)*M)/L + 1; }
void launchClipResampleOut(const float *image, long long imageStreamStride, long long imageChannelStride, float *out, long long outStreamStride, long long outChannelStride,
                           const ClipSeg *srcSegs, const ClipSeg *dstSegs, const ResampleOutEntry *entries, int S, int C, int maxFrames, int maxSpanPitch, hipStream_t st);

// The converter's streaming form (include/smst.h, "Stream resample", has the definition; smst_stream_resample.h the kernel): a stream with the
// setting has been handed `fed` raw frames since its line was last cleared, and the engine the first made = streamResampleDue(fed - H) frames
// of "Resample" applied to them; a call that hands n frames completes k = streamResampleDue(fed + n - H) - made more.  What a batch carries,
// device: per stream and channel the last T - 1 raw frames in a row of kStreamResampleLine floats, two sets [2][S][C][kStreamResampleLine],
// of which a call reads the one its entry names and writes the other.  StreamResampleEntry: one per stream, device -- L == 0: the stream has
// no setting, n < 1: it has no frame in the call; either way the kernel leaves its rows and its line alone.  fresh != 0: the line counts as
// +0.0 (it was cleared); rawAt / outAt: the column of the call's first raw frame in the raw image and of its first frame in the engine's
// image.  maxFrames: the largest k (sizes the grid; a launch with 0 still writes the lines); maxSpanPitch: the largest
// resampleSpanPitchOf(..., streamResampleTileFrames(maxFrames)) of the launch's entries (sizes the LDS)
constexpr int kStreamResampleLine = 288;                 // floats of a channel's line: T - 1 <= 287 (T = 288 at 2/9)
struct StreamResampleEntry { const float *taps; long long fed, made, rawAt, outAt; int n, k, L, M, H, T, pitch, set, fresh, pad; };
inline __host__ __device__ int resampleSpanPitchOf(int L, int M, int T, int frames) { return (((frames - 1)*M + L - 1)/L + T + 3)/4*4; }
inline int streamResampleTileFrames(int maxFrames) { return maxFrames < 1 ? 1 : maxFrames < kResampleTile ? maxFrames : kResampleTile; }
inline long long streamResampleDue(long long q, int L, int M) { return q <= 0 ? 0 : (q*L + M - 1)/M; } // R(q) = ceil(max(q, 0)*L/M)
void launchPcmStreamResample(const float *raw, long long rawStreamStride, long long rawChannelStride, float *image, long long imageStreamStride, long long imageChannelStride,
                             float *lines, long long lineSetStride, const StreamResampleEntry *entries, int S, int C, int maxFrames, int maxSpanPitch, hipStream_t st);

// The converter's streaming form BEHIND the engine (include/smst.h, "Stream output resample", has the definition; smst_stream_resample_out.h
// the kernels): a stream with the setting has received `delivered` frames at the delivery rate since its line was last cleared, and the engine
// has rendered rendered = streamResampleOutDue(delivered) frames for it; a call that delivers Nd frames renders
// E = streamResampleOutDue(delivered + Nd) - rendered more.  Delivered frame n < Dl = streamResampleOutLatency is +0.0, frame n >= Dl is
// frame n - Dl of "Resample" applied to the rendered frames.  What a batch carries, device: per stream and channel the last
// kStreamResampleOutLine rendered frames, r(rendered - kStreamResampleOutLine + j) at [j], two sets [2][S][C][kStreamResampleOutLine], of
// which a call reads the one its entry names and writes the other.
// The line's length: the call's first frame n = delivered >= Dl sits at i = ((delivered - Dl)*M)/L and reaches back to i - (H - 1).  With
// a = delivered*M/L and b = (delivered - Dl)*M/L, a - b = Dl*M/L < (H*L/M + 1)*M/L = H + M/L, and ceil(a) - floor(b) < a - b + 2, a whole
// number, so ceil(a) - floor(b) <= H + ceil(M/L) + 1: the reach rendered - (i - (H - 1)) is at most T + ceil(M/L).  M/L <= 4.5 gives
// H <= 144, T <= 288, ceil(M/L) <= 5: 293 frames at 2/9, which kStreamResampleLine (288) does not hold.
// StreamResampleOutEntry: one per stream, device -- L == 0: the stream has no setting, Nd < 1: it has no frame in the call; either way the
// kernels leave its rows and its line alone.  fresh != 0: the line counts as +0.0 (it was cleared); imageAt / outAt: the column of the
// call's first rendered frame in the engine's output image and of its first delivered frame in the image the kernel writes.
// maxFrames: the largest Nd (sizes the grid); maxSpanPitch: the largest resampleSpanPitchOf(..., streamResampleTileFrames(maxFrames)) of the
// launch's entries (sizes the LDS)
constexpr int kStreamResampleOutLine = 296;              // floats of a channel's line: T + ceil(M/L) <= 293, in whole 16-byte words
static_assert(kStreamResampleOutLine >= 2*((32*9 + 1)/2) + (9 + 1)/2 && kStreamResampleOutLine%4 == 0, "the line holds T + ceil(M/L) frames at 2/9, the longest");
struct StreamResampleOutEntry { const float *taps; long long delivered, rendered, imageAt, outAt; int Nd, E, Dl, L, M, H, T, pitch, set, fresh; };
inline long long streamResampleOutDue(long long delivered, int L, int M) { return (delivered*M + L - 1)/L; } // ceil(delivered*M/L), delivered >= 0
inline int streamResampleOutLatency(int L, int M, int H) { return int(((long long)H*L + M - 1)/M); }       // Dl = ceil(H*L/M)
void launchPcmStreamResampleOut(const float *image, long long imageStreamStride, long long imageChannelStride, float *out, long long outStreamStride, long long outChannelStride,
                                float *lines, long long lineSetStride, const StreamResampleOutEntry *entries, int S, int C, int maxFrames, int maxSpanPitch, hipStream_t st);
// ... and the delivered frames of the streams that have the setting from `from`, column outAt of their rows, over the rendered ones in
// `image`, from column imageAt: the output stages then read ONE image, as they did.  Streams without the setting are not touched
void launchPcmStreamResampleOutCopy(const float *from, long long fromStreamStride, long long fromChannelStride, float *image, long long imageStreamStride, long long imageChannelStride,
                                    const StreamResampleOutEntry *entries, int S, int C, int maxFrames, hipStream_t st);

// The R 128 meters' streaming form (include/smst.h, "Stream meter", has the definition; smst_stream_meter.h the kernels), for the streams whose
// configuration has `on`: every frame that smst_batch_process_pcm / _flush_pcm write for the stream, up to cap = maxSubBlocks*h of them, is
// measured behind the output conversion.  What a batch carries, device, ONE set ordered by the batch's stream: per stream its configuration
// (written by the setter's clear kernel, so a call in flight keeps the one it was issued under), per (stream, channel) kStreamMeterDoubles
// doubles -- x_in at [0], the state run from it at [4], the state run from zero at [8], e0, e1, the running sub-block sum, and the frames
// metered so far (Tm, a whole number) at [kStreamMeterAt] -- and the last kStreamMeterLine frames, per stream the running true-peak and
// sample-peak words, [2][S], and the closed sub-block sums sub[(s*C + c)*maxSub + j] in LoudScratch::sub's layout, appended and never rewritten
constexpr int kStreamMeterDoubles = 16, kStreamMeterAt = 15;
constexpr int kStreamMeterLine = kTruePeakLead + kTruePeakTrail; // 11 frames: what the taps of the next frames reach back to
struct StreamMeterConfig { LoudCoef k; double Ac[16]; int h, on, cap, pad; };
struct PcmStreamMeter {
	StreamMeterConfig *config = nullptr;
	double *state = nullptr;
	float *frames = nullptr;
	int *words = nullptr;
	double *sub = nullptr;
	int maxSub = 0;
	double *scan = nullptr; // the chunk-scan form's scratch of a call, stream-ordered as the images are: streamMeterScanDoubles(S, C, maxChunks)
	int maxChunks = 0;
};
// The update's two forms give the same bits.  The short-call form serves a call by one lane per (stream, channel), whatever its length; the
// chunk-scan form spreads a call's chunks over lanes in three passes and pays four launches for it.  A call whose longest metered count
// reaches kStreamMeterScanFrames takes the chunk-scan form (EXPERIMENTS.md, "Stream meter", has the measurement)
#ifndef SMST_STREAM_METER_SCAN_FRAMES
#define SMST_STREAM_METER_SCAN_FRAMES 2048
#endif
constexpr int kStreamMeterScanFrames = SMST_STREAM_METER_SCAN_FRAMES;
inline bool streamMeterScans(int maxFrames, int form) { return form == 2 || (form == 0 && maxFrames >= kStreamMeterScanFrames); }
inline int streamMeterChunksOf(int maxFrames) { return maxFrames/kLoudChunk + 2; } // the chunks that maxFrames frames touch, from any position
inline size_t streamMeterScanDoubles(int S, int C, int maxChunks) { return (size_t)S*C*((size_t)maxChunks*6 + 4); }
// a reading's words beside the clip stages' scratch: peaks [2][S] (true peak, sample peak, float bits), newest [S][2] (z[nb - 1], st[ns - 1])
struct StreamMeterReading { int *peaks; double *newest; };
// the stream's (-1: every stream's) meter cleared -- nothing metered -- and, cfg != null, its configuration set; on `st`
void launchPcmStreamMeterClear(const PcmStreamMeter &m, int S, int C, int stream, const StreamMeterConfig *cfg, hipStream_t st);
// a call's update: counts [S] device, the frames written for each stream, which lie from column starts[s] (null: 0) of its rows of the image;
// maxFrames: the largest count of a metered stream (nothing is launched for 0).  form: 0 -- the launcher chooses by maxFrames --, 1 the
// short-call form, 2 the chunk-scan form; both give the same bits.  On `st`
void launchPcmStreamMeter(const float *image, long long imageStreamStride, long long imageChannelStride, const int *counts, const int *starts, int S, int C, int maxFrames,
                          const PcmStreamMeter &m, int form, hipStream_t st);
// a reading: kLoudGate from its second stage on and kLoudRange over the histories (w.sub = m.sub, w.maxSub = m.maxSub; segs: one segment of
// count Tm per stream; loud: h == 0 where the stream is not metered), then the true-peak edge and the newest powers.  Three launches on `st`
void launchPcmStreamMeterRead(const ClipSeg *segs, const LoudEntry *loud, const float *weights, int S, int C, const PcmStreamMeter &m, const LoudScratch &w, const LoudRangeScratch &r,
                              const StreamMeterReading &out, hipStream_t st);

} // namespace smst
