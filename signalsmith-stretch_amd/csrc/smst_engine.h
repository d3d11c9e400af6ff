// Host-side engine: owns a batch of independent streams on one GPU, mirrors the reference's block scheduler
// (signalsmith-stretch.h:280-319) per stream, and drives the gfx950 kernels tile by tile.
#pragma once
#include <algorithm>
#include <array>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>
#include <hip/hip_runtime.h>
#include "smst_device.h"
#include "smst_recurrence_form.h"
#include "smst_staging.h"
#include "smst_pcm_tables.h"

namespace smst {

struct StreamSched { // reference members: signalsmith-stretch.h:494-529
	size_t samplesSinceLast = SIZE_MAX; // blockProcess.samplesSinceLast, :496
	int prevInputOffset = -1;           // :527
	bool didSeek = false;               // :528
	float seekTimeFactor = 1;           // :529
	size_t silenceCounter = 0;          // :510
	bool silenceFirst = true;           // :511
	unsigned seed = 0;                  // randomEngine, :616 -- the state of libstdc++'s minstd_rand0 (smst_kernels_common.h: engineDraw)
};

// Split computation (signalsmith-stretch.h:292-296,321-325): a block's steps are spread over its interval, so between two interval
// boundaries one block is IN FLIGHT -- analysed from the input as it stood at the block's start (:293), everything else still to come,
// and the steps that come read the live parameters and the live Band state.  The engine analyses such a block when it starts, keeps its
// spectra, and runs the rest when the interval is complete (or when a flush() needs part of it); what happened in between is recorded here.
struct PendingBlock {
	bool valid = false;
	unsigned flags = 0;      // HopDesc.flags as latched at the block's start (:299-310)
	float timeFactor = 1;    // :312
	unsigned seed = 0;       // the random engine's state before this block's draws
	int startBin = 0;        // a flush() between two chunks of the main prediction (:722-803): the bins below were computed, then zeroed (:458-463)
	bool zeroPrevAfter = false; // a flush() after `.input -> .prevInput` (:806-811): Band.prevInput stays zero
	// the parameters as findPeaks (:874), updateFormants step 0 (:982) and step 2 (:1020) saw them, once each has run (frozen*)
	bool frozenPeaks = false, frozenForm0 = false, frozenForm2 = false;
	StreamParams peaks{}, form0{}, form2{};
};
struct StepLayout { // index of each step of a block in the reference's order (:304-318, :620-632); -1: the block has no such step
	int reanalyse0 = -1, analyse0 = -1, copyIn = -1, peaks = -1, form0 = -1, form2 = -1, main0 = 0, prevCopy = -1, spectrum = 0, synth0 = 0, steps = 0;
};

struct BatchTimings { // filled when profiling is enabled (hipEvent pairs around each kernel class)
	double analyseMs = 0, feedMs = 0, predictMs = 0, chainMs = 0, synthMs = 0, emitMs = 0, otherMs = 0;
	long analyseLaunches = 0, synthLaunches = 0, chainLaunches = 0, predictLaunches = 0, emitLaunches = 0;
	double chainLiveMs = 0;   // mode 2: the recurrence kernel timed in place (events on its own stream, nothing serialised)
	long chainLiveLaunches = 0;
};

class Batch {
public:
	Batch(int streams, int channels, int block, int interval, bool split, int device, long seed, bool halfState = false);
	~Batch();
	Batch(const Batch &) = delete;
	Batch &operator=(const Batch &) = delete;

	// geometry queries (signalsmith-stretch.h:42-47,96-104,166-168,205-207)
	int streams() const { return S; }
	int channels() const { return C; }
	int blockSamples() const { return B; }
	int intervalSamples() const { return I; }
	int fftSamples() const { return N; }
	int bands() const { return M; }
	bool splitComputation() const { return split; }
	bool halfPrecisionState() const { return halfState; }
	int inputLatency() const { return B - B/2; }
	int outputLatency() const { return B/2 + (split ? I : 0); }
	int seekLength() const { return B + I; }
	int outputSeekLength(float playbackRate) const { return int(inputLatency() + playbackRate*outputLatency()); }

	void reset(); // :49-60, all streams
	// parameter setters, stream = -1 for all (signalsmith-stretch.h:107-135)
	void setTransposeFactor(int stream, float multiplier, float tonalityLimit);
	void setTransposeSemitones(int stream, float semitones, float tonalityLimit);
	void setFormantFactor(int stream, float multiplier, bool compensatePitch);
	void setFormantSemitones(int stream, float semitones, bool compensatePitch);
	void setFormantBase(int stream, float baseFreq);
	void setFreqMapTable(int stream, const float *table, int n); // table form of setFreqMap (:120); n == 0 clears

	// All sample pointers are DEVICE pointers here (planar: stream stride, channel stride, contiguous samples).
	// `active` (host, may be null) masks streams out of the call entirely.
	void process(const float *in, long long inStreamStride, long long inChannelStride, const int *inSamples,
	             float *out, long long outStreamStride, long long outChannelStride, const int *outSamples,
	             const unsigned char *active = nullptr); // :210-423
	void seek(const float *in, long long inStreamStride, long long inChannelStride, const int *inSamples,
	          const double *playbackRates, const unsigned char *active = nullptr); // :140-165
	void flush(float *out, long long outStreamStride, long long outChannelStride, const int *outSamples,
	           const float *playbackRates, const unsigned char *active = nullptr); // :427-464
	void outputSeek(const float *in, long long inStreamStride, long long inChannelStride, const int *inputLengths,
	                const unsigned char *active = nullptr); // :173-204; with a mask: only those streams are reset, sought and folded back
	// exact() (:468-491): the lengths of its three stages for one clip -- outputSeek(in[0, seekLength)), process(in[seekLength, in) -> out[0, outputIndex)),
	// flush(out[outputIndex, out), rate) -- in the reference's own arithmetic (:470-472, :483).  outputSamples > 0; tooShort: :471-480, nothing else is set.
	struct ExactLengths { float rate; int seekLength, outputIndex; bool tooShort; };
	ExactLengths exactLengths(int inputSamples, int outputSamples) const {
		ExactLengths l{inputSamples/float(outputSamples), 0, 0, false};
		l.seekLength = outputSeekLength(l.rate);
		l.tooShort = inputSamples < l.seekLength;
		if (!l.tooShort) l.outputIndex = int(outputSamples - l.seekLength/l.rate);
		return l;
	}
	// exact() of every stream with outSamples[s] >= 0, each a whole clip of its own length and rate, in ONE outputSeek, ONE main process and ONE
	// flush.  The caller's buffers (device memory) are planar fp32 (format 0: inner stride = channel stride) or frames of an SMST_PCM_* format
	// (inner stride = frame stride); the stages run on the engine's own planar images, in which every stream's stage begins at one column
	// (smst_clip.h).  A stream whose input is shorter than its outputSeekLength gets zeros and keeps its state (:471-480).  tooShort (host, may
	// be null): 1 for such a stream, 0 for the others that take part, written once every stage has been issued; a stream left out keeps its entry.  overs (device, may be null): [S][2] counters of the frame conversion.
	// Counts are checked by the caller: outSamples[s] != 0, inSamples[s] >= 0 where outSamples[s] > 0.
	// pcm (frame formats; smst_pcm_tables.h): the device side of the output conversion, which rides in the caller's per-call table.  wholeClip
	// (host, [S]; null where the call is not levelled): which streams' gains come from their clip's peak -- if one of them runs, kClipPeak
	// does.  loudHop (host, [S]; null where no stream is measured): h of the streams in the loudness mode and of the metered ones, 0 for the others -- if one of
	// them runs, the four passes of smst_loudness.h do, and kClipOut finds the gains in the engine's meters.  truePeak (host, [S]; null where
	// no stream has the true-peak flag): the streams that have it -- if one of them runs, kClipTruePeak (smst_true_peak.h) does, and kClipOut
	// forms those streams' whole-clip gains from the words it leaves in the engine's memory
	struct ClipIo { const void *in; long long inStreamStride, inInnerStride; void *out; long long outStreamStride, outInnerStride; int format;
		PcmOutCall pcm; const unsigned char *wholeClip = nullptr; const int *loudHop = nullptr; const unsigned char *truePeak = nullptr;
		const unsigned char *loudMeter = nullptr;  // (host, [S]; null where no stream is metered: the streams whose loudness entry has the meter flag -- loudHop has their
		                                           // h whatever their mode, and if one of them runs, kLoudRange (smst_loudness_range.h) does behind the four passes)
		const unsigned char *limiter = nullptr;    // (host, [S]; null where no stream is limited: the streams whose level entry pcmLimited() names -- if one
		                                           // of them runs, the two passes of smst_limiter.h do, and kClipOut takes their r from the engine's scratch)
		bool outResample = false;                  // (the call serves the streams' OUTPUT ratios, a frame format only: outSamples[s] of a stream that has one counts delivered
		                                           // frames, the engine renders outRenderLengthOf(s, outSamples[s]), and kClipResampleOut (smst_resample_out.h) forms the delivered
		                                           // frames in front of the level stages; false: the caller has refused them)
		bool resample = false; };                  // (the call serves the streams' ratios, a frame format only: inSamples[s] of a stream that has one counts frames at the
		                                           // clip's rate, and kClipResample (smst_resample.h) forms its Nr frames in front of the stages; false: the caller has refused them)
	// Resample (include/smst.h, "Resample"): a stream's ratio up/down, the batch's rate over its clips' rate; 1/1: none.  setResample reduces
	// and checks the ratio (Error with the limit in its message) and, for the first stream that takes a ratio, builds the ratio's table and puts
	// it into device memory -- never in a call; a ratio that no stream has any more frees its table.  stream -1: every stream
	// streaming: the stream's OTHER setting, the one the streaming calls read (include/smst.h, "Stream resample") -- a ratio of its own per
	// stream, which shares the tables and their kResampleMaxRatios slots: a slot is live while any setting of any stream uses it
	// output: the stream's THIRD setting (include/smst.h, "Output resample"), the delivery rate over the batch's rate, which exact() serves
	// behind the engine; it shares the tables and the slots as well
	// streaming output: the stream's FOURTH setting (include/smst.h, "Stream output resample"), the delivery rate over the batch's rate in the
	// streaming calls; it shares the tables and the slots too
	enum ResampleSetting { kResampleClip = 0, kResampleStream = 1, kResampleOut = 2, kResampleStreamOut = 3 };
	void setResample(int stream, int up, int down, int setting = kResampleClip);
	bool outResampled(int stream) const { return outResampleSlot[stream] >= 0; }
	void outResampleOf(int stream, int &up, int &down) const;
	long long outRenderLengthOf(int stream, long long outSamples) const; // E of outSamples delivered frames of the stream (outSamples itself where it has no output ratio)
	bool resampled(int stream) const { return resampleSlot[stream] >= 0; }
	bool streamResampled(int stream) const { return streamResampleSlot[stream] >= 0; }
	void streamResampleOf(int stream, int &up, int &down) const;
	// shape and table (device) of a stream that has the streaming setting
	const ResampleShape &streamResampleShape(int stream) const { return resampleSlots[streamResampleSlot[stream]].shape; }
	const float *streamResampleTaps(int stream) const { return resampleSlots[streamResampleSlot[stream]].taps; }
	bool streamOutResampled(int stream) const { return streamOutResampleSlot[stream] >= 0; }
	void streamOutResampleOf(int stream, int &up, int &down) const;
	// shape and table (device) of a stream that has the streaming output setting
	const ResampleShape &streamOutResampleShape(int stream) const { return resampleSlots[streamOutResampleSlot[stream]].shape; }
	const float *streamOutResampleTaps(int stream) const { return resampleSlots[streamOutResampleSlot[stream]].taps; }
	void resampleOf(int stream, int &up, int &down) const;
	long long resampledLengthOf(int stream, long long inSamples) const; // Nr of a clip of the stream (inSamples itself where it has no ratio)
	// The limiter's lookahead H in frames (include/smst.h, "Limiter"), 1 ... kLimitMaxLookahead, the batch's one.  prepareLimiter() puts the
	// window of the current H into device memory (the first call allocates it); setLimiterLookahead() does so again where it is there already.
	// Neither runs in an exact call.  readLimiter: the meters of the newest exact call that limited, [S] each (1 and 0: a stream it did not
	// limit); false: none has.  Synchronises
	void setLimiterLookahead(int frames);
	int limiterLookahead() const { return limitH; }
	void prepareLimiter();
	const float *limiterWindow() const { return dLimitWin; } // (device; null before the first prepareLimiter(): the stream limiter of the C ABI reads it too)
	bool readLimiter(float *minGain, long long *limitedFrames);
	// the true peaks of the newest exact call that measured, [S] (0: a stream it did not measure); false: none has.  Synchronises
	bool readTruePeaks(float *truePeaks);
	// the loudness meters of the newest exact call that measured, [S] and [S][2] (blocks past the absolute gate, past both); false: none has.  Synchronises
	bool readLoudness(double *Z, int *counts);
	// the range meters of the newest exact call that metered, [S][4] (M, ST, lo, hi: powers) and [S][2] (ns, n); false: none has.  Synchronises
	bool readLoudnessRange(double *meters, int *counts);
	void exact(const ClipIo &io, const int *inSamples, const int *outSamples, unsigned char *tooShort);
	void synchronize();

	hipStream_t stream() const { return st; }
	int device() const { return dev; }
	void growLivePool(size_t pairs);
	void enableProfiling(int mode); // 1: every kernel class, serialised; 2: recurrence kernel in place (timing events come from a pool created here, not inside process())
	BatchTimings takeTimings();
	// Host time of process() since the last take: wall time inside the calls, the part of it spent WAITING for the device (the call before the
	// previous one to finish -- there are two sets of per-call tables -- and the silence gate's readback), and the number of calls.  What is
	// left is the host's own work: the per-stream block scheduler, the table fills and the enqueues.
	struct HostTimes { double callMs = 0, waitTablesMs = 0, waitGateMs = 0; long calls = 0; };
	HostTimes takeHostTimes() { HostTimes t = hostTimes; hostTimes = HostTimes(); return t; }
	size_t workspaceBytes() const { return wsBytes; }
	long allocationEvents() const { return allocEvents; } // test hook: must not move across steady-state process() calls
	// order the batch's work after everything already enqueued on `other` / make `other` wait for the batch's work so far
	void waitForStream(hipStream_t other);
	void signalStream(hipStream_t other);
	int subBatchStreams() const { return subS; }
	int lastBlockSteps(int stream) const { return (stream >= 0 && stream < S) ? lastSteps[stream] : 0; } // blockProcess.steps of the stream's newest block (:284-318)
	int lastCallBlocks(int stream) const { return (stream >= 0 && stream < S) ? lastStarts[stream] : 0; } // blocks that began in the stream's most recent process() (:281)
	// the object is copyable in the reference (a plain struct, signalsmith-stretch.h:34-35): same geometry, stream count and device required;
	// the whole carried state of every stream of `other` replaces this batch's (moveStreamsFrom, stream s to stream s)
	void copyStateFrom(Batch &other);
	// What the reference's configure() (:71-94) leaves ALONE when an instance is configured again: the random engine (seeded in the
	// constructor only, :38-39), prevInputOffset, didSeek / seekTimeFactor, the silence counter and the pitch-estimate averages
	// (all reset by reset(), :49-60, not by configure).  `other` is the stream's previous batch (same stream count).
	void inheritAcrossConfigure(Batch &other);
	// One stream's whole carried state from a batch of the SAME geometry and device but any stream count (a pool's group takes a member
	// in, lets one go, regrows), for the rows of the listed streams: every device array of carriedArrays() (of a double-buffered one the
	// source's CURRENT half, into both halves here: which half is current belongs to a batch, not to a stream), the host row
	// (takeHostRow) and the stream's own frequency-map tables.  The device part is ONE launch (kMoveStreams) however many streams move.
	// Both batches are synchronised; the source rows are left as they are.
	void moveStreamFrom(Batch &src, int srcStream, int dstStream) { moveStreamsFrom(src, &srcStream, &dstStream, 1); }
	void moveStreamsFrom(Batch &src, const int *srcStreams, const int *dstStreams, int n);
	// reset() (:49-60) of ONE stream: its neighbours are not touched
	void resetStream(int stream);
	void resetStreamsMasked(const unsigned char *active); // ... of every stream with active[s] != 0

	// test hooks: copy state rows to the host (which: 0 input, 1 prevInput, 2 output -> 2*C*M floats; 3 energy -> C*M)
	void debugGetState(int stream, int which, float *dst);
	void debugGetCarry(int stream, float *sums, float *products); // [C][B+I], [B+I]
	// teacher-forcing hooks (tests only): overwrite the carried per-bin state / overlap-add carry of one stream
	void debugSetState(int stream, int which, const float *src);
	void debugSetCarry(int stream, const float *sums, const float *products);
	// output map (inputBin, freqGrad per bin, signalsmith-stretch.h:587-590) of the stream's last hop of the last process()
	// call; false if that hop had no frequency map
	bool debugGetMap(int stream, float *dst);
	// formant stage of the stream's newest hop of the last process() call (separate feed kernels only): energy ratio per bin, envelope per bin,
	// the pitch estimate in bins; false if that hop had no formant processing or the batch runs the fused feed kernels
	bool debugGetFormants(int stream, float *ratio, float *envelope, float *freqEstimate);

private:
	int S, C, B, I, N, M, L;
	bool split;
	bool halfState = false; // carried Band.output / Prediction.energy / overlap-add sums in fp16 (fp32 arithmetic throughout)
	int dev;
	hipStream_t st = nullptr;       // feed-forward kernels + everything the caller synchronises on
	hipStream_t stChain = nullptr;  // the bin recurrence (few waves, latency-bound): overlaps with the bulk kernels
	hipStream_t stSynth = nullptr;  // synthesis + emission of the previous tile
	hipStream_t stGate = nullptr;   // silence-gate reduction + table uploads of the NEXT call, while the previous call still runs
	// Per-call device tables exist twice (smst_staging.h): a call fills one set on `stGate` while kernels of the previous call read the other
	// ... and so does their PINNED host staging (h*): nothing pageable is handed to an async copy, so the only host
	// synchronisation of a call is the silence-gate readback.  That holds for every table of the engine: the sets below (callSets,
	// pendSets, stageSets, clipSets) and the parameter rows (hParams) are all of its uploads on the calling paths.
	struct CallSet {
		int *inSamples, *outSamples, *flags, *tileInfo, *resetBits; HopDesc *hops; EmitDesc *emit;
		int *hInSamples, *hOutSamples, *hFlags, *hTileInfo, *hResetBits; HopDesc *hHops; EmitDesc *hEmit; float *hEnergy;
		HopDesc *pendHops = nullptr, *hPendHops = nullptr; // split computation: the block each stream leaves in flight at the end of the call ([S], analysis only)
		size_t hopsCap, emitCap, tileInfoCap;
		hipEvent_t tables; // the uploads on `stGate`, for `st` to wait on
		std::vector<void *> retiredDevice, retiredPinned; // outgrown tables that the previous call may still read
		~CallSet() { if (tables) hipEventDestroy(tables); }
	};
	TwoSets<CallSet> callSets;
	// The whole-call stages (seek, flush, outputSeek's fold-back, resetStreams) hand the device per-stream COLUMNS of S ints: a stage takes a
	// set, fills its first columns, uploads them in one copy on `st`, launches, and gives the set back.  hEnergy: seek()'s readback.
	static constexpr int kStageColumns = 3;
	struct StageSet { int *host, *dev; float *hEnergy; };
	TwoSets<StageSet> stageSets;
	void uploadStage(const StageSet &t, int columns);
	hipEvent_t evStart = nullptr, evFeed[3] = {nullptr, nullptr, nullptr}, evChain[3] = {nullptr, nullptr, nullptr}, evOut[3] = {nullptr, nullptr, nullptr}, evSynth[3] = {nullptr, nullptr, nullptr}; // (the third set: the continuous wavefront's tile pipeline is one stage deeper)
	struct TileBuffers { float2 *Xcur, *Xprev, *OUT, *dump, *map, *peaksT; float4 *REC; PredEntry *PE; float *ratio, *envelope, *energyT, *smoothT, *est, *freqEst, *frames; float2 *fftScratch; } slots[3]{}; // [2]: only what a plain tile touches, only where the continuous wavefront applies (allocateWorkspace)
	bool overlap = true, carriedEmit = true; // (smst_switches.h)
	FormSwitches formSwitches{};             // ... those that take part in the choice of a tile's recurrence (smst_recurrence_form.h)
	int contWriterWave = 4;
	float2 *dContSave = nullptr; // kVocoderCont: the recurrence wave's history between two launches, [S][8*C*64]
	double workspaceGiB = 0;
	int subStreamsAsked = 0;
	int subS = 0;
	// per-call host scratch, kept between calls (no heap traffic in steady state); growth events are counted
	std::vector<int> hopFirst, hopCount, maxSpanV;
	std::vector<TileSummary> tileHasV, pendTileHas; // [sub][tile] of a call, [sub] of a run of blocks in flight
	std::vector<unsigned char> leavesPendingV, ridesV;
	// ... and of the whole-call stages, [S] each: a stage's own, never shared (exact() hands its own down to outputSeek(), process() and flush())
	struct FlushScratch { std::vector<int> blockOut, blockIn, synthChannels; std::vector<unsigned char> runBlock, on; } flushV;
	struct OutputSeekScratch { std::vector<int> seekSamples, surplus, preOut, done; std::vector<double> rates; std::vector<unsigned char> mask; } outputSeekV;
	struct ExactScratch { std::vector<int> seekLen, rest, procOut, flushN, frames, render; std::vector<float> rates; std::vector<unsigned char> run; } exactV; // (frames: a clip's length at the batch's rate; render: the frames the engine renders, E of an out-resampled stream)
	long allocEvents = 0; // device allocations + pinned allocations + host table growth since construction
	size_t wsBytes = 0;
	DevBatch d{};
	std::vector<StreamSched> sched;
	unsigned lcgHopJump = 1; // 16807^(2M - 2) mod (2^31 - 1): what one randomised hop advances a stream's engine by
	unsigned advanceOneHop(unsigned seed) const;
	struct LastHop { int slot = -1, local = -1, subLocal = 0; bool mapped = false, formants = false; };
	std::vector<LastHop> lastHop; // where each stream's newest hop sits in the tile workspaces (debugGetMap)
	void noteLastHop(int s, int slot, int local, unsigned flags);
	std::vector<StreamParams> params;
	bool paramsDirty = true;
	// ---- split computation: the block in flight (see PendingBlock) ----
	std::vector<int> lastSteps, lastStarts;
	std::vector<int> carryBase; // the host's copy of DevBatch::carryBase[carryCur]
	EmitDesc *dZeroEmit = nullptr;
	std::vector<int> histBase;  // the host's copy of DevBatch::histBase (where each stream's input-history window begins)
	std::vector<PendingBlock> pend;
	float2 *dPendIn = nullptr, *dPendPrev = nullptr; // its spectra, [S][C][Mp]: Band.input and (re-analysed) Band.prevInput
	struct PendSet { // tables of one run of blocks in flight (twice, like CallSet: pinned staging, asynchronous uploads)
		HopDesc *hops, *hHops; EmitDesc *emit, *hEmit; int *tileInfo, *hTileInfo, *bits, *hBits, *synthChannels, *hSynthChannels;
		StreamParams *prm[3], *hPrm[3];
	};
	TwoSets<PendSet> pendSets;
	int *dZeroCounts = nullptr; // [S] zeros: the sample counts of a run that consumes and emits nothing
	std::vector<int> pendList;  // streams of the run being prepared
	std::vector<int> pendMaxSpan;
	StepLayout stepLayout(unsigned flags) const;
	size_t stepsExecuted(size_t steps, size_t samplesIntoInterval) const;
	void freezePendingParams(int s);   // before a setter changes params[s]
	unsigned seedAfterDroppedBlock(int s) const; // the random engine once the block in flight is dropped (reset / silence / configure)
	void pendingHop(int s, HopDesc &hd) const; // the HopDesc of stream s's block in flight
	int aheadOffset(int s) const;
	void runPendingBlocks(const int *synthChannels); // runs the blocks of `pendList` (a tile of one hop per stream; no input, no output samples)
	struct TileRun { const IoArgs *io; int nTiles, maxHops; const TileSummary *tileHas; const int *maxSpan; const int *dTileInfo; bool pendingRun; const int *dSynthChannels; bool carriedOnly; };
	void settleCarry();
	void runTiles(const TileRun &run);
	struct TileStreams { bool serial; hipStream_t sF, sC, sS; }; // a segment's streams: feed-forward, recurrence, synthesis + emission (all `st` when serial)
	TileStreams forkTileStreams(const TileRun &run);
	void joinTileStreams(const TileStreams &ts, int first, int passes, int depth);
	template <typename F> void timedRecurrence(const TileStreams &ts, F &&launch);
	DevBatch tileView(const TileBuffers &w, int carryCur, const int *tileInfo) const;
	void runTilesRange(const TileRun &run, int tile0, int tile1, int carryFirst); // tile by tile
	bool continuousApplies(const TileRun &run, int tile) const;
	void runTilesContinuous(const TileRun &run, int tile0, int tile1, int carryFirst); // the recurrence as ONE wavefront through the tiles [tile0, tile1) (kVocoderCont)
	struct CallPlan { // what the stages of one process() call hand to each other
		CallSet *cs; const unsigned char *active; // process(): the call's table set, the caller's stream mask (may be null)
		int maxHops; bool anyPass, anyClear;      // gateAndCount(): most hops of any stream; a stream passed through / cleared by the silence gate
		int nTiles, hopStride; size_t needHops, needEmit, needInfo; // process(): tiles, descriptors per stream row, elements of the hops / emit / tileInfo tables
		bool anyPendAnalysis, pendInCall, pendLate; // scheduleStream(): a block left in flight needs analysing; its windows lie in the call / reach into the history
	};
	void gateAndCount(CallPlan &c);
	template <typename T> void growCallTable(CallSet &t, bool mine, T *&dev, T *&host, size_t &cap, size_t need);
	void growCallTables(const CallPlan &c);
	void scheduleStream(CallPlan &c, int s);
	void summariseStreamTiles(const CallPlan &c, int s);
	bool profiling = false, liveTiming = false;
	std::vector<std::pair<hipEvent_t, hipEvent_t>> liveEvents; // pairs recorded since the last takeTimings()
	std::vector<std::pair<hipEvent_t, hipEvent_t>> livePool;   // every pair ever created; [0, liveEvents.size()) are in use
	BatchTimings timings;
	HostTimes hostTimes;

	std::vector<void *> allocations;
	float *dEnergy = nullptr;
	int *dInSamples = nullptr, *dOutSamples = nullptr, *dFlags = nullptr;
	HopDesc *dHops = nullptr;
	EmitDesc *dEmit = nullptr;
	int *dTileInfo = nullptr;
	float *dSeedWp = nullptr; // reset(0.1) window-product seed, device copy
	hipEvent_t evOrder = nullptr;
	std::vector<void *> pinned;
	template <typename T> T *pinnedAlloc(size_t count);
	void pinnedFree(void *p);
	void releaseAll();
	template <typename Pick> void resetStreams(Pick pick, int bits, bool keepAhead = false); // kResetStreams with `bits` for the streams that pick(s) names; keepAhead: see launchResetStreams' keep
	template <typename Pick> void resetPicked(Pick pick); // resetStream / resetStreamsMasked
	bool checkLaunches = false; // SMST_CHECK_LAUNCHES=1: hipGetLastError() after every launch group of process(), not only at its end
	void checkLaunch(const char *what);
	float *dZeros = nullptr;
	size_t zerosCapacity = 0;
	float *dScratchOut = nullptr;
	size_t scratchOutCapacity = 0;
	// exact(): the planar images the stages run on ([S][C][pitch], grown on demand) and the segment tables of the two clip kernels, twice as the
	// per-call tables are (a call returns before its last kernel has run)
	float *dClipIn = nullptr, *dClipOut = nullptr;
	size_t clipInCapacity = 0, clipOutCapacity = 0;
	float *dLoud = nullptr; // the loudness passes' scratch (LoudScratch: float64, the meters in front), grown on demand as the images are
	size_t loudCapacity = 0;
	float *dLoudRange = nullptr; // kLoudRange's scratch (LoudRangeScratch: float64, the meters in front of the short-term powers), grown by the calls that meter
	size_t loudRangeCapacity = 0;
	float *dTruePeak = nullptr; // the true-peak words of the newest exact call that measured ([S] float bits), allocated by the first one
	size_t truePeakCapacity = 0;
	// the limiter: the meters of the newest exact call that limited ([2][S] ints) in front of need and r ([S][pitch] floats each), grown on
	// demand as the images are; the window of 2*kLimitMaxLookahead + 1 floats, allocated by the first prepareLimiter()
	float *dLimit = nullptr, *dLimitWin = nullptr;
	size_t limitCapacity = 0;
	int limitH = kLimitDefaultLookahead;
	// resHost / resDev: the table of a call with a resampled stream (ResampleTableLayout), allocated by the first such call
	// outHost / outDev: the table of a call with an out-resampled stream (ResampleOutTableLayout), allocated by the first such call
	struct ClipSet { ClipSeg *host, *dev; unsigned char *resHost, *resDev, *outHost, *outDev; }; // [2][S][2]: input segments, output segments
	TwoSets<ClipSet> clipSets;
	// Resample: the raw image of the resampled streams' clips ([S][C][pitch], grown on demand as the images are); the ratios' tables, each
	// [L][pitch] floats in device memory from the first stream that takes the ratio to the last that drops it; every stream's slot (-1: none)
	float *dClipRaw = nullptr;
	size_t clipRawCapacity = 0;
	struct ResampleSlot { ResampleShape shape{0, 0, 0, 0, 0}; float *taps = nullptr; int users = 0; };
	ResampleSlot resampleSlots[kResampleMaxRatios];
	std::vector<int> resampleSlot, streamResampleSlot, outResampleSlot, streamOutResampleSlot; // per stream, the slot of its whole-clip, its streaming, its output and its streaming output ratio (-1: none)
	// a device scratch that holds `need` floats, allocated with `room` more; true: it was replaced (the old one freed behind a synchronise).  workspace: counted in workspaceBytes()
	bool growScratch(float *&scratch, size_t &capacity, size_t need, size_t room, bool workspace);
	StreamParams *dParams = nullptr, *hParams = nullptr; // (hParams: pinned staging of uploadParams())
	float *dMapTable = nullptr;
	std::vector<float> hostMapTable;
	std::vector<float> seedCarryWp;

	template <typename T> T *devAlloc(size_t count);
	void devFree(void *p);
	// A stream's CARRIED state, the device half: every array that lets a stream continue from one call to the next, [S] rows each, named
	// ONCE in carriedArrays().  Allocation, moveStreamsFrom (so copyStateFrom) and the debug hooks read that list: add an array there.
	struct CarriedArray {
		void **ptr[2];          // where the array's pointer lives in `d` / the batch; ptr[1] set: double-buffered, two arrays
		const int *cur;         // ... and which half is current (d.histCur / d.carryCur)
		size_t rowBytes;        // one stream's row; the fp16 narrowing (halfState) is folded in here and nowhere else
		bool narrowed;          // ... for this array: its values are stored as half_t
		bool splitOnly;         // exists only with split computation
		size_t slack;           // allocation: bytes beyond the S rows
		bool zeroed;            // allocation: cleared (the others are written by reset() before they are read)
		int halves() const { return ptr[1] ? 2 : 1; }
		char *current() const { return static_cast<char *>(*ptr[cur ? *cur : 0]); }
	};
	// (in the order construct() allocates them; the debug selectors 0..3 are the first four; [kHistBase, kStFreq) are the double-buffered
	// ones, each of which takes two of kMoveStreams' segments; from kPendIn: split computation only)
	enum { kStInput, kStPrev, kStOut, kStEnergy, kHist, kHistBase, kCarrySum, kCarryWp, kCarryBase, kStFreq, kPendIn, kPendPrev, kCarriedArrays };
	static_assert(kCarriedArrays + (kStFreq - kHistBase) <= kMoveSegs, "moveStreamsFrom: too many state arrays for one kMoveStreams launch");
	std::array<CarriedArray, kCarriedArrays> carriedArrays();
	void allocateCarried(int first, int last);
	// ... and the host half: sched, params, pend, lastSteps, lastStarts, histBase, carryBase, lastHop
	void clearHostRow(int s);                             // reset() of one stream: the random engine stays (seedAfterDroppedBlock)
	void takeHostRow(const Batch &o, int from, int to);   // moveStreamsFrom of one stream
	void growMapTable(int pitch); // the frequency-map table to a longer row pitch: every row keeps its knots
	void uploadMapTable();
	// debug hooks: `rows` rows of `len` stored values, devPitch values apart on the device, to (set == false) or from packed floats on the host
	void debugCopy(bool set, void *device, float *host, size_t rows, size_t len, size_t devPitch, bool narrowed, bool root);
	void debugCarry(bool set, int stream, float *sums, float *products);
	struct StatePlane { char *row; size_t values; bool narrowed, root; };
	StatePlane statePlane(int stream, int which); // selector -> the stream's row, its length, stored in fp16?, stored as the square root?
	// construct() in its order
	void createStreamsAndEvents();
	void readSwitches(const FftPlan &plan);
	void uploadConstantTables();
	void allocateCarriedState();
	void allocateCallTables();
	void initHostRows(long seed);
	void allocateSplitTables();
	void construct(const FftPlan &plan, long seed);
	void uploadParams();
	void allocateWorkspace();
	template <typename F> void timed(double &acc, F &&f);
};

// error plumbing for the C ABI
struct Error : std::exception {
	std::string msg;
	bool device; // true: a HIP runtime call failed (SMST_ERR_DEVICE); false: a bad argument / state (SMST_ERR_INVALID)
	explicit Error(std::string m, bool deviceError = false) : msg(std::move(m)), device(deviceError) {}
	const char *what() const noexcept override { return msg.c_str(); }
};

// up/down reduced by their gcd, then checked against the limits of include/smst.h, "Resample"; Error, the limit in its message, where one is missed
void resampleReduce(int &up, int &down);

} // namespace smst
