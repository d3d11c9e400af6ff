// C ABI (include/smst.h) over smst::Batch.  Host-memory calls are staged through device buffers owned by the
// handle; device-memory calls go straight to the engine.
#include "../../include/smst.h"
#include "smst_engine.h"
#include <cstdio>
#include <mutex>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

using smst::Batch;

static thread_local std::string g_lastError;

// Memory a handle (or one call of a debug hook) owns: `cap` elements of T in device memory or in pinned host memory, released in the
// destructor.  The owner selects the device first (hipSetDevice) wherever it frees or allocates.
template <typename T, bool Pinned, size_t Slack = 0> struct Buffer {
	T *p = nullptr;
	size_t cap = 0;
	Buffer() {}
	Buffer(const Buffer &) = delete;
	Buffer &operator=(const Buffer &) = delete;
	~Buffer() { release(); }
	operator T *() const { return p; }
	void release() {
		if (p) { if (Pinned) hipHostFree(p); else hipFree(p); }
		p = nullptr;
		cap = 0;
	}
	// exactly n elements, the contents undefined; what: the buffer's name in the error
	void allocate(size_t n, const char *what) {
		release();
		const hipError_t err = Pinned ? hipHostMalloc(reinterpret_cast<void **>(&p), n*sizeof(T), hipHostMallocDefault) : hipMalloc(reinterpret_cast<void **>(&p), n*sizeof(T));
		if (err != hipSuccess) throw smst::Error(std::string(Pinned ? "hipHostMalloc (" : "hipMalloc (") + what + ") failed", true);
		cap = n;
	}
	// at least `need` elements (the contents are not kept); a growth is one event of `allocs` and takes need/8 + Slack elements more
	void ensure(size_t need, int device, long long &allocs, const char *what) {
		if (need <= cap) return;
		++allocs;
		hipSetDevice(device);
		allocate(need + need/8 + Slack, what);
	}
};
// the two growth formulas: float staging need + need/8 + 1024 elements, raw PCM frames need + need/8 + 4096 bytes
typedef Buffer<float, false, 1024> DeviceFloats;
typedef Buffer<float, true, 1024> PinnedFloats;
typedef Buffer<unsigned char, false, 4096> DeviceBytes;
typedef Buffer<unsigned char, true, 4096> PinnedBytes;

static size_t pcmOversBytes(int streams) { return (size_t)2*streams*sizeof(unsigned); }
static void checkDitherMode(int mode) {
	if (mode != SMST_DITHER_NONE && mode != SMST_DITHER_TPDF && mode != SMST_DITHER_TPDF_HP) throw smst::Error("unknown dither mode (SMST_DITHER_NONE, _TPDF or _TPDF_HP)");
}
static void checkPcmLevel(int mode, float gain, float ceiling) {
	if (mode != SMST_LEVEL_FIXED && mode != SMST_LEVEL_PROTECT && mode != SMST_LEVEL_NORMALISE) throw smst::Error("unknown level mode (SMST_LEVEL_FIXED, _PROTECT or _NORMALISE; smst_batch_set_pcm_loudness sets _LOUDNESS)");
	if (!std::isfinite(gain)) throw smst::Error("level: the gain is not finite");
	if (mode == SMST_LEVEL_PROTECT && !(gain > 0)) throw smst::Error("level: SMST_LEVEL_PROTECT needs a gain above 0");
	if (mode != SMST_LEVEL_FIXED && !(std::isfinite(ceiling) && ceiling > 0)) throw smst::Error("level: the whole-clip modes need a finite ceiling above 0");
}

// The output side of a batch's frame-format calls: what the setters set per stream, and what the conversion kernels count and meter.  A call's
// share of it travels in the call's table (smst_pcm_tables.h): fill() writes it there.  The owner has selected the device wherever HIP is called.
struct PcmOutState {
	int S = 0, C = 0;
	// dither of the int16 / int24 output (smst_batch_set_pcm_dither): the mode, the seed, its hash and the frame counter
	struct Dither { int mode = SMST_DITHER_NONE; long long seed = 0; unsigned h = 0; unsigned long long frames = 0; };
	// level (smst_batch_set_pcm_level): the mode, the gain and the ceiling; the batch is a levelled one from the first set on
	struct Level { int mode = SMST_LEVEL_FIXED; float gain = 1.0f, ceiling = 1.0f; };
	// ... and, for a stream in SMST_LEVEL_LOUDNESS (smst_batch_set_pcm_loudness), the target, the sample rate and the table entry made of them
	struct Loud { double target = 0, sampleRate = 0; smst::LoudEntry entry{}; };
	std::vector<Dither> dither;
	std::vector<Level> level;
	std::vector<Loud> loud;
	std::vector<float> loudWeights; // [C], the batch's
	// the true-peak flag (smst_batch_set_pcm_true_peak): a setting of its own beside the stream's mode, which the two setters above leave as
	// it is; the first stream that gets it makes the batch a levelled one
	std::vector<unsigned char> truePeak;
	// the limiter flag (smst_batch_set_pcm_limiter): likewise; it acts in SMST_LEVEL_PROTECT and _LOUDNESS only (smst::pcmLimited)
	std::vector<unsigned char> limiter;
	// the meter flag (smst_batch_set_pcm_loudness_range): likewise, with the rate -- and the entry made of it -- that a stream outside
	// SMST_LEVEL_LOUDNESS is measured at; the caps on the two maxima (smst_batch_set_pcm_loudness_caps) in LUFS, +inf: none
	struct Meter { unsigned char on = 0; double sampleRate = 0; smst::LoudEntry entry{}; double capMomentary = INFINITY, capShortTerm = INFINITY; };
	std::vector<Meter> meter;
	// the stream limiter (smst_batch_set_pcm_stream_limiter; include/smst.h, "Stream limiter"): the setting and its ceiling, and which of the
	// stream's two carried lines the next call reads.  The lines -- both sets in one buffer, sized for the lookahead they were allocated at --
	// and the two meter words per stream exist from the first setter call with `on`; the need and r rows of a call grow on demand, as the
	// images do.  streamLimitView: where the kernels find all of that (smst::PcmStreamLimit).  truePeak: the stream's true-peak flag
	// (smst_batch_set_pcm_stream_limiter_true_peak), inert while `on` is 0; the lines it carries -- both sets in a buffer of their own, sized
	// as the others are -- exist from the first setter call with the flag on
	struct StreamLimit { unsigned char on = 0, set = 0, truePeak = 0; float ceiling = 1.0f; };
	std::vector<StreamLimit> streamLimit;
	DeviceFloats dLimitLines, dLimitRows, dLimitTruePeakLines;
	Buffer<int, false> dLimitMeters;
	int limitLinesH = 0, limitTruePeakLinesH = 0;
	smst::PcmStreamLimit streamLimitView;
	std::vector<int> hLimitMeters;
	// the stream meter (smst_batch_set_pcm_stream_meter; include/smst.h, "Stream meter"): the setting, the entry made of its rate, the frames
	// emitted for the stream since the clear (T) and the most that are metered (cap = maxSubBlocks*h).  The device side -- configurations,
	// carried state, histories of meterPitch sub-blocks per channel, a reading's scratch and tables -- exists from the first setter call with
	// `on`.  streamMeterView: where the kernels find it (smst::PcmStreamMeter)
	struct StreamMeter { unsigned char on = 0; double sampleRate = 0; int maxSub = 0; long long frames = 0, cap = 0; smst::LoudEntry entry{}; };
	std::vector<StreamMeter> streamMeter;
	Buffer<smst::StreamMeterConfig, false> dMeterConfig;
	Buffer<double, false> dMeterState, dMeterSub, dMeterRead;
	Buffer<double, false, 1024> dMeterScan;    // the chunk-scan form's scratch: grows on demand, as the images do
	Buffer<float, false> dMeterFrames;
	Buffer<int, false> dMeterWords;
	Buffer<unsigned char, false> dMeterTables; // a reading's: [2S] ClipSeg, [S] LoudEntry, [kMaxChannels] weights
	int meterPitch = 0;
	const double *meterReadZ = nullptr, *meterReadSt = nullptr;
	smst::PcmStreamMeter streamMeterView;
	bool levelled = false;
	// overs ([S][2]: clamped, NaN): the kernels add to them, takeOvers() reads and clears them; the meter words (smst::PcmMeters)
	Buffer<unsigned, false> dOvers;
	Buffer<int, false> dMeters;
	std::vector<unsigned> hOvers;
	std::vector<int> hMeters;
	std::vector<unsigned char> wholeClip, limited, metered; // clipModes()' arrays
	std::vector<int> loudHop;

	void create(int streams, int channels) {
		S = streams; C = channels;
		const smst::PcmMeters meters(S);
		dither.assign((size_t)S, Dither());
		level.assign((size_t)S, Level());
		loud.assign((size_t)S, Loud());
		loudWeights.assign((size_t)C, 1.0f);
		truePeak.assign((size_t)S, 0);
		limiter.assign((size_t)S, 0);
		meter.assign((size_t)S, Meter());
		streamLimit.assign((size_t)S, StreamLimit());
		streamMeter.assign((size_t)S, StreamMeter());
		metered.assign((size_t)S, 0);
		wholeClip.assign((size_t)S, 0);
		limited.assign((size_t)S, 0);
		loudHop.assign((size_t)S, 0);
		hOvers.assign((size_t)2*S, 0u);
		dOvers.allocate((size_t)2*S, "PCM overs");
		if (hipMemset(dOvers, 0, pcmOversBytes(S)) != hipSuccess) throw smst::Error("hipMemset (PCM overs) failed", true);
		hMeters.resize(meters.words());
		meters.start(hMeters.data());
		dMeters.allocate(meters.words(), "PCM level");
		if (hipMemcpy(dMeters, hMeters.data(), meters.bytes(), hipMemcpyHostToDevice) != hipSuccess) throw smst::Error("hipMemcpy (PCM level) failed", true);
	}
	size_t workspaceBytes() const {
		return (dOvers ? pcmOversBytes(S) : 0) + (dMeters ? smst::PcmMeters(S).bytes() : 0) + (dLimitLines.cap + dLimitRows.cap + dLimitTruePeakLines.cap)*sizeof(float) + dLimitMeters.cap*sizeof(int) +
		       dMeterConfig.cap*sizeof(smst::StreamMeterConfig) + (dMeterState.cap + dMeterSub.cap + dMeterRead.cap + dMeterScan.cap)*sizeof(double) + dMeterFrames.cap*sizeof(float) +
		       dMeterWords.cap*sizeof(int) + dMeterTables.cap;
	}

	// f(s) for the streams that `stream` names: -1 is every one
	template <typename F> void forStreams(int stream, F f) {
		if (stream < -1 || stream >= S) throw smst::Error("stream index out of range");
		for (int s = stream < 0 ? 0 : stream; s < (stream < 0 ? S : stream + 1); ++s) f(s);
	}
	void setDither(int stream, int mode, long long seed) {
		checkDitherMode(mode);
		forStreams(stream, [&](int s) {
			Dither &d = dither[s];
			d.mode = mode;
			d.seed = stream < 0 ? (long long)((unsigned long long)seed + (unsigned long long)s) : seed;
			d.h = smst::pcmDitherHash(d.seed);
			d.frames = 0;
		});
	}
	void setLevel(int stream, int mode, float gain, float ceiling) {
		checkPcmLevel(mode, gain, ceiling);
		forStreams(stream, [&](int s) { level[s] = Level{mode, gain, ceiling}; });
		levelled = true;
	}
	void setLoudness(int stream, double targetLufs, float ceiling, double sampleRate) {
		if (!std::isfinite(targetLufs)) throw smst::Error("loudness: the target is not finite");
		if (!(ceiling > 0)) throw smst::Error("loudness: the ceiling is not above 0 (+inf: no limit)");
		if (!(std::isfinite(sampleRate) && sampleRate > 0)) throw smst::Error("loudness: the sample rate is not finite or not above 0");
		Loud l;
		l.target = targetLufs; l.sampleRate = sampleRate;
		if (!smst::loudEntryOf(sampleRate, targetLufs, l.entry)) throw smst::Error("loudness: the sample rate gives a 100-ms step of fewer than " + std::to_string(smst::kLoudChunk) + " samples (or is beyond 1e9)");
		forStreams(stream, [&](int s) {
			level[s] = Level{SMST_LEVEL_LOUDNESS, 1.0f, ceiling};
			loud[s] = l;
		});
		levelled = true;
	}
	void setTruePeak(int stream, int on) {
		forStreams(stream, [&](int s) { truePeak[s] = on ? 1 : 0; });
		if (on) levelled = true;
	}
	bool anyTruePeak() const {
		if (levelled) for (unsigned char on : truePeak) if (on) return true;
		return false;
	}
	void setLimiter(int stream, int on) {
		forStreams(stream, [&](int s) { limiter[s] = on ? 1 : 0; });
		if (on) levelled = true;
	}
	// The stream limiter's lines for the engine's lookahead H, every one cleared: allocated where they are missing or were made for another H
	// (the caller has synchronised the batch then: a call in flight reads the lines it was issued with)
	void prepareStreamLimitLines(Batch &e) {
		const int H = e.limiterLookahead();
		if (!dLimitLines || limitLinesH != H) {
			const size_t set = smst::pcmStreamLimitSetFloats(S, C, H);
			dLimitLines.allocate(2*set, "stream limiter lines");
			limitLinesH = H;
			for (int k = 0; k < 2; ++k) {
				streamLimitView.need[k] = dLimitLines + k*set;
				streamLimitView.frames[k] = dLimitLines + k*set + (size_t)S*4*H;
			}
			streamLimitView.H = H;
			dLimitRows.release(); // (their pitch depends on H: the next limited call grows them)
		}
		if (dLimitTruePeakLines && limitTruePeakLinesH != H) allocateStreamLimitTruePeakLines(e);
		if (!dLimitMeters) {
			dLimitMeters.allocate((size_t)2*S, "stream limiter meters");
			hLimitMeters.assign((size_t)2*S, 0);
			if (hipMemsetAsync(dLimitMeters, 0, (size_t)2*S*sizeof(int), e.stream()) != hipSuccess) throw smst::Error("hipMemsetAsync (stream limiter meters) failed", true);
		}
		streamLimitView.meters = dLimitMeters;
		streamLimitView.window = e.limiterWindow();
		clearStreamLimitLines(e, -1);
	}
	// The lines of the true-peak flag for the engine's lookahead H, as +0.0: allocated where they are missing or were made for another H (no
	// call in flight reads them then: the lookahead's setter has synchronised, and before the first flag no call knows them)
	void allocateStreamLimitTruePeakLines(Batch &e) {
		const int H = e.limiterLookahead();
		const size_t set = smst::pcmStreamLimitTruePeakSetFloats(S, C, H);
		dLimitTruePeakLines.allocate(2*set, "stream limiter true-peak lines");
		limitTruePeakLinesH = H;
		for (int k = 0; k < 2; ++k) streamLimitView.truePeakFrames[k] = dLimitTruePeakLines + k*set;
		if (hipMemsetAsync(dLimitTruePeakLines, 0, 2*set*sizeof(float), e.stream()) != hipSuccess) throw smst::Error("hipMemsetAsync (stream limiter true-peak lines) failed", true);
	}
	// need <- 1, frames <- +0.0 for the stream (-1: every one), in the batch's stream order
	void clearStreamLimitLines(Batch &e, int stream) {
		if (!dLimitLines) return;
		if (hipSetDevice(e.device()) != hipSuccess) throw smst::Error("hipSetDevice failed", true);
		smst::launchPcmLimitClear(streamLimitView, S, C, stream, e.stream());
		for (int s = stream < 0 ? 0 : stream; s < (stream < 0 ? S : stream + 1); ++s) streamLimit[s].set = 0;
	}
	void setStreamLimiter(Batch &e, int stream, int on, float ceiling) {
		if (!(ceiling > 0)) throw smst::Error("stream limiter: the ceiling is NaN or not above 0 (+inf: no limit)");
		forStreams(stream, [](int) {}); // (refused before anything is allocated)
		if (on) {
			if (hipSetDevice(e.device()) != hipSuccess) throw smst::Error("hipSetDevice failed", true);
			if (!e.limiterWindow()) e.prepareLimiter(); // (the window goes to the device here, not in a call)
			if (!dLimitLines) prepareStreamLimitLines(e);
			levelled = true;
		}
		forStreams(stream, [&](int s) { streamLimit[s].on = on ? 1 : 0; streamLimit[s].ceiling = ceiling; });
		clearStreamLimitLines(e, stream);
	}
	// The flag beside the setting: the delay of the stream(s) changes, so their lines are cleared, on or off.  The first call with `on`
	// allocates the flag's lines (and, where the setting has never been on, what that carries: a flagged stream's need line is one of those)
	void setStreamLimiterTruePeak(Batch &e, int stream, int on) {
		forStreams(stream, [](int) {}); // (refused before anything is allocated)
		if (on) {
			if (hipSetDevice(e.device()) != hipSuccess) throw smst::Error("hipSetDevice failed", true);
			if (!e.limiterWindow()) e.prepareLimiter(); // (the window goes to the device here, not in a call)
			if (!dLimitLines) prepareStreamLimitLines(e);
			if (!dLimitTruePeakLines || limitTruePeakLinesH != e.limiterLookahead()) allocateStreamLimitTruePeakLines(e);
		}
		forStreams(stream, [&](int s) { streamLimit[s].truePeak = on ? 1 : 0; });
		clearStreamLimitLines(e, stream);
	}
	bool anyStreamLimit() const {
		if (levelled) for (const StreamLimit &l : streamLimit) if (l.on) return true;
		return false;
	}
	// the largest count of a stream that a streaming call of these counts limits: the setting, a FIXED level and frames; truePeak (may be
	// null): the largest among those of them that have the true-peak flag
	int mostStreamLimited(const int *n, int *truePeak = nullptr) const {
		int most = 0, flagged = 0;
		if (anyStreamLimit()) for (int s = 0; s < S; ++s) if (streamLimit[s].on && level[s].mode == SMST_LEVEL_FIXED) {
			most = std::max(most, n[s]);
			if (streamLimit[s].truePeak) flagged = std::max(flagged, n[s]);
		}
		if (truePeak) *truePeak = flagged;
		return most;
	}
	// ... and among those without the flag
	int mostStreamLimitedPlain(const int *n) const {
		int most = 0;
		if (anyStreamLimit()) for (int s = 0; s < S; ++s) if (streamLimit[s].on && !streamLimit[s].truePeak && level[s].mode == SMST_LEVEL_FIXED) most = std::max(most, n[s]);
		return most;
	}
	int streamLimitLatency(const Batch &e, int s) const {
		return streamLimit[s].on ? 2*e.limiterLookahead() + (streamLimit[s].truePeak ? SMST_STREAM_LIMITER_TRUE_PEAK_DELAY : 0) : 0;
	}
	// the rows of a call whose longest limited count is `most`, before the engine is called (a growth frees, which synchronises the device)
	void ensureStreamLimitRows(Batch &e, int most, long long &allocs) {
		const long long lead = (long long)4*limitLinesH, pitch = ((long long)most + 3)/4*4;
		dLimitRows.ensure((size_t)S*size_t(lead + 2*pitch), e.device(), allocs, "stream limiter rows");
		// laid out for the capacity, so that a buffer that has served a longer call serves this one with the pitches of that one
		const long long per = (long long)(dLimitRows.cap/(size_t)S);
		streamLimitView.rPitch = (per - lead)/2/4*4;
		streamLimitView.needPitch = lead + streamLimitView.rPitch;
		streamLimitView.needRow = dLimitRows;
		streamLimitView.rRow = dLimitRows + (size_t)S*size_t(streamLimitView.needPitch);
	}
	// after a call that limited: the streams that took part read the other set next time
	void advanceStreamLimit(const int *n) {
		for (int s = 0; s < S; ++s) if (streamLimit[s].on && level[s].mode == SMST_LEVEL_FIXED && n[s] > 0) streamLimit[s].set ^= 1;
	}
	void takeStreamLimiter(float *minGain, long long *limitedFrames) {
		for (int s = 0; s < S; ++s) {
			if (minGain) minGain[s] = 1.0f;
			if (limitedFrames) limitedFrames[s] = 0;
		}
		if (!dLimitMeters) return; // (the setting was never on: nothing has limited)
		if (hipMemcpy(hLimitMeters.data(), dLimitMeters, (size_t)2*S*sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) throw smst::Error("hipMemcpy (stream limiter meters) failed", true);
		if (hipMemset(dLimitMeters, 0, (size_t)2*S*sizeof(int)) != hipSuccess) throw smst::Error("hipMemset (stream limiter meters) failed", true);
		for (int s = 0; s < S; ++s) {
			const int bits = 0x3f800000 - hLimitMeters[s];
			if (minGain) std::memcpy(minGain + s, &bits, sizeof(float));
			if (limitedFrames) limitedFrames[s] = (long long)(unsigned)hLimitMeters[(size_t)S + s]; // (the count wraps as an unsigned 32-bit word does)
		}
	}
	// Stream meter.  The doubles of a reading's scratch: the gate stage's meters and block powers, the range stage's, the reading's words
	static size_t meterReadDoubles(int S, int pitch) { return (size_t)2*S + (S + 1)/2 + (size_t)S*pitch + smst::loudRangeDoubles(S, pitch) + (size_t)3*S; }
	static size_t meterTableBytes(int S) { return (size_t)2*S*sizeof(smst::ClipSeg) + (size_t)S*sizeof(smst::LoudEntry) + smst::kMaxChannels*sizeof(float); }
	static smst::StreamMeterConfig meterConfig(const StreamMeter &m) {
		smst::StreamMeterConfig cfg{};
		cfg.k = m.entry.k;
		for (int i = 0; i < 16; ++i) cfg.Ac[i] = m.entry.Ac[i];
		cfg.h = m.entry.h; cfg.on = m.on; cfg.cap = int(m.cap);
		return cfg;
	}
	void setStreamMeter(int device, hipStream_t st, int stream, int on, double sampleRate, int maxSubBlocks, long long &allocs) {
		forStreams(stream, [](int) {}); // (refused before anything is allocated)
		StreamMeter m;
		if (on) {
			if (!(std::isfinite(sampleRate) && sampleRate > 0)) throw smst::Error("stream meter: the sample rate is not finite or not above 0");
			if (!smst::loudEntryOf(sampleRate, 0.0, m.entry)) throw smst::Error("stream meter: the sample rate gives a 100-ms step of fewer than " + std::to_string(smst::kLoudChunk) + " samples (or is beyond 1e9)");
			if (maxSubBlocks < 1) throw smst::Error("stream meter: maxSubBlocks is below 1");
			if ((long long)maxSubBlocks*m.entry.h >= (1LL << 31)) throw smst::Error("stream meter: maxSubBlocks 100-ms sub-blocks are 2^31 frames or more at this rate");
			if (dMeterState && maxSubBlocks > meterPitch)
				throw smst::Error("stream meter: maxSubBlocks is above " + std::to_string(meterPitch) + ", what the batch's histories were allocated for by the first call with the setting on");
			m.on = 1; m.sampleRate = sampleRate; m.maxSub = maxSubBlocks; m.cap = (long long)maxSubBlocks*m.entry.h;
			m.entry.meter = 1;
		}
		if (hipSetDevice(device) != hipSuccess) throw smst::Error("hipSetDevice failed", true);
		if (on && !dMeterState) {
			++allocs;
			meterPitch = maxSubBlocks;
			dMeterConfig.allocate((size_t)S, "stream meter configurations");
			dMeterState.allocate((size_t)S*C*smst::kStreamMeterDoubles, "stream meter state");
			dMeterFrames.allocate((size_t)S*C*smst::kStreamMeterLine, "stream meter frames");
			dMeterWords.allocate((size_t)2*S, "stream meter words");
			dMeterSub.allocate((size_t)S*C*meterPitch, "stream meter histories");
			dMeterRead.allocate(meterReadDoubles(S, meterPitch), "stream meter reading");
			dMeterTables.allocate(meterTableBytes(S), "stream meter tables");
			streamMeterView.config = dMeterConfig; streamMeterView.state = dMeterState; streamMeterView.frames = dMeterFrames;
			streamMeterView.words = dMeterWords; streamMeterView.sub = dMeterSub; streamMeterView.maxSub = meterPitch;
			const smst::StreamMeterConfig off{};
			smst::launchPcmStreamMeterClear(streamMeterView, S, C, -1, &off, st);
		}
		forStreams(stream, [&](int s) { streamMeter[s] = m; });
		if (dMeterState) {
			const smst::StreamMeterConfig cfg = meterConfig(m);
			smst::launchPcmStreamMeterClear(streamMeterView, S, C, stream, &cfg, st);
		}
	}
	// nothing metered, the settings kept, for the stream (-1: every one), in the batch's stream order
	void clearStreamMeter(int device, hipStream_t st, int stream) {
		for (int s = stream < 0 ? 0 : stream; s < (stream < 0 ? S : stream + 1); ++s) streamMeter[s].frames = 0;
		if (!dMeterState) return;
		if (hipSetDevice(device) != hipSuccess) throw smst::Error("hipSetDevice failed", true);
		smst::launchPcmStreamMeterClear(streamMeterView, S, C, stream, nullptr, st);
	}
	bool streamMeterHolds() const {
		for (const StreamMeter &m : streamMeter) if (m.frames > 0) return true;
		return false;
	}
	// the largest count of a stream that a streaming call of these counts meters (a full meter takes none of them)
	int mostStreamMetered(const int *n) const {
		int most = 0;
		if (dMeterState) for (int s = 0; s < S; ++s) if (streamMeter[s].on && streamMeter[s].frames < streamMeter[s].cap) most = std::max(most, n[s]);
		return most;
	}
	// the chunk-scan form's scratch for a call whose longest metered count is `most`, before the engine is called (a growth frees, which
	// synchronises the device)
	void ensureStreamMeterScan(int device, int most, int form, long long &allocs) {
		if (most < 1 || !smst::streamMeterScans(most, form)) return;
		const int chunks = smst::streamMeterChunksOf(most);
		dMeterScan.ensure(smst::streamMeterScanDoubles(S, C, chunks), device, allocs, "stream meter scan");
		streamMeterView.scan = dMeterScan;
		streamMeterView.maxChunks = int((dMeterScan.cap/((size_t)S*C) - 4)/6); // (laid out for the capacity: a buffer that has served a longer call serves this one)
	}
	// a call's update behind its output conversion, and the host's count of what the streams were handed
	// (dStarts, form: the test hook's -- where each stream's frames begin in its rows, and the update form forced)
	void meterStream(hipStream_t st, const float *image, long long imageSS, long long imageCS, const int *n, const int *dCounts, const int *dStarts = nullptr, int form = 0) {
		const int most = mostStreamMetered(n);
		if (most > 0) smst::launchPcmStreamMeter(image, imageSS, imageCS, dCounts, dStarts, S, C, most, streamMeterView, form, st);
		for (int s = 0; s < S; ++s) if (streamMeter[s].on && n[s] > 0) streamMeter[s].frames += n[s];
	}
	struct MeterReading { std::vector<double> Z, range, newest; std::vector<int> counts, rangeCounts, peaks; };
	// a reading, behind a synchronisation of the batch (false: the setting was never on -- nothing is defined)
	const double *readBlockPowers(int s) const { return meterReadZ + (size_t)s*meterPitch; }  // (of the newest reading, device)
	const double *readShortPowers(int s) const { return meterReadSt + (size_t)s*meterPitch; }
	bool readStreamMeter(hipStream_t st, MeterReading &r) {
		r.Z.assign((size_t)S, 0.0); r.range.assign((size_t)4*S, 0.0); r.newest.assign((size_t)2*S, 0.0);
		r.counts.assign((size_t)2*S, 0); r.rangeCounts.assign((size_t)2*S, 0); r.peaks.assign((size_t)2*S, 0);
		if (!dMeterState) return false;
		auto hip = [&](hipError_t err) { if (err != hipSuccess) throw smst::Error(std::string("stream meter reading: ") + hipGetErrorString(err), true); };
		std::vector<unsigned char> tables(meterTableBytes(S));
		smst::ClipSeg *segs = reinterpret_cast<smst::ClipSeg *>(tables.data());
		smst::LoudEntry *entries = reinterpret_cast<smst::LoudEntry *>(segs + 2*S);
		float *weights = reinterpret_cast<float *>(entries + S);
		for (int s = 0; s < S; ++s) {
			const StreamMeter &m = streamMeter[s];
			segs[2*s] = smst::ClipSeg{0, 0, int(std::min(m.frames, m.cap)), 0};
			segs[2*s + 1] = smst::ClipSeg{0, 0, 0, 0};
			entries[s] = m.on ? m.entry : smst::LoudEntry{};
		}
		for (int k = 0; k < smst::kMaxChannels; ++k) weights[k] = k < C ? loudWeights[k] : 0.0f;
		hip(hipMemcpy(dMeterTables, tables.data(), tables.size(), hipMemcpyHostToDevice));
		const smst::ClipSeg *dSegs = reinterpret_cast<const smst::ClipSeg *>(dMeterTables.p);
		const smst::LoudEntry *dEntries = reinterpret_cast<const smst::LoudEntry *>(dSegs + 2*S);
		const float *dWeights = reinterpret_cast<const float *>(dEntries + S);
		smst::LoudScratch w{};
		double *p = dMeterRead;
		w.Z = p; p += S;
		w.counts = reinterpret_cast<int *>(p); p += S;
		w.gain = reinterpret_cast<float *>(p); p += (S + 1)/2;
		w.z = p; p += (size_t)S*meterPitch;
		w.sub = dMeterSub; w.maxSub = meterPitch; w.maxChunks = 0;
		const smst::LoudRangeScratch range = smst::loudRangeAt(p, S, meterPitch);
		p += smst::loudRangeDoubles(S, meterPitch);
		const smst::StreamMeterReading out{reinterpret_cast<int *>(p), p + S};
		meterReadZ = w.z; meterReadSt = range.st;
		smst::launchPcmStreamMeterRead(dSegs, dEntries, dWeights, S, C, streamMeterView, w, range, out, st);
		hip(hipGetLastError());
		hip(hipStreamSynchronize(st));
		hip(hipMemcpy(r.Z.data(), w.Z, (size_t)S*sizeof(double), hipMemcpyDeviceToHost));
		hip(hipMemcpy(r.counts.data(), w.counts, (size_t)2*S*sizeof(int), hipMemcpyDeviceToHost));
		hip(hipMemcpy(r.range.data(), range.meters, (size_t)4*S*sizeof(double), hipMemcpyDeviceToHost));
		hip(hipMemcpy(r.rangeCounts.data(), range.counts, (size_t)2*S*sizeof(int), hipMemcpyDeviceToHost));
		hip(hipMemcpy(r.peaks.data(), out.peaks, (size_t)2*S*sizeof(int), hipMemcpyDeviceToHost));
		hip(hipMemcpy(r.newest.data(), out.newest, (size_t)2*S*sizeof(double), hipMemcpyDeviceToHost));
		return true;
	}
	void setLoudnessRange(int stream, int on, double sampleRate) {
		Meter m;
		if (on) {
			if (!(std::isfinite(sampleRate) && sampleRate > 0)) throw smst::Error("loudness range: the sample rate is not finite or not above 0");
			if (!smst::loudEntryOf(sampleRate, 0.0, m.entry)) throw smst::Error("loudness range: the sample rate gives a 100-ms step of fewer than " + std::to_string(smst::kLoudChunk) + " samples (or is beyond 1e9)");
		}
		forStreams(stream, [&](int s) {
			meter[s].on = on ? 1 : 0;
			if (on) { meter[s].sampleRate = sampleRate; meter[s].entry = m.entry; }
		});
		if (on) levelled = true;
	}
	void setLoudnessCaps(int stream, double maxMomentaryLufs, double maxShortTermLufs) {
		for (double cap : {maxMomentaryLufs, maxShortTermLufs}) if (std::isnan(cap) || cap == -INFINITY) throw smst::Error("loudness caps: a cap is NaN or -inf (+inf: none)");
		forStreams(stream, [&](int s) { meter[s].capMomentary = maxMomentaryLufs; meter[s].capShortTerm = maxShortTermLufs; });
		if (std::isfinite(maxMomentaryLufs) || std::isfinite(maxShortTermLufs)) levelled = true;
	}
	bool capped(int s) const { return std::isfinite(meter[s].capMomentary) || std::isfinite(meter[s].capShortTerm); }
	// The loudness entry a call's table carries for the stream.  A stream in SMST_LEVEL_LOUDNESS is measured at its mode's rate, metered where it
	// has the flag or a finite cap, and capped; another one is measured at the meter flag's rate where it has the flag -- a cap is inert there
	smst::LoudEntry loudEntry(int s) const {
		static const auto power = [](double lufs) { return std::isfinite(lufs) ? std::pow(10.0, (lufs + 0.691)/10) : double(INFINITY); };
		if (level[s].mode == SMST_LEVEL_LOUDNESS) {
			smst::LoudEntry e = loud[s].entry;
			e.meter = meter[s].on || capped(s);
			e.Pm = power(meter[s].capMomentary); e.Ps = power(meter[s].capShortTerm);
			return e;
		}
		if (!meter[s].on) return smst::LoudEntry{};
		smst::LoudEntry e = meter[s].entry;
		e.meter = 1;
		return e;
	}
	unsigned flags(int s) const { return (truePeak[s] ? smst::kPcmFlagTruePeak : 0u) | (limiter[s] ? smst::kPcmFlagLimiter : 0u); }
	// a call's level entry: a FIXED stream with the stream limiter's setting carries that limiter's ceiling in the word its mode does not use,
	// the setting in bit 2 of the flags, the set of lines the call reads in bit 3 and the setting's true-peak flag in bit 4
	smst::PcmLevel levelEntry(int s) const {
		const bool limit = streamLimit[s].on && level[s].mode == SMST_LEVEL_FIXED;
		const unsigned limitFlags = smst::kPcmFlagStreamLimiter | (streamLimit[s].set ? smst::kPcmFlagStreamLimitSet : 0u) | (streamLimit[s].truePeak ? smst::kPcmFlagStreamLimitTruePeak : 0u);
		return smst::PcmLevel{unsigned(level[s].mode), level[s].gain, limit ? streamLimit[s].ceiling : level[s].ceiling, flags(s) | (limit ? limitFlags : 0u)};
	}
	void setLoudnessWeights(const float *weights) {
		for (int c = 0; weights && c < C; ++c) if (!(std::isfinite(weights[c]) && weights[c] >= 0)) throw smst::Error("loudness: a channel weight is negative or not finite");
		if (streamMeterHolds()) throw smst::Error("loudness: a stream meter holds frames that were metered under the present weights (smst_batch_set_pcm_stream_meter clears it)");
		for (int c = 0; c < C; ++c) loudWeights[c] = weights ? weights[c] : 1.0f;
	}

	// whether a call of this format dithers: a stream has a mode, and the format has a step to dither
	bool dithers(int format) const {
		if (format != SMST_PCM_S16 && format != SMST_PCM_S24) return false;
		for (const Dither &d : dither) if (d.mode != SMST_DITHER_NONE) return true;
		return false;
	}
	bool anyLoudness() const {
		if (levelled) for (const Level &l : level) if (l.mode == SMST_LEVEL_LOUDNESS) return true;
		if (levelled) for (const Meter &m : meter) if (m.on) return true; // (measured whatever its mode)
		return false;
	}
	// A call's sections into its table's pinned copy `host` -> where the kernels find them in the device twin `dev`.  A call that dithers has
	// every stream's mode and hash, and its frame counter as the index of the call's first frame; a levelled batch's calls the streams' level
	// entries too (the dither entries then travel whether the call dithers or not) and, where a stream is measured (loudEntry), the loudness
	// entries and the channel weights
	smst::PcmOutCall fill(void *host, void *dev, const smst::PcmTableLayout &at, int format) const {
		smst::PcmOutCall call;
		const bool dithered = dithers(format);
		call.overs = dOvers;
		if (anyLoudness()) {
			for (int s = 0; s < S; ++s) at.loud(host)[s] = loudEntry(s);
			for (int k = 0; k < smst::kMaxChannels; ++k) at.weights(host)[k] = k < C ? loudWeights[k] : 0.0f;
			call.loud = at.loud(dev);
			call.loudWeights = at.weights(dev);
		}
		if (levelled) {
			for (int s = 0; s < S; ++s) at.level(host)[s] = levelEntry(s);
			call.level = smst::PcmMeters(S).io(at.level(dev), dMeters);
		}
		if (dithered || levelled) {
			for (int s = 0; s < S; ++s) at.dither(host)[s] = smst::PcmDither{unsigned(dither[s].mode), dither[s].h, unsigned(dither[s].frames), unsigned(dither[s].frames >> 32)};
			if (dithered) call.dither = at.dither(dev);
		}
		return call;
	}
	// What exact() needs on the host beside a call's view: which streams' gains come from their clip's peak (they decide whether kClipPeak
	// runs), h of the measured ones (whether the four passes do) and which of them are metered (whether kLoudRange does), the true-peak flags (whether kClipTruePeak does) and the streams
	// that are limited (whether the limiter's two passes do).  Null as the view's members are
	void clipModes(const smst::PcmOutCall &call, Batch::ClipIo &io) {
		bool anyLimited = false, anyMetered = false;
		for (int s = 0; s < S; ++s) {
			limited[s] = levelled && smst::pcmLimited(smst::PcmLevel{unsigned(level[s].mode), level[s].gain, level[s].ceiling, flags(s)});
			anyLimited = anyLimited || limited[s];
			wholeClip[s] = level[s].mode != SMST_LEVEL_FIXED;
			const smst::LoudEntry e = loudEntry(s);
			loudHop[s] = e.h;
			metered[s] = e.h > 0 && e.meter;
			anyMetered = anyMetered || metered[s];
		}
		io.pcm = call;
		io.wholeClip = call.level.table ? wholeClip.data() : nullptr;
		io.loudHop = call.loud ? loudHop.data() : nullptr;
		io.loudMeter = call.loud && anyMetered ? metered.data() : nullptr;
		io.truePeak = call.level.table && anyTruePeak() ? truePeak.data() : nullptr;
		io.limiter = call.level.table && anyLimited ? limited.data() : nullptr;
	}
	// after a call that emitted n[s] frames: the counters of the streams that have a mode move on, whatever the call's format
	void advance(const int *n) {
		for (int s = 0; s < S; ++s) if (dither[s].mode != SMST_DITHER_NONE && n[s] > 0) dither[s].frames += (unsigned long long)n[s];
	}
	// the takes: behind a synchronisation of the batch
	void takeOvers(long long *clamped, long long *nans) {
		if (!dOvers) throw smst::Error("this batch has no PCM over counters");
		if (hipMemcpy(hOvers.data(), dOvers, pcmOversBytes(S), hipMemcpyDeviceToHost) != hipSuccess) throw smst::Error("hipMemcpy (PCM overs) failed", true);
		if (hipMemset(dOvers, 0, pcmOversBytes(S)) != hipSuccess) throw smst::Error("hipMemset (PCM overs) failed", true);
		for (int s = 0; s < S; ++s) {
			if (clamped) clamped[s] = hOvers[2*s];
			if (nans) nans[s] = hOvers[2*s + 1];
		}
	}
	void takePeaks(float *peaks, float *gains) {
		const smst::PcmMeters meters(S);
		if (!dMeters) throw smst::Error("this batch has no PCM level meters");
		if (hipMemcpy(hMeters.data(), dMeters, meters.takeBytes(), hipMemcpyDeviceToHost) != hipSuccess) throw smst::Error("hipMemcpy (PCM level) failed", true);
		if (hipMemset(dMeters, 0, meters.clearBytes()) != hipSuccess) throw smst::Error("hipMemset (PCM level) failed", true);
		meters.taken(hMeters.data(), peaks, gains);
	}
};

// The input side of a batch's frame-format streaming calls where a stream has the setting of include/smst.h, "Stream resample": per stream the
// two 64-bit counters, which set of its two carried lines the next call reads and whether the line counts as cleared; the lines (both sets in
// one buffer), allocated by the first setter call with a ratio other than 1/1, and the raw image, which grows on demand as the images do.  The
// ratios, their tables and their slots are the engine's (Batch::setResample, streaming).  The owner has selected the device wherever HIP is called.
struct PcmStreamResampleState {
	struct Stream { long long fed = 0, made = 0; unsigned char set = 0, fresh = 1; };
	std::vector<Stream> stream;
	std::vector<int> counts; // the frames the engine gets from each stream in the newest call
	Buffer<float, false> dLines;
	DeviceFloats dRaw;
	size_t tableBytes = 0;   // of the call tables' device twins (both sets)
	void create(int S) { stream.assign((size_t)S, Stream()); counts.assign((size_t)S, 0); }
	size_t workspaceBytes() const { return (dLines.cap + dRaw.cap)*sizeof(float) + tableBytes; }
	// frames <- +0.0, fed = made = 0 for the stream (-1: every one): the next call reads zeros in the place of the line
	void clear(int stream_) {
		for (size_t s = stream_ < 0 ? 0 : size_t(stream_); s < (stream_ < 0 ? stream.size() : size_t(stream_) + 1); ++s) { stream[s].fed = stream[s].made = 0; stream[s].fresh = 1; }
	}
	static bool any(const Batch &e) {
		for (int s = 0; s < e.streams(); ++s) if (e.streamResampled(s)) return true;
		return false;
	}
	// k of a call that hands the stream n frames (fresh: as after a clear); Error where it does not fit an int
	long long framesOf(const Batch &e, int s, long long n, bool fresh) const {
		if (!e.streamResampled(s)) return n;
		const smst::ResampleShape &g = e.streamResampleShape(s);
		const long long fed = fresh ? 0 : stream[s].fed;
		if (n > (1LL << 40) || fed > (1LL << 62) - n) throw smst::Error("stream resample: stream " + std::to_string(s) + ": " + std::to_string(n) + " frames give the engine more than 2147483647 (k must fit an int)");
		const long long k = smst::streamResampleDue(fed + n - g.H, g.L, g.M) - smst::streamResampleDue(fed - g.H, g.L, g.M);
		if (k > 0x7fffffffLL) throw smst::Error("stream resample: stream " + std::to_string(s) + ": " + std::to_string(n) + " frames give the engine " + std::to_string(k) + ", more than 2147483647 (k must fit an int)");
		return k;
	}
};

// The output side of a batch's frame-format streaming calls where a stream has the setting of include/smst.h, "Stream output resample": per
// stream the 64-bit count of frames delivered since the clear, which set of its two carried lines the next call reads and whether the line
// counts as cleared; the lines (both sets in one buffer), allocated by the first setter call with a ratio other than 1/1, and the image of
// the delivered frames, which grows on demand as the images do.  The ratios, their tables and their slots are the engine's
// (Batch::setResample, kResampleStreamOut).  The owner has selected the device wherever HIP is called.
struct PcmStreamResampleOutState {
	struct Stream { long long delivered = 0; unsigned char set = 0, fresh = 1; };
	std::vector<Stream> stream;
	std::vector<int> render; // the frames the engine renders for each stream in the newest call: its E, or the call's own count
	Buffer<float, false> dLines;
	DeviceFloats dDelivered;
	size_t tableBytes = 0;   // of the call tables' device twins (both sets)
	void create(int S) { stream.assign((size_t)S, Stream()); render.assign((size_t)S, 0); }
	size_t workspaceBytes() const { return (dLines.cap + dDelivered.cap)*sizeof(float) + tableBytes; }
	// frames <- +0.0, delivered = 0 for the stream (-1: every one): the next call reads zeros in the place of the line
	void clear(int stream_) {
		for (size_t s = stream_ < 0 ? 0 : size_t(stream_); s < (stream_ < 0 ? stream.size() : size_t(stream_) + 1); ++s) { stream[s].delivered = 0; stream[s].fresh = 1; }
	}
	static bool any(const Batch &e) {
		for (int s = 0; s < e.streams(); ++s) if (e.streamOutResampled(s)) return true;
		return false;
	}
	// E of a call that delivers Nd frames to the stream (fresh: as after a clear); Error where it does not fit an int
	// (2*M <= 9*L: E < 4.5*Nd + 1, and delivered*M stays below 2^62)
	long long renderOf(const Batch &e, int s, long long Nd, bool fresh) const {
		if (!e.streamOutResampled(s)) return Nd;
		const smst::ResampleShape &g = e.streamOutResampleShape(s);
		const long long delivered = fresh ? 0 : stream[s].delivered;
		const std::string what = "stream out resample: stream " + std::to_string(s) + ": " + std::to_string(Nd) + " delivered frames";
		if (Nd > (1LL << 40)) throw smst::Error(what + " need more than 2147483647 rendered frames (E must fit an int)");
		if (delivered > (1LL << 52) - Nd) throw smst::Error(what + " take the stream beyond 2^52 delivered frames (smst_batch_set_pcm_stream_out_resample clears the count)");
		const long long E = smst::streamResampleOutDue(delivered + Nd, g.L, g.M) - smst::streamResampleOutDue(delivered, g.L, g.M);
		if (E > 0x7fffffffLL) throw smst::Error(what + " need " + std::to_string(E) + " rendered frames, more than 2147483647 (E must fit an int)");
		return E;
	}
	// render[s] of a call whose streams are delivered n[s] frames (a negative count: no part, the count itself) -> whether a stream of the
	// batch has the setting.  Every refusal of the output side, before anything has changed
	bool prepare(const Batch &e, const int *n) {
		if (!any(e)) return false;
		for (int s = 0; s < e.streams(); ++s) render[s] = n[s] < 0 ? n[s] : int(renderOf(e, s, n[s], stream[s].fresh != 0));
		return true;
	}
};

struct smst_batch {
	std::unique_ptr<Batch> engine;
	// host staging (SMST_MEM_HOST)
	DeviceFloats dIn, dOut;
	long long stagingAllocs = 0;
	// interleaved PCM (smst_batch_*_pcm): the raw frames as they cross PCIe, one device and one pinned host buffer per direction (bytes); the
	// planar image the engine works on is dIn / dOut above
	DeviceBytes dPcmIn, dPcmOut;
	PinnedBytes hPcmIn, hPcmOut;
	// The per-call table of the conversion kernels (smst::PcmTableLayout: the streams' frame counts, then the output side's entries) exists
	// twice, as the engine's per-call tables do: a device-memory call returns before its kernels have run.  out: where the call's output
	// conversion finds its entries in `dev` (PcmOutState::fill)
	struct PcmTable {
		Buffer<unsigned char, true> host;
		Buffer<unsigned char, false> dev;
		smst::PcmOutCall out;
		Buffer<unsigned char, true> resHost; // the input side's table of a call with a stream-resampled stream (smst::StreamResampleTableLayout),
		Buffer<unsigned char, false> resDev; // allocated -- both sets -- by the first setter call with a ratio other than 1/1
		Buffer<unsigned char, true> outResHost; // the output side's table of a call with a stream-out-resampled stream (smst::StreamResampleOutTableLayout),
		Buffer<unsigned char, false> outResDev; // allocated -- both sets -- by the first setter call with a ratio other than 1/1
		int mostLimitedPlain = 0, mostLimitedTruePeak = 0; // ... of one without and of one with the stream limiter's true-peak flag
		int mostLimited = 0; // the largest count of a stream that the call's output limits ("Stream limiter"); 0: the call launches what it did without the setting
		int mostDelivered = 0, deliveredLen = 1, outSpanPitch = 4; // "Stream output resample": the largest Nd of a stream with the setting (0: as mostLimited), the row length of the delivered image, what sizes the LDS
	};
	smst::TwoSets<PcmTable> pcmTables; // (smst_staging.h)
	PcmOutState pcmOut;
	PcmStreamResampleState pcmIn;
	PcmStreamResampleOutState pcmOutRes;
	~smst_batch() { if (engine) hipSetDevice(engine->device()); } // (the buffers above go behind it, the engine last)
};

struct smst_stretch {
	long seed = 0;
	int device = 0;
	std::unique_ptr<smst_batch> batch; // S = 1, created by configure/preset
	// parameters set before configure() survive it, as members of the reference object do
	float transposeFactor = 1, tonalityLimit = 0;
	bool transposeSet = false;
	float formantFactor = 1;
	bool formantComp = false;
	float formantBase = 0;
	std::vector<float> mapTable;
	// ---- pool membership (extension, include/smst.h group 3).  A member that is configured lives in slot `slot` of its group's engine and
	// owns no engine (`batch` is null); one that is not configured yet is only registered.  A handle that never meets a pool has none of this set.
	smst_pool *pool = nullptr;
	struct PoolGroup *group = nullptr;
	int slot = -1;
	bool pending = false; // a request of smst_process_begin that has not run yet
	const float *const *reqIn = nullptr;
	float *const *reqOut = nullptr;
	int reqIn_n = 0, reqOut_n = 0;
	int reqStatus = SMST_OK; // of the newest request (smst_process_end reports it)
	std::string reqError;
};

// One geometry (channels, block, interval, split) of a pool: ONE engine whose streams are the members' slots
struct PoolGroup {
	std::unique_ptr<smst_batch> batch;
	std::vector<smst_stretch *> slots; // the member in each slot, null = free
	std::vector<int> freeSlots;        // descending: the lowest free slot is taken first
	int used = 0;
	// per-run scratch, sized with the engine (nothing is allocated in a steady-state run)
	std::vector<int> nIn, nOut;
	std::vector<unsigned char> active;
	PinnedFloats hIn, hOut; // pinned staging: the members' planes gathered as [slot][channel][longest count]
};
struct smst_pool {
	int device = 0;
	std::vector<std::unique_ptr<PoolGroup>> groups;
	std::vector<smst_stretch *> members;
	long long engineCalls = 0; // Batch::process calls issued by smst_pool_run / smst_process_end
	long long allocEvents = 0; // group engines created / regrown, staging growth, plus the counts of engines that have been retired
};

#define SMST_TRY try {
#define SMST_CATCH \
	} catch (const smst::Error &e) { g_lastError = e.what(); return e.device ? SMST_ERR_DEVICE : SMST_ERR_INVALID; } \
	catch (const std::exception &e) { g_lastError = e.what(); return SMST_ERR_INVALID; }

static int fail(const char *msg) {
	g_lastError = msg;
	return SMST_ERR_INVALID;
}

// the planar staging image of one direction, [rows][len] floats
static void ensureStage(smst_batch *b, DeviceFloats &image, size_t need) { image.ensure(need, b->engine->device(), b->stagingAllocs, "staging"); }
// A call's counts as the staging side takes them: used[s] = n[s], 0 for a stream that moves nothing (a negative count; takesPart[s] < 0) ->
// the largest, and the row length of a dense image [S][C][len], which is at least 1
struct Counts { int most, len; };
static Counts countsOf(const int *n, int S, int *used = nullptr, const int *takesPart = nullptr) {
	int most = 0;
	for (int s = 0; s < S; ++s) {
		const int k = (takesPart && takesPart[s] < 0) ? 0 : std::max(n[s], 0);
		if (used) used[s] = k;
		most = std::max(most, k);
	}
	return Counts{most, std::max(most, 1)};
}
// flush(): a NEGATIVE count leaves that stream out of the call (flush() of an instance also resets it, :456-463: a count of 0 would do that)
struct FlushCounts {
	std::vector<int> counts;
	std::vector<unsigned char> active;
	bool all = true;
	FlushCounts(const int *n, int S) : counts(n, n + S), active(S, 1) {
		for (int s = 0; s < S; ++s) if (counts[s] < 0) { active[s] = 0; counts[s] = 0; all = false; }
	}
	const unsigned char *mask() const { return all ? nullptr : active.data(); }
};

extern "C" {

const char *smst_last_error(void) { return g_lastError.c_str(); }
void smst_reference_version(int out[3]) { out[0] = 1; out[1] = 3; out[2] = 2; }
int smst_device_count(void) {
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess) return 0;
	return n;
}

// ---------------------------------------------------------------------------------------------------------
// batch API
// ---------------------------------------------------------------------------------------------------------
int smst_batch_create_ex(smst_batch **out, int streams, int channels, int block, int interval, int split, int device, long seed, unsigned flags) {
	if (!out) return fail("null output pointer");
	SMST_TRY
	if (flags & ~unsigned(SMST_FLAG_HALF_STATE)) throw smst::Error("unknown creation flag");
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) throw smst::Error("hipGetDeviceCount: no HIP device available (the gfx950 path has no CPU fallback)", true);
	if (device < 0 || device >= n) throw smst::Error("device ordinal out of range");
	std::unique_ptr<smst_batch> b(new smst_batch());
	b->engine.reset(new Batch(streams, channels, block, interval, split != 0, device, seed, (flags & SMST_FLAG_HALF_STATE) != 0));
	b->pcmOut.create(streams, channels);
	b->pcmIn.create(streams);
	b->pcmOutRes.create(streams);
	*out = b.release();
	return SMST_OK;
	SMST_CATCH
}
int smst_batch_create(smst_batch **out, int streams, int channels, int block, int interval, int split, int device, long seed) {
	return smst_batch_create_ex(out, streams, channels, block, interval, split, device, seed, 0u);
}
int smst_batch_create_preset_ex(smst_batch **out, int streams, int channels, int preset, float sampleRate, int split, int device, long seed, unsigned flags) {
	// signalsmith-stretch.h:63-68 (float products truncated to int by configure's int parameters)
	if (preset == 0) return smst_batch_create_ex(out, streams, channels, int(sampleRate*0.12), int(sampleRate*0.03), split < 0 ? 0 : split, device, seed, flags);
	if (preset == 1) return smst_batch_create_ex(out, streams, channels, int(sampleRate*0.1), int(sampleRate*0.04), split < 0 ? 1 : split, device, seed, flags);
	return fail("unknown preset");
}
int smst_batch_create_preset(smst_batch **out, int streams, int channels, int preset, float sampleRate, int split, int device, long seed) {
	return smst_batch_create_preset_ex(out, streams, channels, preset, sampleRate, split, device, seed, 0u);
}
void smst_batch_destroy(smst_batch *b) { delete b; }

#define BATCH_Q(name, expr) int name(const smst_batch *b) { if (!b || !b->engine) return fail("null batch"); return (expr); }
BATCH_Q(smst_batch_streams, b->engine->streams())
BATCH_Q(smst_batch_channels, b->engine->channels())
BATCH_Q(smst_batch_block_samples, b->engine->blockSamples())
BATCH_Q(smst_batch_interval_samples, b->engine->intervalSamples())
BATCH_Q(smst_batch_fft_samples, b->engine->fftSamples())
BATCH_Q(smst_batch_bands, b->engine->bands())
BATCH_Q(smst_batch_input_latency, b->engine->inputLatency())
BATCH_Q(smst_batch_output_latency, b->engine->outputLatency())
BATCH_Q(smst_batch_seek_length, b->engine->seekLength())
BATCH_Q(smst_batch_half_state, b->engine->halfPrecisionState() ? 1 : 0)
int smst_batch_output_seek_length(const smst_batch *b, float rate) { if (!b || !b->engine) return fail("null batch"); return b->engine->outputSeekLength(rate); }
long long smst_batch_workspace_bytes(const smst_batch *b) { if (!b || !b->engine) return fail("null batch"); return (long long)(b->engine->workspaceBytes() + b->pcmOut.workspaceBytes() + b->pcmIn.workspaceBytes() + b->pcmOutRes.workspaceBytes()); }

#define BATCH_CALL(...) if (!b || !b->engine) return fail("null batch"); SMST_TRY __VA_ARGS__; return SMST_OK; SMST_CATCH

int smst_batch_reset(smst_batch *b) {
	BATCH_CALL({
		b->engine->reset();
		b->pcmOut.clearStreamLimitLines(*b->engine, -1); // (the stream limiter's lines begin again, in stream order behind the calls in flight)
		b->pcmIn.clear(-1);                              // (... and the stream resampler's)
		b->pcmOutRes.clear(-1);                          // (... and the stream output resampler's)
		b->pcmOut.clearStreamMeter(b->engine->device(), b->engine->stream(), -1);     // (... and the stream meter's)
	})
}
int smst_batch_set_transpose_factor(smst_batch *b, int s, float m, float t) { BATCH_CALL(b->engine->setTransposeFactor(s, m, t)) }
int smst_batch_set_transpose_semitones(smst_batch *b, int s, float st, float t) { BATCH_CALL(b->engine->setTransposeSemitones(s, st, t)) }
int smst_batch_set_formant_factor(smst_batch *b, int s, float m, int c) { BATCH_CALL(b->engine->setFormantFactor(s, m, c != 0)) }
int smst_batch_set_formant_semitones(smst_batch *b, int s, float st, int c) { BATCH_CALL(b->engine->setFormantSemitones(s, st, c != 0)) }
int smst_batch_set_formant_base(smst_batch *b, int s, float f) { BATCH_CALL(b->engine->setFormantBase(s, f)) }
int smst_batch_set_freq_map_table(smst_batch *b, int s, const float *table, int n) { BATCH_CALL(b->engine->setFreqMapTable(s, table, n)) }
int smst_batch_synchronize(smst_batch *b) { BATCH_CALL(b->engine->synchronize()) }
void *smst_batch_hip_stream(smst_batch *b) { return (b && b->engine) ? (void *)b->engine->stream() : nullptr; }
int smst_batch_enable_profiling(smst_batch *b, int mode) { BATCH_CALL(b->engine->enableProfiling(mode)) }
int smst_batch_take_timings(smst_batch *b, double ms[8], long long launches[6]) {
	BATCH_CALL({
		smst::BatchTimings t = b->engine->takeTimings();
		ms[0] = t.analyseMs; ms[1] = t.feedMs; ms[2] = t.predictMs; ms[3] = t.chainMs; ms[4] = t.synthMs; ms[5] = t.emitMs; ms[6] = t.otherMs;
		launches[0] = t.analyseLaunches; launches[1] = t.predictLaunches; launches[2] = t.chainLaunches; launches[3] = t.synthLaunches; launches[4] = t.emitLaunches;
		ms[7] = t.chainLiveMs; launches[5] = t.chainLiveLaunches;
	})
}
int smst_batch_take_host_times(smst_batch *b, double ms[3], long long *calls) {
	BATCH_CALL({
		const smst::Batch::HostTimes t = b->engine->takeHostTimes();
		ms[0] = t.callMs; ms[1] = t.waitTablesMs; ms[2] = t.waitGateMs;
		if (calls) *calls = t.calls;
	})
}
int smst_batch_debug_get_state(smst_batch *b, int stream, int which, float *dst) { BATCH_CALL(b->engine->debugGetState(stream, which, dst)) }
int smst_batch_debug_get_carry(smst_batch *b, int stream, float *sums, float *products) { BATCH_CALL(b->engine->debugGetCarry(stream, sums, products)) }
int smst_batch_debug_set_state(smst_batch *b, int stream, int which, const float *src) { BATCH_CALL(b->engine->debugSetState(stream, which, src)) }
int smst_batch_debug_set_carry(smst_batch *b, int stream, const float *sums, const float *products) { BATCH_CALL(b->engine->debugSetCarry(stream, sums, products)) }
long long smst_batch_debug_allocation_events(const smst_batch *b) { if (!b || !b->engine) return fail("null batch"); return (long long)b->engine->allocationEvents() + b->stagingAllocs; }
int smst_batch_wait_for_stream(smst_batch *b, void *hipStream) { BATCH_CALL(b->engine->waitForStream(static_cast<hipStream_t>(hipStream))) }
int smst_batch_signal_stream(smst_batch *b, void *hipStream) { BATCH_CALL(b->engine->signalStream(static_cast<hipStream_t>(hipStream))) }
// a helper self-test: n tuples of `inWidth` floats to the device, the kernel, n rows of `outWidth` floats back
static int complexSelfTest(int device, const float *in, float *out, int n, int inWidth, int outWidth, void (*launch)(const float *, float *, int, hipStream_t)) {
	SMST_TRY
	if (n < 1 || !in || !out) throw smst::Error("complex self-test: bad arguments");
	if (hipSetDevice(device) != hipSuccess) throw smst::Error("hipSetDevice failed", true);
	float *dIn = nullptr, *dOut = nullptr;
	if (hipMalloc(reinterpret_cast<void **>(&dIn), (size_t)n*inWidth*sizeof(float)) != hipSuccess) throw smst::Error("hipMalloc failed", true);
	if (hipMalloc(reinterpret_cast<void **>(&dOut), (size_t)n*outWidth*sizeof(float)) != hipSuccess) { hipFree(dIn); throw smst::Error("hipMalloc failed", true); }
	hipError_t e = hipMemcpy(dIn, in, (size_t)n*inWidth*sizeof(float), hipMemcpyHostToDevice);
	if (e == hipSuccess) { launch(dIn, dOut, n, nullptr); e = hipGetLastError(); }
	if (e == hipSuccess) e = hipMemcpy(out, dOut, (size_t)n*outWidth*sizeof(float), hipMemcpyDeviceToHost);
	hipFree(dIn);
	hipFree(dOut);
	if (e != hipSuccess) throw smst::Error(std::string("complex self-test: ") + hipGetErrorString(e), true);
	return 0;
	SMST_CATCH
}
int smst_debug_complex_selftest(int device, const float *in, float *out, int n) { return complexSelfTest(device, in, out, n, 7, 8, smst::launchComplexSelfTest); }
int smst_debug_fft_complex_selftest(int device, const float *in, float *out, int n) { return complexSelfTest(device, in, out, n, 4, 20, smst::launchFftComplexSelfTest); }
long long smst_debug_launch_count(const char *name) { return smst::launchCount(name); }
int smst_batch_debug_get_formants(smst_batch *b, int stream, float *ratio, float *envelope, float *freqEstimate) {
	if (!b || !b->engine) return fail("null batch");
	if (!ratio || !envelope || !freqEstimate) return fail("null destination");
	SMST_TRY
	return b->engine->debugGetFormants(stream, ratio, envelope, freqEstimate) ? 1 : 0;
	SMST_CATCH
}
int smst_batch_debug_get_map(smst_batch *b, int stream, float *dst) {
	if (!b || !b->engine) return fail("null batch");
	SMST_TRY
	return b->engine->debugGetMap(stream, dst) ? 1 : 0;
	SMST_CATCH
}

// host staging: copy the strided host planes into a dense device image [S][C][maxLen]
static const float *stageIn(smst_batch *b, const float *in, long long ss, long long cs, const int *n, int &maxLen) {
	Batch &e = *b->engine;
	const int S = e.streams(), C = e.channels();
	maxLen = countsOf(n, S).len;
	ensureStage(b, b->dIn, (size_t)S*C*maxLen);
	hipSetDevice(e.device());
	for (int s = 0; s < S; ++s) {
		for (int c = 0; c < C; ++c) {
			if (n[s] <= 0) continue;
			if (hipMemcpyAsync(b->dIn + ((size_t)s*C + c)*maxLen, in + s*ss + c*cs, (size_t)n[s]*sizeof(float), hipMemcpyHostToDevice, e.stream()) != hipSuccess)
				throw smst::Error("hipMemcpyAsync (H2D) failed", true);
		}
	}
	if (hipStreamSynchronize(e.stream()) != hipSuccess) throw smst::Error("hipStreamSynchronize failed", true);
	return b->dIn;
}
static void unstageOut(smst_batch *b, float *out, long long ss, long long cs, const int *n, int maxLen) {
	Batch &e = *b->engine;
	const int S = e.streams(), C = e.channels();
	hipSetDevice(e.device());
	for (int s = 0; s < S; ++s) {
		for (int c = 0; c < C; ++c) {
			if (n[s] <= 0) continue;
			if (hipMemcpyAsync(out + s*ss + c*cs, b->dOut + ((size_t)s*C + c)*maxLen, (size_t)n[s]*sizeof(float), hipMemcpyDeviceToHost, e.stream()) != hipSuccess)
				throw smst::Error("hipMemcpyAsync (D2H) failed", true);
		}
	}
	if (hipStreamSynchronize(e.stream()) != hipSuccess) throw smst::Error("hipStreamSynchronize failed", true);
}

int smst_batch_seek(smst_batch *b, const float *in, long long ss, long long cs, const int *inSamples, const double *rates, int memory) {
	BATCH_CALL({
		if (!inSamples) throw smst::Error("null sample counts");
		if (memory == SMST_MEM_DEVICE) {
			b->engine->seek(in, ss, cs, inSamples, rates);
		} else {
			int maxLen;
			const float *dIn = stageIn(b, in, ss, cs, inSamples, maxLen);
			b->engine->seek(dIn, (long long)b->engine->channels()*maxLen, maxLen, inSamples, rates);
			b->engine->synchronize();
		}
	})
}
int smst_batch_process(smst_batch *b, const float *in, long long iss, long long ics, const int *inSamples,
                       float *out, long long oss, long long ocs, const int *outSamples, int memory) {
	BATCH_CALL({
		if (!inSamples || !outSamples) throw smst::Error("null sample counts");
		if (memory == SMST_MEM_DEVICE) {
			b->engine->process(in, iss, ics, inSamples, out, oss, ocs, outSamples);
		} else {
			Batch &e = *b->engine;
			int maxIn;
			const float *dIn = stageIn(b, in, iss, ics, inSamples, maxIn);
			const int maxOut = countsOf(outSamples, e.streams()).len;
			ensureStage(b, b->dOut, (size_t)e.streams()*e.channels()*maxOut);
			e.process(dIn, (long long)e.channels()*maxIn, maxIn, inSamples, b->dOut, (long long)e.channels()*maxOut, maxOut, outSamples);
			unstageOut(b, out, oss, ocs, outSamples, maxOut);
		}
	})
}
int smst_batch_flush(smst_batch *b, float *out, long long oss, long long ocs, const int *outSamples, const float *rates, int memory) {
	BATCH_CALL({
		if (!outSamples) throw smst::Error("null sample counts");
		Batch &e = *b->engine;
		const FlushCounts f(outSamples, e.streams());
		if (memory == SMST_MEM_DEVICE) {
			e.flush(out, oss, ocs, f.counts.data(), rates, f.mask());
		} else {
			const int maxOut = countsOf(f.counts.data(), e.streams()).len;
			ensureStage(b, b->dOut, (size_t)e.streams()*e.channels()*maxOut);
			e.flush(b->dOut, (long long)e.channels()*maxOut, maxOut, f.counts.data(), rates, f.mask());
			unstageOut(b, out, oss, ocs, f.counts.data(), maxOut);
		}
	})
}
int smst_batch_output_seek(smst_batch *b, const float *in, long long ss, long long cs, const int *inputLengths, int memory) {
	BATCH_CALL({
		if (!inputLengths) throw smst::Error("null lengths");
		if (memory == SMST_MEM_DEVICE) {
			b->engine->outputSeek(in, ss, cs, inputLengths);
		} else {
			int maxLen;
			const float *dIn = stageIn(b, in, ss, cs, inputLengths, maxLen);
			b->engine->outputSeek(dIn, (long long)b->engine->channels()*maxLen, maxLen, inputLengths);
			b->engine->synchronize();
		}
	})
}

// ---------------------------------------------------------------------------------------------------------
// interleaved PCM: the four calls above with frame buffers of the SMST_PCM_* formats (include/smst.h).  kPcmIn fills the planar image the engine
// reads, kPcmOut empties the one it wrote; both run on the engine's stream.
// ---------------------------------------------------------------------------------------------------------
static size_t pcmElemBytes(int format) { return format == SMST_PCM_S16 || format == SMST_PCM_F16 ? 2 : format == SMST_PCM_S24 ? 3 : 4; }
// the raw frames of one direction: the pinned host buffer, then the device buffer
static void ensurePcmBytes(smst_batch *b, PinnedBytes &host, DeviceBytes &dev, size_t bytes) {
	host.ensure(bytes, b->engine->device(), b->stagingAllocs, "PCM staging");
	dev.ensure(bytes, b->engine->device(), b->stagingAllocs, "PCM staging");
}
static void checkPcmSide(const void *buf, long long frameStride, const int *n, int S, int C, bool negativeSkips) {
	if (!n) throw smst::Error("null sample counts");
	if (frameStride < C) throw smst::Error("frame stride smaller than the channel count");
	for (int s = 0; s < S; ++s) {
		if (n[s] < 0 && !negativeSkips) throw smst::Error("negative sample count");
		if (n[s] > 0 && !buf) throw smst::Error("null buffer with a non-zero sample count");
	}
}
static void checkPcmFormat(int format, int memory) {
	if (format != SMST_PCM_S16 && format != SMST_PCM_F32 && format != SMST_PCM_S24 && format != SMST_PCM_S32 && format != SMST_PCM_F16)
		throw smst::Error("unknown PCM format (SMST_PCM_S16, _F32, _S24, _S32 or _F16)");
	if (memory != SMST_MEM_HOST && memory != SMST_MEM_DEVICE) throw smst::Error("unknown memory kind");
}
// the table of this call: the set the call before the previous one used (its conversion kernels must have run)
static smst_batch::PcmTable &beginPcmCall(smst_batch *b) {
	Batch &e = *b->engine;
	hipSetDevice(e.device());
	b->pcmTables.create();
	smst_batch::PcmTable &c = b->pcmTables.begin();
	if (!c.host) { // (both sets with the first call, as Batch::exact's segment tables: the second call allocates nothing)
		++b->stagingAllocs;
		for (smst_batch::PcmTable &t : b->pcmTables.sets) {
			t.host.allocate(smst::PcmTableLayout(e.streams()).bytes(), "PCM counts");
			t.dev.allocate(smst::PcmTableLayout(e.streams()).bytes(), "PCM counts");
		}
	}
	c.out = smst::PcmOutCall();
	c.mostLimited = c.mostLimitedPlain = c.mostLimitedTruePeak = 0;
	c.mostDelivered = 0;
	return c;
}
// The output side's sections of the call's table, from the batch's state, and their upload -- with the S output counts in front of them where
// the call has some -- in one copy; c.out is where the kernels read them
static void pcmUploadOutTable(smst_batch *b, smst_batch::PcmTable &c, int format, bool withOutCounts) {
	Batch &e = *b->engine;
	const smst::PcmTableLayout at(e.streams());
	c.out = b->pcmOut.fill(c.host, c.dev, at, format);
	const smst::PcmTableLayout::Range r = at.upload(withOutCounts, c.out.dither != nullptr, c.out.level.table != nullptr, c.out.loud != nullptr);
	if (hipMemcpyAsync(c.dev + r.offset, c.host + r.offset, r.bytes, hipMemcpyHostToDevice, e.stream()) != hipSuccess) throw smst::Error("hipMemcpyAsync (H2D) failed", true);
}
static void endPcmCall(smst_batch *b) { b->pcmTables.end(b->engine->stream()); }
// a stream's row in the library's own raw buffers: its frames densely, rows a multiple of 16 bytes apart for every element size
static long long pcmRowElems(int maxFrames, int C) { return ((long long)maxFrames*C + 15)/16*16; }

// Host frames -> the library's raw device buffer b->dPcmIn (rows of pcmRowElems(most, C) elements, frames dense), one copy across PCIe on the engine's stream
static void pcmRawIn(smst_batch *b, const void *in, long long ss, long long fs, const int *n, int most, int format) {
	Batch &e = *b->engine;
	const int S = e.streams(), C = e.channels();
	const size_t esz = pcmElemBytes(format);
	const long long row = pcmRowElems(most, C);
	const size_t bytes = (size_t)S*row*esz;
	ensurePcmBytes(b, b->hPcmIn, b->dPcmIn, bytes);
	for (int s = 0; s < S; ++s) {
		if (n[s] <= 0) continue;
		const unsigned char *src = static_cast<const unsigned char *>(in) + (size_t)s*ss*esz;
		unsigned char *dst = b->hPcmIn + (size_t)s*row*esz;
		if (fs == C) std::memcpy(dst, src, (size_t)n[s]*C*esz);
		else for (int i = 0; i < n[s]; ++i) std::memcpy(dst + (size_t)i*C*esz, src + (size_t)i*fs*esz, (size_t)C*esz);
	}
	if (hipMemcpyAsync(b->dPcmIn, b->hPcmIn, bytes, hipMemcpyHostToDevice, e.stream()) != hipSuccess) throw smst::Error("hipMemcpyAsync (H2D) failed", true);
}
// ... and b->dPcmOut back into the caller's host frames: one copy, a synchronisation, one memcpy per stream (frame by frame where frameStride > C)
static void pcmRawOut(smst_batch *b, void *out, long long ss, long long fs, const int *n, int most, int format) {
	Batch &e = *b->engine;
	const int S = e.streams(), C = e.channels();
	const size_t esz = pcmElemBytes(format);
	const long long row = pcmRowElems(most, C);
	if (hipMemcpyAsync(b->hPcmOut, b->dPcmOut, (size_t)S*row*esz, hipMemcpyDeviceToHost, e.stream()) != hipSuccess) throw smst::Error("hipMemcpyAsync (D2H) failed", true);
	if (hipStreamSynchronize(e.stream()) != hipSuccess) throw smst::Error("hipStreamSynchronize failed", true);
	for (int s = 0; s < S; ++s) {
		if (n[s] <= 0) continue;
		const unsigned char *src = b->hPcmOut + (size_t)s*row*esz;
		unsigned char *dst = static_cast<unsigned char *>(out) + (size_t)s*ss*esz;
		if (fs == C) std::memcpy(dst, src, (size_t)n[s]*C*esz);
		else for (int i = 0; i < n[s]; ++i) std::memcpy(dst + (size_t)i*fs*esz, src + (size_t)i*C*esz, (size_t)C*esz);
	}
}

// Raw frames -> the planar image b->dIn [S][C][maxLen] (returns maxLen), on the engine's stream and in front of every reader of the call's input
// A streaming call in which a stream has the stream-resample setting (include/smst.h, "Stream resample"): kPcmIn runs once per destination
// image that has frames -- the plain streams into b->dIn as ever, the streams with the setting into the raw image --, and kPcmStreamResample
// forms those streams' k frames into b->dIn from their lines and the raw image.  b->pcmIn.counts: what the engine gets.  clearLines: a seek --
// the lines of the streams that take part are cleared before their frames go in.  Every refusal comes before anything changes
static int pcmStageInResampled(smst_batch *b, smst_batch::PcmTable &c, const void *in, long long ss, long long fs, const int *n, int format, int memory, bool clearLines) {
	Batch &e = *b->engine;
	PcmStreamResampleState &r = b->pcmIn;
	const int S = e.streams(), C = e.channels();
	const smst::StreamResampleTableLayout at(S);
	int most = 0, mostPlain = 0, mostRaw = 0, mostK = 0, maxLen = 1;
	for (int s = 0; s < S; ++s) {
		const int frames = std::max(n[s], 0);
		most = std::max(most, frames);
		if (e.streamResampled(s)) {
			r.counts[s] = int(r.framesOf(e, s, frames, clearLines || r.stream[s].fresh));
			mostRaw = std::max(mostRaw, frames);
			mostK = std::max(mostK, r.counts[s]);
		} else {
			r.counts[s] = n[s];
			mostPlain = std::max(mostPlain, frames);
		}
		maxLen = std::max(maxLen, r.counts[s]);
	}
	const int rawLen = std::max(mostRaw, 1), tileFrames = smst::streamResampleTileFrames(mostK);
	ensureStage(b, b->dIn, (size_t)S*C*maxLen);
	ensureStage(b, r.dRaw, (size_t)S*C*rawLen);
	hipSetDevice(e.device());
	int maxSpanPitch = 4;
	for (int s = 0; s < S; ++s) {
		const int frames = std::max(n[s], 0);
		smst::StreamResampleEntry entry{nullptr, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
		const bool on = e.streamResampled(s);
		if (on) {
			PcmStreamResampleState::Stream &st = r.stream[s];
			if (clearLines && n[s] >= 0) { st.fed = st.made = 0; st.fresh = 1; }
			const smst::ResampleShape &g = e.streamResampleShape(s);
			entry = smst::StreamResampleEntry{e.streamResampleTaps(s), st.fed, st.made, 0, 0, frames, r.counts[s], g.L, g.M, g.H, g.T, g.pitch, st.set, st.fresh, 0};
			maxSpanPitch = std::max(maxSpanPitch, smst::resampleSpanPitchOf(g.L, g.M, g.T, tileFrames));
			if (frames > 0) { st.fed += frames; st.made += r.counts[s]; st.set ^= 1; st.fresh = 0; } // (a stream with no frame keeps its line)
		}
		at.plainCounts(c.resHost)[s] = on ? 0 : frames;
		at.rawCounts(c.resHost)[s] = on ? frames : 0;
		at.entries(c.resHost)[s] = entry;
	}
	if (hipMemcpyAsync(c.resDev, c.resHost, at.bytes(), hipMemcpyHostToDevice, e.stream()) != hipSuccess) throw smst::Error("hipMemcpyAsync (H2D) failed", true);
	const void *raw = in;
	long long rawSS = ss, rawFS = fs;
	if (memory == SMST_MEM_HOST && most > 0) {
		pcmRawIn(b, in, ss, fs, n, most, format);
		raw = b->dPcmIn; rawSS = pcmRowElems(most, C); rawFS = C;
	}
	smst::launchPcmIn(format, raw, rawSS, rawFS, b->dIn, (long long)C*maxLen, maxLen, at.plainCounts(c.resDev), S, C, mostPlain, e.stream());
	smst::launchPcmIn(format, raw, rawSS, rawFS, r.dRaw, (long long)C*rawLen, rawLen, at.rawCounts(c.resDev), S, C, mostRaw, e.stream());
	if (mostRaw > 0)
		smst::launchPcmStreamResample(r.dRaw, (long long)C*rawLen, rawLen, b->dIn, (long long)C*maxLen, maxLen, r.dLines, (long long)(r.dLines.cap/2), at.entries(c.resDev), S, C, mostK, maxSpanPitch, e.stream());
	e.waitForStream(e.stream());
	return maxLen;
}
// engineCounts (null: the call serves no stream-resample setting): the frames the engine gets from each stream -- n itself, or the k of "Stream resample"
static int pcmStageIn(smst_batch *b, smst_batch::PcmTable &c, const void *in, long long ss, long long fs, const int *n, int format, int memory, const int **engineCounts = nullptr, bool clearLines = false) {
	Batch &e = *b->engine;
	if (engineCounts) *engineCounts = n;
	if (engineCounts && PcmStreamResampleState::any(e)) {
		const int maxLen = pcmStageInResampled(b, c, in, ss, fs, n, format, memory, clearLines);
		*engineCounts = b->pcmIn.counts.data();
		return maxLen;
	}
	const int S = e.streams(), C = e.channels();
	const smst::PcmTableLayout at(S);
	const Counts k = countsOf(n, S, at.inCounts(c.host));
	const int most = k.most, maxLen = k.len;
	ensureStage(b, b->dIn, (size_t)S*C*maxLen);
	hipSetDevice(e.device());
	if (hipMemcpyAsync(at.inCounts(c.dev), at.inCounts(c.host), S*sizeof(int), hipMemcpyHostToDevice, e.stream()) != hipSuccess) throw smst::Error("hipMemcpyAsync (H2D) failed", true);
	const void *raw = in;
	long long rawSS = ss, rawFS = fs;
	if (memory == SMST_MEM_HOST && most > 0) {
		pcmRawIn(b, in, ss, fs, n, most, format);
		raw = b->dPcmIn; rawSS = pcmRowElems(most, C); rawFS = C;
	}
	smst::launchPcmIn(format, raw, rawSS, rawFS, b->dIn, (long long)C*maxLen, maxLen, at.inCounts(c.dev), S, C, most, e.stream());
	// the engine reads its input on more than one stream (the silence gate on its own): the edge a caller's producer stream gets
	e.waitForStream(e.stream());
	return maxLen;
}
// the output side's buffers, before the engine is called (a growth frees, which synchronises the device): returns maxLen of b->dOut [S][C][maxLen]
// A streaming call in which a stream of the batch has the stream-output-resample setting (include/smst.h, "Stream output resample"): n[s]
// counts delivered frames, render[s] (PcmStreamResampleOutState::prepare) is what the engine renders.  The call's entries -- uploaded in one
// copy --, the image of the delivered frames, and the streams' counters, which move on here.  Returns the row length b->dOut needs: it holds
// a stream's E rendered frames first and its Nd delivered frames then
static int pcmPrepareOutResampled(smst_batch *b, smst_batch::PcmTable &c, const int *n, const int *render, int len) {
	Batch &e = *b->engine;
	PcmStreamResampleOutState &r = b->pcmOutRes;
	const int S = e.streams(), C = e.channels();
	const smst::StreamResampleOutTableLayout at(S);
	int most = 0;
	for (int s = 0; s < S; ++s) {
		len = std::max(len, render[s]);
		if (e.streamOutResampled(s)) most = std::max(most, n[s]);
	}
	const int tileFrames = smst::streamResampleTileFrames(most);
	c.mostDelivered = most; c.deliveredLen = std::max(most, 1); c.outSpanPitch = 4;
	if (most > 0) ensureStage(b, r.dDelivered, (size_t)S*C*c.deliveredLen);
	hipSetDevice(e.device());
	for (int s = 0; s < S; ++s) {
		smst::StreamResampleOutEntry entry{nullptr, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
		if (e.streamOutResampled(s)) {
			PcmStreamResampleOutState::Stream &st = r.stream[s];
			const smst::ResampleShape &g = e.streamOutResampleShape(s);
			entry = smst::StreamResampleOutEntry{e.streamOutResampleTaps(s), st.delivered, smst::streamResampleOutDue(st.delivered, g.L, g.M), 0, 0, std::max(n[s], 0), std::max(render[s], 0),
			                                     smst::streamResampleOutLatency(g.L, g.M, g.H), g.L, g.M, g.H, g.T, g.pitch, st.set, st.fresh};
			c.outSpanPitch = std::max(c.outSpanPitch, smst::resampleSpanPitchOf(g.L, g.M, g.T, tileFrames));
			if (n[s] > 0) { st.delivered += n[s]; st.set ^= 1; st.fresh = 0; } // (a stream with no frame keeps its line)
		}
		at.entries(c.outResHost)[s] = entry;
	}
	if (hipMemcpyAsync(c.outResDev, c.outResHost, at.bytes(), hipMemcpyHostToDevice, e.stream()) != hipSuccess) throw smst::Error("hipMemcpyAsync (H2D) failed", true);
	return len;
}
// render (null: no stream of the batch has the stream-output-resample setting): the frames the engine renders for each stream
static int pcmPrepareOut(smst_batch *b, smst_batch::PcmTable &c, const int *n, int format, int memory, const int *render = nullptr) {
	Batch &e = *b->engine;
	const int S = e.streams(), C = e.channels();
	Counts k = countsOf(n, S, smst::PcmTableLayout(S).outCounts(c.host));
	if (render) k.len = pcmPrepareOutResampled(b, c, smst::PcmTableLayout(S).outCounts(c.host), render, k.len);
	ensureStage(b, b->dOut, (size_t)S*C*k.len);
	if (memory == SMST_MEM_HOST && k.most > 0) ensurePcmBytes(b, b->hPcmOut, b->dPcmOut, (size_t)S*pcmRowElems(k.most, C)*pcmElemBytes(format));
	hipSetDevice(e.device());
	b->pcmOut.ensureStreamMeterScan(e.device(), b->pcmOut.mostStreamMetered(smst::PcmTableLayout(S).outCounts(c.host)), 0, b->stagingAllocs);
	c.mostLimited = b->pcmOut.mostStreamLimited(smst::PcmTableLayout(S).outCounts(c.host), &c.mostLimitedTruePeak);
	c.mostLimitedPlain = c.mostLimitedTruePeak > 0 ? b->pcmOut.mostStreamLimitedPlain(smst::PcmTableLayout(S).outCounts(c.host)) : c.mostLimited;
	if (c.mostLimited > 0) b->pcmOut.ensureStreamLimitRows(e, c.mostLimited, b->stagingAllocs);
	pcmUploadOutTable(b, c, format, true);
	return k.len;
}
// The planar image b->dOut -> raw frames, behind the engine's last emitting kernel (everything of a call is joined into the engine's stream,
// which is what smst_batch_synchronize and smst_batch_signal_stream wait on).  Host memory: the call returns with the frames in place.
static void pcmStageOut(smst_batch *b, smst_batch::PcmTable &c, void *out, long long ss, long long fs, int maxLen, int format, int memory) {
	Batch &e = *b->engine;
	const int S = e.streams(), C = e.channels();
	const smst::PcmTableLayout at(S);
	const int *n = at.outCounts(c.host);
	const int most = countsOf(n, S).most;
	hipSetDevice(e.device());
	// a call that delivers frames to a stream with the stream-output-resample setting: those streams' delivered frames, formed from their lines
	// and the frames the engine has just rendered, take the place of the rendered ones in b->dOut, in front of every stage below
	if (c.mostDelivered > 0) {
		PcmStreamResampleOutState &r = b->pcmOutRes;
		const smst::StreamResampleOutEntry *entries = smst::StreamResampleOutTableLayout(S).entries(c.outResDev);
		smst::launchPcmStreamResampleOut(b->dOut, (long long)C*maxLen, maxLen, r.dDelivered, (long long)C*c.deliveredLen, c.deliveredLen, r.dLines, (long long)(r.dLines.cap/2), entries, S, C,
		                                 c.mostDelivered, c.outSpanPitch, e.stream());
		smst::launchPcmStreamResampleOutCopy(r.dDelivered, (long long)C*c.deliveredLen, c.deliveredLen, b->dOut, (long long)C*maxLen, maxLen, entries, S, C, c.mostDelivered, e.stream());
	}
	// a call that limits a stream: the two passes and the limited conversion (a kernel of its own) in the place of the levelled one
	auto convert = [&](void *raw, long long rawSS, long long rawFS) {
		if (c.mostLimited > 0) {
			smst::launchPcmOutLimited(format, b->dOut, (long long)C*maxLen, maxLen, raw, rawSS, rawFS, at.outCounts(c.dev), S, C, most, c.mostLimitedPlain, c.mostLimitedTruePeak, c.out.overs, e.stream(), c.out.dither,
			                          c.out.level, b->pcmOut.streamLimitView);
			b->pcmOut.advanceStreamLimit(n);
		} else {
			smst::launchPcmOut(format, b->dOut, (long long)C*maxLen, maxLen, raw, rawSS, rawFS, at.outCounts(c.dev), S, C, most, c.out.overs, e.stream(), c.out.dither, c.out.level);
		}
	};
	if (memory == SMST_MEM_DEVICE) {
		convert(out, ss, fs);
	} else if (most >= 1) {
		convert(b->dPcmOut, pcmRowElems(most, C), C);
		pcmRawOut(b, out, ss, fs, n, most, format);
	}
	// the stream meter: behind the call's last emitting kernel (and behind a host call's copy back: the call does not wait for it)
	b->pcmOut.meterStream(e.stream(), b->dOut, (long long)C*maxLen, maxLen, n, at.outCounts(c.dev));
	b->pcmOut.advance(n);
}

int smst_batch_set_pcm_dither(smst_batch *b, int stream, int mode, long long seed) { BATCH_CALL(b->pcmOut.setDither(stream, mode, seed)) }
int smst_batch_pcm_dither(const smst_batch *b, int stream, int *mode, long long *seed, long long *frames) {
	if (!b || !b->engine) return fail("null batch");
	if (stream < 0 || stream >= b->engine->streams()) return fail("stream index out of range");
	const PcmOutState::Dither &d = b->pcmOut.dither[stream];
	if (mode) *mode = d.mode;
	if (seed) *seed = d.seed;
	if (frames) *frames = (long long)d.frames;
	return SMST_OK;
}
int smst_batch_set_pcm_level(smst_batch *b, int stream, int mode, float gain, float ceiling) { BATCH_CALL(b->pcmOut.setLevel(stream, mode, gain, ceiling)) }
int smst_batch_pcm_level(const smst_batch *b, int stream, int *mode, float *gain, float *ceiling) {
	if (!b || !b->engine) return fail("null batch");
	if (stream < 0 || stream >= b->engine->streams()) return fail("stream index out of range");
	const PcmOutState::Level &l = b->pcmOut.level[stream];
	if (mode) *mode = l.mode;
	if (gain) *gain = l.gain;
	if (ceiling) *ceiling = l.ceiling;
	return SMST_OK;
}
int smst_batch_set_pcm_loudness(smst_batch *b, int stream, double targetLufs, float ceiling, double sampleRate) { BATCH_CALL(b->pcmOut.setLoudness(stream, targetLufs, ceiling, sampleRate)) }
int smst_batch_pcm_loudness(const smst_batch *b, int stream, double *target, double *sampleRate) {
	if (!b || !b->engine) return fail("null batch");
	if (stream < 0 || stream >= b->engine->streams()) return fail("stream index out of range");
	if (b->pcmOut.level[stream].mode != SMST_LEVEL_LOUDNESS) return fail("the stream is not in SMST_LEVEL_LOUDNESS");
	if (target) *target = b->pcmOut.loud[stream].target;
	if (sampleRate) *sampleRate = b->pcmOut.loud[stream].sampleRate;
	return SMST_OK;
}
int smst_batch_set_pcm_loudness_weights(smst_batch *b, const float *weights) { BATCH_CALL(b->pcmOut.setLoudnessWeights(weights)) }
int smst_batch_set_pcm_true_peak(smst_batch *b, int stream, int on) { BATCH_CALL(b->pcmOut.setTruePeak(stream, on)) }
int smst_batch_pcm_true_peak(const smst_batch *b, int stream, int *on) {
	if (!b || !b->engine) return fail("null batch");
	if (stream < 0 || stream >= b->engine->streams()) return fail("stream index out of range");
	if (on) *on = b->pcmOut.truePeak[stream];
	return SMST_OK;
}
int smst_batch_take_pcm_true_peaks(smst_batch *b, float *truePeaks) {
	BATCH_CALL({
		Batch &e = *b->engine;
		e.synchronize();
		std::vector<float> peaks((size_t)e.streams(), 0.0f);
		e.readTruePeaks(peaks.data()); // (false: no call has measured yet -- 0 for every stream)
		if (truePeaks) std::copy(peaks.begin(), peaks.end(), truePeaks);
	})
}
int smst_batch_set_pcm_limiter(smst_batch *b, int stream, int on) {
	BATCH_CALL({
		b->pcmOut.setLimiter(stream, on);
		if (on) b->engine->prepareLimiter(); // (the window goes to the device here, not in a call)
	})
}
int smst_batch_pcm_limiter(const smst_batch *b, int stream, int *on) {
	if (!b || !b->engine) return fail("null batch");
	if (stream < 0 || stream >= b->engine->streams()) return fail("stream index out of range");
	if (on) *on = b->pcmOut.limiter[stream];
	return SMST_OK;
}
int smst_batch_set_pcm_limiter_lookahead(smst_batch *b, int frames) {
	BATCH_CALL({
		b->engine->setLimiterLookahead(frames); // (synchronises where the window is on the device: the stream limiter's lines are then idle)
		if (b->pcmOut.dLimitLines) b->pcmOut.prepareStreamLimitLines(*b->engine);
	})
}
// Stream limiter (include/smst.h): the setting lives beside the level entries, the lines and rows in the batch's PCM output state
int smst_batch_set_pcm_stream_limiter(smst_batch *b, int stream, int on, float ceiling) { BATCH_CALL(b->pcmOut.setStreamLimiter(*b->engine, stream, on, ceiling)) }
int smst_batch_pcm_stream_limiter(const smst_batch *b, int stream, int *on, float *ceiling) {
	if (!b || !b->engine) return fail("null batch");
	if (stream < 0 || stream >= b->engine->streams()) return fail("stream index out of range");
	if (on) *on = b->pcmOut.streamLimit[stream].on;
	if (ceiling) *ceiling = b->pcmOut.streamLimit[stream].ceiling;
	return SMST_OK;
}
int smst_batch_pcm_stream_limiter_latency(const smst_batch *b, int *frames) {
	if (!b || !b->engine) return fail("null batch");
	if (frames) *frames = 2*b->engine->limiterLookahead();
	return SMST_OK;
}
int smst_batch_set_pcm_stream_limiter_true_peak(smst_batch *b, int stream, int on) { BATCH_CALL(b->pcmOut.setStreamLimiterTruePeak(*b->engine, stream, on)) }
int smst_batch_pcm_stream_limiter_true_peak(const smst_batch *b, int stream, int *on) {
	if (!b || !b->engine) return fail("null batch");
	if (stream < 0 || stream >= b->engine->streams()) return fail("stream index out of range");
	if (on) *on = b->pcmOut.streamLimit[stream].truePeak;
	return SMST_OK;
}
int smst_batch_pcm_stream_limiter_latency_of(const smst_batch *b, int stream, int *frames) {
	if (!b || !b->engine) return fail("null batch");
	if (stream < 0 || stream >= b->engine->streams()) return fail("stream index out of range");
	if (frames) *frames = b->pcmOut.streamLimitLatency(*b->engine, stream);
	return SMST_OK;
}
int smst_batch_take_pcm_stream_limiter(smst_batch *b, float *minGain, long long *limitedFrames) {
	BATCH_CALL({
		b->engine->synchronize();
		hipSetDevice(b->engine->device());
		b->pcmOut.takeStreamLimiter(minGain, limitedFrames);
	})
}
// Stream meter (include/smst.h): the setting, the counters and the device side live in the batch's PCM output state
int smst_batch_set_pcm_stream_meter(smst_batch *b, int stream, int on, double sampleRate, int maxSubBlocks) {
	BATCH_CALL(b->pcmOut.setStreamMeter(b->engine->device(), b->engine->stream(), stream, on, sampleRate, maxSubBlocks, b->stagingAllocs))
}
int smst_batch_pcm_stream_meter(const smst_batch *b, int stream, int *on, double *sampleRate, int *maxSubBlocks) {
	if (!b || !b->engine) return fail("null batch");
	if (stream < 0 || stream >= b->engine->streams()) return fail("stream index out of range");
	const PcmOutState::StreamMeter &m = b->pcmOut.streamMeter[stream];
	if (on) *on = m.on;
	if (sampleRate) *sampleRate = m.sampleRate;
	if (maxSubBlocks) *maxSubBlocks = m.maxSub;
	return SMST_OK;
}
int smst_batch_pcm_stream_meter_frames(const smst_batch *b, int stream, long long *frames, long long *metered) {
	if (!b || !b->engine) return fail("null batch");
	if (stream < 0 || stream >= b->engine->streams()) return fail("stream index out of range");
	const PcmOutState::StreamMeter &m = b->pcmOut.streamMeter[stream];
	if (frames) *frames = m.frames;
	if (metered) *metered = std::min(m.frames, m.cap);
	return SMST_OK;
}
static double loudnessLufs(double Z, int gated);
static double powerLufs(double P);
static double rangeLu(double lo, double hi, int n);
int smst_batch_take_pcm_stream_meter(smst_batch *b, double *lufs, int *blocks, int *gated, double *momentary, double *shortTerm,
                                     double *momentaryMax, double *shortTermMax, double *range, double *low, double *high,
                                     int *shortBlocks, int *rangeBlocks, float *truePeaks, float *samplePeaks) {
	BATCH_CALL({
		Batch &e = *b->engine;
		const int S = e.streams();
		e.synchronize();
		PcmOutState::MeterReading r;
		hipSetDevice(e.device());
		b->pcmOut.readStreamMeter(e.stream(), r); // (false: the setting was never on -- nothing is defined)
		for (int s = 0; s < S; ++s) {
			const int n = r.rangeCounts[2*s + 1];
			if (lufs) lufs[s] = loudnessLufs(r.Z[s], r.counts[2*s + 1]);
			if (blocks) blocks[s] = r.counts[2*s];
			if (gated) gated[s] = r.counts[2*s + 1];
			if (momentary) momentary[s] = powerLufs(r.newest[2*s]);
			if (shortTerm) shortTerm[s] = powerLufs(r.newest[2*s + 1]);
			if (momentaryMax) momentaryMax[s] = powerLufs(r.range[4*s]);
			if (shortTermMax) shortTermMax[s] = powerLufs(r.range[4*s + 1]);
			if (range) range[s] = rangeLu(r.range[4*s + 2], r.range[4*s + 3], n);
			if (low) low[s] = n > 0 ? powerLufs(r.range[4*s + 2]) : -INFINITY;
			if (high) high[s] = n > 0 ? powerLufs(r.range[4*s + 3]) : -INFINITY;
			if (shortBlocks) shortBlocks[s] = r.rangeCounts[2*s];
			if (rangeBlocks) rangeBlocks[s] = n;
			if (truePeaks) std::memcpy(truePeaks + s, &r.peaks[s], sizeof(float));
			if (samplePeaks) std::memcpy(samplePeaks + s, &r.peaks[(size_t)S + s], sizeof(float));
		}
	})
}
int smst_batch_pcm_limiter_lookahead(const smst_batch *b, int *frames) {
	if (!b || !b->engine) return fail("null batch");
	if (frames) *frames = b->engine->limiterLookahead();
	return SMST_OK;
}
int smst_batch_take_pcm_limiter(smst_batch *b, float *minGain, long long *limitedFrames) {
	BATCH_CALL({
		Batch &e = *b->engine;
		e.synchronize();
		std::vector<float> gains((size_t)e.streams(), 1.0f);
		std::vector<long long> frames((size_t)e.streams(), 0);
		e.readLimiter(gains.data(), frames.data()); // (false: no call has limited yet -- 1 and 0 for every stream)
		if (minGain) std::copy(gains.begin(), gains.end(), minGain);
		if (limitedFrames) std::copy(frames.begin(), frames.end(), limitedFrames);
	})
}
// Z and the count of gated blocks -> LUFS; -inf where loudness is undefined
static double loudnessLufs(double Z, int gated) { return (gated > 0 && Z > 0 && std::isfinite(Z)) ? -0.691 + 10*std::log10(Z) : -INFINITY; }
int smst_batch_take_pcm_loudness(smst_batch *b, double *lufs, int *blocks, int *gated) {
	BATCH_CALL({
		Batch &e = *b->engine;
		const int S = e.streams();
		e.synchronize();
		std::vector<double> Z((size_t)S, 0.0);
		std::vector<int> counts((size_t)2*S, 0);
		e.readLoudness(Z.data(), counts.data()); // (false: no call has measured yet -- nothing is defined)
		for (int s = 0; s < S; ++s) {
			if (lufs) lufs[s] = loudnessLufs(Z[s], counts[2*s + 1]);
			if (blocks) blocks[s] = counts[2*s];
			if (gated) gated[s] = counts[2*s + 1];
		}
	})
}
int smst_batch_set_pcm_loudness_range(smst_batch *b, int stream, int on, double sampleRate) { BATCH_CALL(b->pcmOut.setLoudnessRange(stream, on, sampleRate)) }
int smst_batch_pcm_loudness_range(const smst_batch *b, int stream, int *on, double *sampleRate) {
	if (!b || !b->engine) return fail("null batch");
	if (stream < 0 || stream >= b->engine->streams()) return fail("stream index out of range");
	if (on) *on = b->pcmOut.meter[stream].on;
	if (sampleRate) *sampleRate = b->pcmOut.meter[stream].sampleRate;
	return SMST_OK;
}
int smst_batch_set_pcm_loudness_caps(smst_batch *b, int stream, double maxMomentaryLufs, double maxShortTermLufs) { BATCH_CALL(b->pcmOut.setLoudnessCaps(stream, maxMomentaryLufs, maxShortTermLufs)) }
int smst_batch_pcm_loudness_caps(const smst_batch *b, int stream, double *maxMomentaryLufs, double *maxShortTermLufs) {
	if (!b || !b->engine) return fail("null batch");
	if (stream < 0 || stream >= b->engine->streams()) return fail("stream index out of range");
	if (maxMomentaryLufs) *maxMomentaryLufs = b->pcmOut.meter[stream].capMomentary;
	if (maxShortTermLufs) *maxShortTermLufs = b->pcmOut.meter[stream].capShortTerm;
	return SMST_OK;
}
// a power -> LUFS, -inf where it is 0; lo and hi of n gated values -> the range in LU
static double powerLufs(double P) { return P > 0 ? -0.691 + 10*std::log10(P) : -INFINITY; }
static double rangeLu(double lo, double hi, int n) { return n > 0 && lo > 0 ? 10*std::log10(hi/lo) : 0.0; }
int smst_batch_take_pcm_loudness_range(smst_batch *b, double *momentaryMax, double *shortTermMax, double *range, double *low, double *high, int *shortBlocks, int *rangeBlocks) {
	BATCH_CALL({
		Batch &e = *b->engine;
		const int S = e.streams();
		e.synchronize();
		std::vector<double> m((size_t)4*S, 0.0);
		std::vector<int> counts((size_t)2*S, 0);
		e.readLoudnessRange(m.data(), counts.data()); // (false: no call has metered yet -- nothing is defined)
		for (int s = 0; s < S; ++s) {
			const int n = counts[2*s + 1];
			if (momentaryMax) momentaryMax[s] = powerLufs(m[4*s]);
			if (shortTermMax) shortTermMax[s] = powerLufs(m[4*s + 1]);
			if (range) range[s] = rangeLu(m[4*s + 2], m[4*s + 3], n);
			if (low) low[s] = n > 0 ? powerLufs(m[4*s + 2]) : -INFINITY;
			if (high) high[s] = n > 0 ? powerLufs(m[4*s + 3]) : -INFINITY;
			if (shortBlocks) shortBlocks[s] = counts[2*s];
			if (rangeBlocks) rangeBlocks[s] = n;
		}
	})
}
// a streaming call knows no clip: refused, before anything runs, where a stream that takes part (active null: every one) has a whole-clip mode
// or the true-peak flag (a meter across calls would need 11 frames of carried history per channel)
static void refuseWholeClipLevel(const smst_batch *b, const unsigned char *active) {
	if (!b->pcmOut.levelled) return;
	for (size_t s = 0; s < b->pcmOut.level.size(); ++s)
		if ((!active || active[s]) && b->pcmOut.level[s].mode != SMST_LEVEL_FIXED)
			throw smst::Error("stream " + std::to_string(s) + " has a whole-clip level mode (SMST_LEVEL_PROTECT / _NORMALISE / _LOUDNESS): smst_batch_exact_pcm only");
	for (size_t s = 0; s < b->pcmOut.truePeak.size(); ++s)
		if ((!active || active[s]) && b->pcmOut.truePeak[s])
			throw smst::Error("stream " + std::to_string(s) + " has the true-peak flag (smst_batch_set_pcm_true_peak): smst_batch_exact_pcm only");
	for (size_t s = 0; s < b->pcmOut.limiter.size(); ++s)
		if ((!active || active[s]) && b->pcmOut.limiter[s])
			throw smst::Error("stream " + std::to_string(s) + " has the limiter flag (smst_batch_set_pcm_limiter): smst_batch_exact_pcm only");
	for (size_t s = 0; s < b->pcmOut.meter.size(); ++s)
		if ((!active || active[s]) && (b->pcmOut.meter[s].on || b->pcmOut.capped(int(s))))
			throw smst::Error("stream " + std::to_string(s) + " has the loudness-range meter flag or a loudness cap (smst_batch_set_pcm_loudness_range / _caps), which measure a whole clip: smst_batch_exact_pcm only");
}
static void refuseResampled(const Batch &e, const int *takesPart, const char *call); // (below, with the whole-clip calls)
static void refuseStreamResampled(const Batch &e, const int *takesPart, const char *call);
static void refuseOutResampled(const Batch &e, const int *takesPart, const char *call);
int smst_batch_process_pcm(smst_batch *b, const void *in, long long iss, long long ifs, const int *inSamples,
                           void *out, long long oss, long long ofs, const int *outSamples, int format, int memory) {
	BATCH_CALL({
		Batch &e = *b->engine;
		checkPcmFormat(format, memory);
		checkPcmSide(in, ifs, inSamples, e.streams(), e.channels(), false);
		checkPcmSide(out, ofs, outSamples, e.streams(), e.channels(), false);
		refuseWholeClipLevel(b, nullptr);
		refuseResampled(e, nullptr, "smst_batch_process_pcm");
		refuseOutResampled(e, nullptr, "smst_batch_process_pcm");
		const int *render = b->pcmOutRes.prepare(e, outSamples) ? b->pcmOutRes.render.data() : nullptr; // (a stream with the stream-output-resample setting: its E)
		smst_batch::PcmTable &c = beginPcmCall(b);
		const int *fed = inSamples; // (a stream with the stream-resample setting: its k)
		const int maxIn = pcmStageIn(b, c, in, iss, ifs, inSamples, format, memory, &fed);
		const int maxOut = pcmPrepareOut(b, c, outSamples, format, memory, render);
		e.process(b->dIn, (long long)e.channels()*maxIn, maxIn, fed, b->dOut, (long long)e.channels()*maxOut, maxOut, render ? render : outSamples);
		pcmStageOut(b, c, out, oss, ofs, maxOut, format, memory);
		endPcmCall(b);
	})
}
int smst_batch_seek_pcm(smst_batch *b, const void *in, long long ss, long long fs, const int *inSamples, const double *rates, int format, int memory) {
	BATCH_CALL({
		Batch &e = *b->engine;
		checkPcmFormat(format, memory);
		checkPcmSide(in, fs, inSamples, e.streams(), e.channels(), false);
		refuseResampled(e, nullptr, "smst_batch_seek_pcm");
		smst_batch::PcmTable &c = beginPcmCall(b);
		const int *fed = inSamples;
		const int maxLen = pcmStageIn(b, c, in, ss, fs, inSamples, format, memory, &fed, true);
		e.seek(b->dIn, (long long)e.channels()*maxLen, maxLen, fed, rates);
		endPcmCall(b);
		if (memory == SMST_MEM_HOST) e.synchronize();
	})
}
int smst_batch_flush_pcm(smst_batch *b, void *out, long long oss, long long ofs, const int *outSamples, const float *rates, int format, int memory) {
	BATCH_CALL({
		Batch &e = *b->engine;
		checkPcmFormat(format, memory);
		checkPcmSide(out, ofs, outSamples, e.streams(), e.channels(), true);
		const FlushCounts f(outSamples, e.streams());
		refuseWholeClipLevel(b, f.active.data());
		refuseOutResampled(e, outSamples, "smst_batch_flush_pcm");
		const int *render = b->pcmOutRes.prepare(e, f.counts.data()) ? b->pcmOutRes.render.data() : nullptr; // (a stream left out has no frame: E = 0, its line is kept)
		smst_batch::PcmTable &c = beginPcmCall(b);
		const int maxOut = pcmPrepareOut(b, c, f.counts.data(), format, memory, render);
		e.flush(b->dOut, (long long)e.channels()*maxOut, maxOut, render ? render : f.counts.data(), rates, f.mask());
		pcmStageOut(b, c, out, oss, ofs, maxOut, format, memory);
		endPcmCall(b);
	})
}
int smst_batch_output_seek_pcm(smst_batch *b, const void *in, long long ss, long long fs, const int *inputLengths, int format, int memory) {
	BATCH_CALL({
		Batch &e = *b->engine;
		checkPcmFormat(format, memory);
		checkPcmSide(in, fs, inputLengths, e.streams(), e.channels(), false);
		refuseResampled(e, nullptr, "smst_batch_output_seek_pcm");
		refuseStreamResampled(e, nullptr, "smst_batch_output_seek_pcm");
		smst_batch::PcmTable &c = beginPcmCall(b);
		const int maxLen = pcmStageIn(b, c, in, ss, fs, inputLengths, format, memory);
		e.outputSeek(b->dIn, (long long)e.channels()*maxLen, maxLen, inputLengths);
		endPcmCall(b);
		if (memory == SMST_MEM_HOST) e.synchronize();
	})
}

// ---------------------------------------------------------------------------------------------------------
// whole clips: exact() of every stream (Batch::exact; the clip kernels of smst_clip.h move each stream's segments)
// ---------------------------------------------------------------------------------------------------------
// Refusals, before anything runs.  inner: the frame stride of a frame buffer, 0 for planar ones
static void checkExactArgs(const Batch &e, const void *in, const int *inSamples, const void *out, const int *outSamples, long long inInner, long long outInner, bool frames, int memory) {
	if (memory != SMST_MEM_HOST && memory != SMST_MEM_DEVICE) throw smst::Error("unknown memory kind");
	if (!inSamples || !outSamples) throw smst::Error("null sample counts");
	if (frames && (inInner < e.channels() || outInner < e.channels())) throw smst::Error("frame stride smaller than the channel count");
	for (int s = 0; s < e.streams(); ++s) {
		if (outSamples[s] < 0) continue; // left out of the call
		if (outSamples[s] == 0) throw smst::Error("exact(): outSamples[" + std::to_string(s) + "] is 0 (the playback rate is inSamples/outSamples; a negative count leaves the stream out)");
		if (inSamples[s] < 0) throw smst::Error("exact(): negative inSamples[" + std::to_string(s) + "]");
		if (!out || (inSamples[s] > 0 && !in)) throw smst::Error("null buffer with a non-zero sample count");
	}
}
// the counts of the streams that take part (a stream left out moves no sample in either direction); returns the row length of their image
static int exactCounts(const int *n, const int *outSamples, int S, std::vector<int> &counts) {
	counts.assign(S, 0);
	return countsOf(n, S, counts.data(), outSamples).len;
}
// Batch::exact's flags -> the status array of the call (a stream that was left out keeps its entry)
static void runExact(Batch &e, const Batch::ClipIo &io, const int *inSamples, const int *outSamples, int *status) {
	std::vector<unsigned char> tooShort(e.streams(), 0);
	e.exact(io, inSamples, outSamples, tooShort.data());
	if (status) for (int s = 0; s < e.streams(); ++s) if (outSamples[s] >= 0) status[s] = tooShort[s] ? SMST_ERR_SHORT : SMST_OK;
}
static const char *const kShortMessage = "exact(): input shorter than outputSeekLength";
// Resample (include/smst.h): only smst_batch_exact_pcm serves a stream's ratio.  Every other call with input refuses, before anything runs, where
// a stream that takes part (takesPart null: every one; else the streams with a count >= 0) has one -- skipping the stage would be a silent lie
static void refuseResampled(const Batch &e, const int *takesPart, const char *call) {
	for (int s = 0; s < e.streams(); ++s)
		if ((!takesPart || takesPart[s] >= 0) && e.resampled(s))
			throw smst::Error(std::string(call) + ": stream " + std::to_string(s) + " has a resample ratio other than 1/1 (smst_batch_set_pcm_resample): smst_batch_exact_pcm only");
}
// Stream resample (include/smst.h): that setting is served by smst_batch_process_pcm and _seek_pcm only
static void refuseStreamResampled(const Batch &e, const int *takesPart, const char *call) {
	for (int s = 0; s < e.streams(); ++s)
		if ((!takesPart || takesPart[s] >= 0) && e.streamResampled(s))
			throw smst::Error(std::string(call) + ": stream " + std::to_string(s) + " has the stream-resample setting (smst_batch_set_pcm_stream_resample), which acts in smst_batch_process_pcm and "
			                  "smst_batch_seek_pcm only" + (std::strcmp(call, "smst_batch_exact_pcm") == 0 ? ": the whole-clip form is smst_batch_set_pcm_resample" : ""));
}
// Output resample (include/smst.h): only smst_batch_exact_pcm serves a stream's output ratio.  The other calls that write output refuse where a
// stream that takes part has one
static void refuseOutResampled(const Batch &e, const int *takesPart, const char *call) {
	for (int s = 0; s < e.streams(); ++s)
		if ((!takesPart || takesPart[s] >= 0) && e.outResampled(s))
			throw smst::Error(std::string(call) + ": stream " + std::to_string(s) + " has an output resample ratio other than 1/1 (smst_batch_set_pcm_out_resample): smst_batch_exact_pcm only");
}
// E of a stream's Nd delivered frames, which must fit an int (2*M <= 9*L: E < 4.5*Nd + 1, so a count below 2^40 cannot overflow 64 bits)
static long long outRenderLengthChecked(const Batch &e, int s, long long outSamples) {
	const std::string what = "out resample: stream " + std::to_string(s) + ": " + std::to_string(outSamples) + " delivered frames";
	if (outSamples > (1LL << 40)) throw smst::Error(what + " need more than 2147483647 rendered frames (the length at the batch's rate must fit an int)");
	const long long E = e.outRenderLengthOf(s, outSamples);
	if (E > 0x7fffffffLL) throw smst::Error(what + " need " + std::to_string(E) + " rendered frames, more than 2147483647 (the length at the batch's rate must fit an int)");
	return E;
}
// ... and that call refuses a clip whose length at the batch's rate does not fit an int
static long long resampledLengthChecked(const Batch &e, int s, long long inSamples) {
	if (inSamples > (1LL << 40)) throw smst::Error("resample: stream " + std::to_string(s) + ": " + std::to_string(inSamples) + " frames resample to more than 2147483647 (the length at the batch's rate must fit an int)");
	const long long nr = e.resampledLengthOf(s, inSamples);
	if (nr > 0x7fffffffLL) throw smst::Error("resample: stream " + std::to_string(s) + ": " + std::to_string(inSamples) + " frames resample to " + std::to_string(nr) + ", more than 2147483647 (the length at the batch's rate must fit an int)");
	return nr;
}
static void checkResampledLengths(const Batch &e, const int *inSamples, const int *outSamples) {
	for (int s = 0; s < e.streams(); ++s) if (outSamples[s] >= 0 && e.resampled(s)) resampledLengthChecked(e, s, inSamples[s]);
	for (int s = 0; s < e.streams(); ++s) if (outSamples[s] >= 0 && e.outResampled(s)) outRenderLengthChecked(e, s, outSamples[s]);
}

int smst_batch_exact(smst_batch *b, const float *in, long long iss, long long ics, const int *inSamples,
                     float *out, long long oss, long long ocs, const int *outSamples, int *status, int memory) {
	BATCH_CALL({
		Batch &e = *b->engine;
		checkExactArgs(e, in, inSamples, out, outSamples, 0, 0, false, memory);
		refuseResampled(e, outSamples, "smst_batch_exact");
		refuseOutResampled(e, outSamples, "smst_batch_exact");
		if (memory == SMST_MEM_DEVICE) {
			runExact(e, Batch::ClipIo{in, iss, ics, out, oss, ocs, 0}, inSamples, outSamples, status);
		} else {
			const int S = e.streams(), C = e.channels();
			std::vector<int> nIn, nOut;
			exactCounts(inSamples, outSamples, S, nIn);
			const int maxOut = exactCounts(outSamples, outSamples, S, nOut);
			int maxIn;
			const float *dIn = stageIn(b, in, iss, ics, nIn.data(), maxIn);
			ensureStage(b, b->dOut, (size_t)S*C*maxOut);
			runExact(e, Batch::ClipIo{dIn, (long long)C*maxIn, maxIn, b->dOut, (long long)C*maxOut, maxOut, 0}, inSamples, outSamples, status);
			unstageOut(b, out, oss, ocs, nOut.data(), maxOut);
		}
	})
}
int smst_batch_exact_pcm(smst_batch *b, const void *in, long long iss, long long ifs, const int *inSamples,
                         void *out, long long oss, long long ofs, const int *outSamples, int *status, int format, int memory) {
	BATCH_CALL({
		Batch &e = *b->engine;
		checkPcmFormat(format, memory);
		checkExactArgs(e, in, inSamples, out, outSamples, ifs, ofs, true, memory);
		for (int s = 0; s < e.streams(); ++s)
			if (outSamples[s] >= 0 && b->pcmOut.streamLimit[s].on)
				throw smst::Error("stream " + std::to_string(s) + " has the stream limiter's setting (smst_batch_set_pcm_stream_limiter), which acts in smst_batch_process_pcm and smst_batch_flush_pcm: "
				                  "the whole-clip form is smst_batch_set_pcm_limiter");
		for (int s = 0; s < e.streams(); ++s)
			if (outSamples[s] >= 0 && b->pcmOut.streamMeter[s].on)
				throw smst::Error("stream " + std::to_string(s) + " has the stream meter's setting (smst_batch_set_pcm_stream_meter), which acts in smst_batch_process_pcm and smst_batch_flush_pcm: "
				                  "the whole-clip forms are smst_batch_set_pcm_loudness_range and smst_batch_set_pcm_true_peak");
		refuseStreamResampled(e, outSamples, "smst_batch_exact_pcm");
		for (int s = 0; s < e.streams(); ++s)
			if (outSamples[s] >= 0 && e.streamOutResampled(s))
				throw smst::Error("smst_batch_exact_pcm: stream " + std::to_string(s) + " has the stream-output-resample setting (smst_batch_set_pcm_stream_out_resample), which acts in "
				                  "smst_batch_process_pcm and smst_batch_flush_pcm only: the whole-clip form is smst_batch_set_pcm_out_resample");
		checkResampledLengths(e, inSamples, outSamples);
		// a dithered call: the streams' modes and hashes ride in the _pcm calls' table (the frame index is the place in the clip: the counters
		// are neither read nor moved); a levelled call: the level entries ride there too, and the loudness entries and the channel weights
		smst_batch::PcmTable *table = b->pcmOut.dithers(format) || b->pcmOut.levelled ? &beginPcmCall(b) : nullptr;
		if (table) pcmUploadOutTable(b, *table, format, false);
		smst::PcmOutCall plain;
		plain.overs = b->pcmOut.dOvers;
		Batch::ClipIo io{in, iss, ifs, out, oss, ofs, format};
		b->pcmOut.clipModes(table ? table->out : plain, io);
		io.resample = true; // (checkResampledLengths above: every Nr fits an int)
		io.outResample = true; // (... and every E)
		if (memory == SMST_MEM_DEVICE) {
			runExact(e, io, inSamples, outSamples, status);
		} else {
			const int S = e.streams(), C = e.channels();
			std::vector<int> nIn, nOut;
			const int mostIn = exactCounts(inSamples, outSamples, S, nIn), mostOut = exactCounts(outSamples, outSamples, S, nOut);
			ensurePcmBytes(b, b->hPcmOut, b->dPcmOut, (size_t)S*pcmRowElems(mostOut, C)*pcmElemBytes(format));
			pcmRawIn(b, in, iss, ifs, nIn.data(), mostIn, format);
			io.in = b->dPcmIn; io.inStreamStride = pcmRowElems(mostIn, C); io.inInnerStride = C;
			io.out = b->dPcmOut; io.outStreamStride = pcmRowElems(mostOut, C); io.outInnerStride = C;
			runExact(e, io, inSamples, outSamples, status);
			pcmRawOut(b, out, oss, ofs, nOut.data(), mostOut, format);
		}
		if (table) endPcmCall(b);
	})
}
// Resample (include/smst.h): the streams' ratios live in the engine, beside the tables they select
int smst_batch_set_pcm_resample(smst_batch *b, int stream, int up, int down) { BATCH_CALL(b->engine->setResample(stream, up, down)) }
int smst_batch_pcm_resample(const smst_batch *b, int stream, int *up, int *down) {
	BATCH_CALL({
		int l = 1, m = 1;
		b->engine->resampleOf(stream, l, m);
		if (up) *up = l;
		if (down) *down = m;
	})
}
long long smst_batch_resampled_length(const smst_batch *b, int stream, long long inSamples) {
	if (!b || !b->engine) return fail("null batch");
	SMST_TRY
	if (stream < 0 || stream >= b->engine->streams()) throw smst::Error("stream index out of range");
	if (inSamples < 0) throw smst::Error("resample: negative sample count");
	return resampledLengthChecked(*b->engine, stream, inSamples);
	SMST_CATCH
}
// Output resample (include/smst.h): the ratios live in the engine beside the input side's, whose tables and slots they share
int smst_batch_set_pcm_out_resample(smst_batch *b, int stream, int up, int down) { BATCH_CALL(b->engine->setResample(stream, up, down, Batch::kResampleOut)) }
int smst_batch_pcm_out_resample(const smst_batch *b, int stream, int *up, int *down) {
	BATCH_CALL({
		int l = 1, m = 1;
		b->engine->outResampleOf(stream, l, m);
		if (up) *up = l;
		if (down) *down = m;
	})
}
long long smst_batch_pcm_out_render_length(const smst_batch *b, int stream, long long outSamples) {
	if (!b || !b->engine) return fail("null batch");
	SMST_TRY
	if (stream < 0 || stream >= b->engine->streams()) throw smst::Error("stream index out of range");
	if (outSamples < 0) throw smst::Error("out resample: negative sample count");
	return outRenderLengthChecked(*b->engine, stream, outSamples);
	SMST_CATCH
}
// Stream resample (include/smst.h): the ratios live in the engine beside the whole-clip ones, whose tables and slots they share; the lines,
// the counters and the call tables here.  Everything is allocated by the setter, never in a call
int smst_batch_set_pcm_stream_resample(smst_batch *b, int stream, int up, int down) {
	BATCH_CALL({
		Batch &e = *b->engine;
		e.setResample(stream, up, down, Batch::kResampleStream); // (every refusal, before anything changes)
		hipSetDevice(e.device());
		if (PcmStreamResampleState::any(e) && !b->pcmIn.dLines) {
			const size_t set = (size_t)e.streams()*e.channels()*smst::kStreamResampleLine;
			++b->stagingAllocs;
			b->pcmIn.dLines.allocate(2*set, "stream resample lines");
			if (hipMemsetAsync(b->pcmIn.dLines, 0, 2*set*sizeof(float), e.stream()) != hipSuccess) throw smst::Error("hipMemsetAsync (stream resample lines) failed", true);
			b->pcmTables.create();
			const size_t bytes = smst::StreamResampleTableLayout(e.streams()).bytes();
			for (smst_batch::PcmTable &t : b->pcmTables.sets) {
				t.resHost.allocate(bytes, "stream resample table");
				t.resDev.allocate(bytes, "stream resample table");
			}
			b->pcmIn.tableBytes = 2*bytes;
		}
		b->pcmIn.clear(stream);
	})
}
int smst_batch_pcm_stream_resample(const smst_batch *b, int stream, int *up, int *down) {
	BATCH_CALL({
		int l = 1, m = 1;
		b->engine->streamResampleOf(stream, l, m);
		if (up) *up = l;
		if (down) *down = m;
	})
}
int smst_batch_pcm_stream_resample_latency(const smst_batch *b, int stream, int *frames) {
	BATCH_CALL({
		if (stream < 0 || stream >= b->engine->streams()) throw smst::Error("stream index out of range");
		if (frames) *frames = b->engine->streamResampled(stream) ? b->engine->streamResampleShape(stream).H : 0;
	})
}
long long smst_batch_pcm_stream_resample_frames(const smst_batch *b, int stream, long long inSamples, int fresh) {
	if (!b || !b->engine) return fail("null batch");
	SMST_TRY
	if (stream < 0 || stream >= b->engine->streams()) throw smst::Error("stream index out of range");
	if (inSamples < 0) throw smst::Error("stream resample: negative sample count");
	return b->pcmIn.framesOf(*b->engine, stream, inSamples, fresh != 0 || b->pcmIn.stream[stream].fresh);
	SMST_CATCH
}
long long smst_batch_pcm_stream_resample_need(const smst_batch *b, int stream, long long frames, int fresh) {
	if (!b || !b->engine) return fail("null batch");
	SMST_TRY
	const Batch &e = *b->engine;
	if (stream < 0 || stream >= e.streams()) throw smst::Error("stream index out of range");
	if (frames < 1 || frames > 0x7fffffffLL) throw smst::Error("stream resample: the frame count is below 1 or does not fit an int (1 ... 2147483647)");
	if (!e.streamResampled(stream)) return frames;
	const smst::ResampleShape &g = e.streamResampleShape(stream);
	const PcmStreamResampleState::Stream &st = b->pcmIn.stream[stream];
	const long long fed = fresh ? 0 : st.fed, made = fresh ? 0 : st.made;
	return std::max(0LL, ((made + frames - 1)*g.M)/g.L + g.H + 1 - fed);
	SMST_CATCH
}
// Stream output resample (include/smst.h): the ratios live in the engine beside the three others, whose tables and slots they share; the
// lines, the counters and the call tables here.  Everything but the image of the delivered frames is allocated by the setter, never in a call
int smst_batch_set_pcm_stream_out_resample(smst_batch *b, int stream, int up, int down) {
	BATCH_CALL({
		Batch &e = *b->engine;
		e.setResample(stream, up, down, Batch::kResampleStreamOut); // (every refusal, before anything changes)
		hipSetDevice(e.device());
		if (PcmStreamResampleOutState::any(e) && !b->pcmOutRes.dLines) {
			const size_t set = (size_t)e.streams()*e.channels()*smst::kStreamResampleOutLine;
			++b->stagingAllocs;
			b->pcmOutRes.dLines.allocate(2*set, "stream out resample lines");
			if (hipMemsetAsync(b->pcmOutRes.dLines, 0, 2*set*sizeof(float), e.stream()) != hipSuccess) throw smst::Error("hipMemsetAsync (stream out resample lines) failed", true);
			b->pcmTables.create();
			const size_t bytes = smst::StreamResampleOutTableLayout(e.streams()).bytes();
			for (smst_batch::PcmTable &t : b->pcmTables.sets) {
				t.outResHost.allocate(bytes, "stream out resample table");
				t.outResDev.allocate(bytes, "stream out resample table");
			}
			b->pcmOutRes.tableBytes = 2*bytes;
		}
		b->pcmOutRes.clear(stream);
	})
}
int smst_batch_pcm_stream_out_resample(const smst_batch *b, int stream, int *up, int *down) {
	BATCH_CALL({
		int l = 1, m = 1;
		b->engine->streamOutResampleOf(stream, l, m);
		if (up) *up = l;
		if (down) *down = m;
	})
}
int smst_batch_pcm_stream_out_resample_latency(const smst_batch *b, int stream, int *frames) {
	BATCH_CALL({
		const Batch &e = *b->engine;
		if (stream < 0 || stream >= e.streams()) throw smst::Error("stream index out of range");
		if (frames) *frames = 0;
		if (frames && e.streamOutResampled(stream)) { const smst::ResampleShape &g = e.streamOutResampleShape(stream); *frames = smst::streamResampleOutLatency(g.L, g.M, g.H); }
	})
}
long long smst_batch_pcm_stream_out_resample_render(const smst_batch *b, int stream, long long outSamples, int fresh) {
	if (!b || !b->engine) return fail("null batch");
	SMST_TRY
	if (stream < 0 || stream >= b->engine->streams()) throw smst::Error("stream index out of range");
	if (outSamples < 0) throw smst::Error("stream out resample: negative sample count");
	return b->pcmOutRes.renderOf(*b->engine, stream, outSamples, fresh != 0 || b->pcmOutRes.stream[stream].fresh);
	SMST_CATCH
}
int smst_resample_ratio(double fromRate, double toRate, int *up, int *down) {
	SMST_TRY
	for (double rate : {fromRate, toRate})
		if (!(std::isfinite(rate) && rate >= 1 && rate <= 1e9 && rate == std::floor(rate))) throw smst::Error("resample: a sample rate is not a positive integer (at most 1e9)");
	long long a = (long long)toRate, c = (long long)fromRate, x = a, y = c;
	while (y) { const long long r = x%y; x = y; y = r; }
	a /= x; c /= x;
	if (a > smst::kResampleMaxTerm || c > smst::kResampleMaxTerm)
		throw smst::Error("resample: " + std::to_string((long long)fromRate) + " -> " + std::to_string((long long)toRate) + " Hz reduces to " + std::to_string(a) + "/" + std::to_string(c) +
		                  ", a term above " + std::to_string(smst::kResampleMaxTerm) + " (SMST_RESAMPLE_MAX_TERM)");
	int l = int(a), m = int(c);
	smst::resampleReduce(l, m);
	if (up) *up = l;
	if (down) *down = m;
	return SMST_OK;
	SMST_CATCH
}
} // extern "C"
// What the two debug converters are: the launch of one conversion kernel on device copies of the caller's buffers, which sit as far behind a
// 16-byte boundary as the caller's own do; the launch's table (the counts, or the segments) and, uploaded in front of everything, `first`
// (the dither entries, a levelled hook's DebugLevel block behind them; 0 bytes: none; firstBack, may be null: where it is read back to); the
// overs zeroed and, `counted`, read back.  launch(src, dst, table, first, overs) runs on the null stream.  name: the hook's, in front of a HIP error.
template <typename Launch> static void debugConvert(const std::string &name, int streams, const void *src, size_t srcBytes, void *dst, size_t dstBytes, const void *table, size_t tableBytes,
		const void *first, size_t firstBytes, bool counted, long long *clamped, long long *nans, Launch launch, void *firstBack = nullptr) {
	auto hip = [&](hipError_t err) { if (err != hipSuccess) throw smst::Error(name + ": " + hipGetErrorString(err), true); };
	Buffer<unsigned char, false> dSrc, dDst, dTable, dFirst, dOvers; // freed when the function leaves, whichever way
	std::vector<unsigned> overs((size_t)2*streams, 0u);
	dSrc.allocate(srcBytes + 32, name.c_str());
	if (firstBytes) {
		dFirst.allocate(firstBytes, name.c_str());
		hip(hipMemcpy(dFirst, first, firstBytes, hipMemcpyHostToDevice));
	}
	dDst.allocate(dstBytes + 32, name.c_str());
	dTable.allocate(tableBytes, name.c_str());
	unsigned char *s0 = dSrc + reinterpret_cast<uintptr_t>(src)%16, *d0 = dDst + reinterpret_cast<uintptr_t>(dst)%16;
	if (srcBytes) hip(hipMemcpy(s0, src, srcBytes, hipMemcpyHostToDevice));
	if (dstBytes) hip(hipMemcpy(d0, dst, dstBytes, hipMemcpyHostToDevice));
	hip(hipMemcpy(dTable, table, tableBytes, hipMemcpyHostToDevice));
	if (counted) {
		dOvers.allocate(pcmOversBytes(streams), name.c_str());
		hip(hipMemcpy(dOvers, overs.data(), pcmOversBytes(streams), hipMemcpyHostToDevice));
	}
	launch(s0, d0, dTable.p, dFirst.p, reinterpret_cast<unsigned *>(dOvers.p));
	hip(hipGetLastError());
	hip(hipStreamSynchronize(nullptr));
	if (dstBytes) hip(hipMemcpy(dst, d0, dstBytes, hipMemcpyDeviceToHost));
	if (counted) hip(hipMemcpy(overs.data(), dOvers, pcmOversBytes(streams), hipMemcpyDeviceToHost));
	if (firstBack && firstBytes) hip(hipMemcpy(firstBack, dFirst, firstBytes, hipMemcpyDeviceToHost));
	for (int s = 0; s < streams; ++s) {
		if (clamped) clamped[s] = overs[2*s];
		if (nans) nans[s] = overs[2*s + 1];
	}
}
// A levelled hook's `first` block (smst::PcmDebugBlock): the dither entries (always present, mode 0 where the hook has none), the level
// entries, the meter words of a fresh batch.  io(base): the launch's PcmLevelIo where the block lies at `base`; results(): the peaks and the applied gains
struct DebugLevel {
	smst::PcmDebugBlock at;
	std::vector<unsigned char> block;
	DebugLevel(int streams, const std::vector<smst::PcmDither> &dither, const int *modes, const float *gains, const float *ceilings) : at(streams), block(at.bytes()) {
		for (int s = 0; s < streams; ++s) {
			const int mode = modes ? modes[s] : SMST_LEVEL_FIXED;
			checkPcmLevel(mode, gains[s], ceilings ? ceilings[s] : 1.0f);
			at.dither(block.data())[s] = dither[s];
			at.level(block.data())[s] = smst::PcmLevel{unsigned(mode), gains[s], ceilings ? ceilings[s] : 1.0f, 0u};
		}
		at.meters.start(at.words(block.data()));
	}
	smst::PcmLevelIo io(unsigned char *base) const { return at.meters.io(at.level(base), at.words(base)); }
	void results(float *peaks, float *applied) { at.meters.taken(at.words(block.data()), peaks, applied); }
};
static int pcmConvert(int device, int dir, int format, int streams, int channels, const int *counts,
                      const void *src, long long srcSS, long long srcInner, void *dst, long long dstSS, long long dstInner, long long *clamped, long long *nans,
                      const int *modes = nullptr, const long long *seeds = nullptr, const long long *firstFrames = nullptr, const float *gains = nullptr, float *peaks = nullptr) {
	SMST_TRY
	checkPcmFormat(format, SMST_MEM_HOST);
	if (dir != 0 && dir != 1) throw smst::Error("pcm convert: dir is 0 (PCM -> planar) or 1 (planar -> PCM)");
	if (streams < 1 || channels < 1 || channels > 16 || !counts || !src || !dst || srcSS < 0 || dstSS < 0 || srcInner < 0 || dstInner < 0) throw smst::Error("pcm convert: bad arguments");
	for (int s = 0; s < streams; ++s) if (counts[s] < 0) throw smst::Error("negative sample count");
	const int most = countsOf(counts, streams).most;
	const long long pcmFS = dir == 0 ? srcInner : dstInner;
	if (pcmFS < channels) throw smst::Error("frame stride smaller than the channel count");
	const size_t esz = pcmElemBytes(format);
	// elements either side spans, from its base
	const long long pcmSS = dir == 0 ? srcSS : dstSS, plSS = dir == 0 ? dstSS : srcSS, plCS = dir == 0 ? dstInner : srcInner;
	const size_t pcmBytes = most ? size_t((streams - 1)*pcmSS + (most - 1)*pcmFS + channels)*esz : 0;
	const size_t plBytes = most ? size_t((streams - 1)*plSS + (channels - 1)*plCS + most)*sizeof(float) : 0;
	const size_t srcBytes = dir == 0 ? pcmBytes : plBytes, dstBytes = dir == 0 ? plBytes : pcmBytes;
	if (hipSetDevice(device) != hipSuccess) throw smst::Error("hipSetDevice failed", true);
	// the streams' dither entries (dir 1); a launch is a dithered one when a stream has a mode
	std::vector<smst::PcmDither> dither;
	bool dithered = false;
	if (modes) {
		if (!seeds || !firstFrames) throw smst::Error("pcm convert: null seeds or first frames");
		for (int s = 0; s < streams; ++s) {
			checkDitherMode(modes[s]);
			const unsigned long long n = (unsigned long long)firstFrames[s];
			dither.push_back(smst::PcmDither{unsigned(modes[s]), smst::pcmDitherHash(seeds[s]), unsigned(n), unsigned(n >> 32)});
			dithered = dithered || modes[s] != SMST_DITHER_NONE;
		}
	}
	if (gains) { // the levelled kernel: fixed gains, the meters of a fresh batch
		DebugLevel level(streams, dither, nullptr, gains, nullptr);
		debugConvert("pcm convert", streams, src, srcBytes, dst, dstBytes, counts, streams*sizeof(int), level.block.data(), level.block.size(), clamped || nans, clamped, nans,
		             [&](unsigned char *s0, unsigned char *d0, const unsigned char *dCounts, unsigned char *dFirst, unsigned *dOvers) {
			smst::launchPcmOut(format, reinterpret_cast<const float *>(s0), srcSS, srcInner, d0, dstSS, dstInner, reinterpret_cast<const int *>(dCounts), streams, channels, most, dOvers, nullptr,
			                   dithered ? level.at.dither(dFirst) : nullptr, level.io(dFirst));
		}, level.block.data());
		level.results(peaks, nullptr);
		return SMST_OK;
	}
	debugConvert("pcm convert", streams, src, srcBytes, dst, dstBytes, counts, streams*sizeof(int), dither.data(), dithered ? streams*sizeof(smst::PcmDither) : 0,
	             dir == 1 && (clamped || nans), clamped, nans, [&](unsigned char *s0, unsigned char *d0, const unsigned char *dCounts, unsigned char *dDither, unsigned *dOvers) {
		const int *n = reinterpret_cast<const int *>(dCounts);
		if (dir == 0) smst::launchPcmIn(format, s0, srcSS, srcInner, reinterpret_cast<float *>(d0), dstSS, dstInner, n, streams, channels, most, nullptr);
		else smst::launchPcmOut(format, reinterpret_cast<const float *>(s0), srcSS, srcInner, d0, dstSS, dstInner, n, streams, channels, most, dOvers, nullptr, smst::PcmDebugBlock(streams).dither(dDither));
	});
	return SMST_OK;
	SMST_CATCH
}
extern "C" {
int smst_debug_pcm_convert(int device, int dir, int format, int streams, int channels, const int *counts,
                           const void *src, long long srcSS, long long srcInner, void *dst, long long dstSS, long long dstInner) {
	return pcmConvert(device, dir, format, streams, channels, counts, src, srcSS, srcInner, dst, dstSS, dstInner, nullptr, nullptr);
}
int smst_debug_pcm_convert_counted(int device, int format, int streams, int channels, const int *counts,
                                   const void *src, long long srcSS, long long srcInner, void *dst, long long dstSS, long long dstInner,
                                   long long *clamped, long long *nans) {
	if (!clamped || !nans) return fail("pcm convert: null count arrays");
	return pcmConvert(device, 1, format, streams, channels, counts, src, srcSS, srcInner, dst, dstSS, dstInner, clamped, nans);
}
int smst_debug_pcm_convert_dithered(int device, int format, int streams, int channels, const int *counts,
                                    const void *src, long long srcSS, long long srcInner, void *dst, long long dstSS, long long dstInner,
                                    const int *modes, const long long *seeds, const long long *firstFrames, long long *clamped, long long *nans) {
	if (!modes || !seeds || !firstFrames) return fail("pcm convert: null dither arrays");
	return pcmConvert(device, 1, format, streams, channels, counts, src, srcSS, srcInner, dst, dstSS, dstInner, clamped, nans, modes, seeds, firstFrames);
}
int smst_debug_pcm_convert_levelled(int device, int format, int streams, int channels, const int *counts,
                                    const void *src, long long srcSS, long long srcInner, void *dst, long long dstSS, long long dstInner,
                                    const int *modes, const long long *seeds, const long long *firstFrames, const float *gains, long long *clamped, long long *nans, float *peaks) {
	if (!modes || !seeds || !firstFrames || !gains) return fail("pcm convert: null dither or gain arrays");
	return pcmConvert(device, 1, format, streams, channels, counts, src, srcSS, srcInner, dst, dstSS, dstInner, clamped, nans, modes, seeds, firstFrames, gains, peaks);
}
} // extern "C"
// the clip kernels alone (smst_clip.h): see include/smst.h.  levelModes set: kClipPeak and the levelled kClipOut, into a frame format
static int clipCopy(int device, int dir, int format, int streams, int channels, const int *segments,
                    const void *src, long long srcSS, long long srcInner, void *dst, long long dstSS, long long dstInner, long long *clamped, long long *nans,
                    const int *levelModes = nullptr, const float *gains = nullptr, const float *ceilings = nullptr, const int *ditherModes = nullptr, const long long *seeds = nullptr,
                    float *peaks = nullptr, float *applied = nullptr) {
	SMST_TRY
	if (format != 0) checkPcmFormat(format, SMST_MEM_HOST);
	if (dir != 0 && dir != 1) throw smst::Error("clip copy: dir is 0 (caller's buffer -> planar image) or 1 (planar image -> caller's buffer)");
	if (streams < 1 || channels < 1 || channels > 16 || !segments || !src || !dst || srcSS < 0 || dstSS < 0 || srcInner < 0 || dstInner < 0) throw smst::Error("clip copy: bad arguments");
	// frames either side spans from its base, and the largest count
	int srcEnd = 0, dstEnd = 0, most = 0;
	for (int k = 0; k < 2*streams; ++k) {
		const int *g = segments + 4*k;
		if (g[0] < 0 || g[1] < 0 || g[2] < 0) throw smst::Error("clip copy: negative segment offset or count");
		if (g[2] == 0) continue;
		if (!g[3]) srcEnd = std::max(srcEnd, g[0] + g[2]);
		dstEnd = std::max(dstEnd, g[1] + g[2]);
		most = std::max(most, g[2]);
	}
	// dir 0: src is the caller's side (frames of `format`, or planar for 0), dst the planar image; dir 1: the reverse
	const bool srcFrames = dir == 0 && format != 0, dstFrames = dir == 1 && format != 0;
	if ((srcFrames && srcInner < channels) || (dstFrames && dstInner < channels)) throw smst::Error("frame stride smaller than the channel count");
	auto spanBytes = [&](bool frames, int end, long long ss, long long inner) -> size_t {
		if (!end) return 0;
		return frames ? size_t((streams - 1)*ss + (end - 1)*inner + channels)*pcmElemBytes(format) : size_t((streams - 1)*ss + (channels - 1)*inner + end)*sizeof(float);
	};
	const size_t srcBytes = spanBytes(srcFrames, srcEnd, srcSS, srcInner), dstBytes = spanBytes(dstFrames, dstEnd, dstSS, dstInner);
	if (hipSetDevice(device) != hipSuccess) throw smst::Error("hipSetDevice failed", true);
	if (levelModes) {
		std::vector<smst::PcmDither> dither;
		bool dithered = false;
		for (int s = 0; s < streams; ++s) {
			checkDitherMode(ditherModes[s]);
			dither.push_back(smst::PcmDither{unsigned(ditherModes[s]), smst::pcmDitherHash(seeds[s]), 0u, 0u});
			dithered = dithered || ditherModes[s] != SMST_DITHER_NONE;
		}
		dithered = dithered && (format == SMST_PCM_S16 || format == SMST_PCM_S24);
		DebugLevel level(streams, dither, levelModes, gains, ceilings);
		debugConvert("clip copy", streams, src, srcBytes, dst, dstBytes, segments, (size_t)2*streams*sizeof(smst::ClipSeg), level.block.data(), level.block.size(), clamped || nans, clamped, nans,
		             [&](unsigned char *s0, unsigned char *d0, const unsigned char *dSegs, unsigned char *dFirst, unsigned *dOvers) {
			const smst::ClipSeg *segs = reinterpret_cast<const smst::ClipSeg *>(dSegs);
			const smst::PcmLevelIo io = level.io(dFirst);
			smst::launchClipPeak(reinterpret_cast<const float *>(s0), srcSS, srcInner, segs, streams, channels, most, io.clipPeak, nullptr);
			smst::launchClipOut(format, reinterpret_cast<const float *>(s0), srcSS, srcInner, d0, dstSS, dstInner, segs, streams, channels, most, dOvers, nullptr,
			                    dithered ? level.at.dither(dFirst) : nullptr, io);
		}, level.block.data());
		level.results(peaks, applied);
		return SMST_OK;
	}
	debugConvert("clip copy", streams, src, srcBytes, dst, dstBytes, segments, (size_t)2*streams*sizeof(smst::ClipSeg), nullptr, 0, dstFrames && (clamped || nans), clamped, nans,
	             [&](unsigned char *s0, unsigned char *d0, const unsigned char *dSegs, const unsigned char *, unsigned *dOvers) {
		const smst::ClipSeg *segs = reinterpret_cast<const smst::ClipSeg *>(dSegs);
		if (dir == 0) smst::launchClipIn(format, s0, srcSS, srcInner, reinterpret_cast<float *>(d0), dstSS, dstInner, segs, streams, channels, most, nullptr);
		else smst::launchClipOut(format, reinterpret_cast<const float *>(s0), srcSS, srcInner, d0, dstSS, dstInner, segs, streams, channels, most, dOvers, nullptr);
	});
	return SMST_OK;
	SMST_CATCH
}
extern "C" {
int smst_debug_clip_copy(int device, int dir, int format, int streams, int channels, const int *segments,
                         const void *src, long long srcSS, long long srcInner, void *dst, long long dstSS, long long dstInner,
                         long long *clamped, long long *nans) {
	return clipCopy(device, dir, format, streams, channels, segments, src, srcSS, srcInner, dst, dstSS, dstInner, clamped, nans);
}
int smst_debug_clip_copy_levelled(int device, int format, int streams, int channels, const int *segments,
                                  const void *src, long long srcSS, long long srcInner, void *dst, long long dstSS, long long dstInner,
                                  const int *levelModes, const float *gains, const float *ceilings, const int *ditherModes, const long long *seeds,
                                  long long *clamped, long long *nans, float *peaks, float *applied) {
	if (format == 0) return fail("clip copy: the levelled form writes frames of an SMST_PCM_* format");
	if (!levelModes || !gains || !ceilings || !ditherModes || !seeds) return fail("clip copy: null level or dither arrays");
	return clipCopy(device, 1, format, streams, channels, segments, src, srcSS, srcInner, dst, dstSS, dstInner, clamped, nans, levelModes, gains, ceilings, ditherModes, seeds, peaks, applied);
}
} // extern "C"
// the four passes on a caller's image and, range != null, kLoudRange behind them with every stream metered
struct DebugRange { const double *capsLufs; double *momentaryMax, *shortTermMax, *low, *high; int *shortBlocks, *rangeBlocks; double *shortPowers; };
static int debugClipLoudness(int device, int streams, int channels, const int *segments, const float *image, long long imageSS, long long imageCS,
                             const double *sampleRates, const float *weights, double targetLufs, double *Z, int *blocks, int *gated, float *gains, double *blockPowers, int maxBlocks,
                             const DebugRange *range) {
	SMST_TRY
	if (streams < 1 || channels < 1 || channels > smst::kMaxChannels || !segments || !image || imageSS < 0 || imageCS < 0 || !sampleRates || maxBlocks < 0) throw smst::Error("clip loudness: bad arguments");
	auto hip = [&](hipError_t err) { if (err != hipSuccess) throw smst::Error(std::string("clip loudness: ") + hipGetErrorString(err), true); };
	std::vector<smst::LoudEntry> entries((size_t)streams);
	int end = 0, most = 0, maxSub = 1;
	for (int s = 0; s < streams; ++s) {
		const int *g = segments + 8*s;
		if (g[0] < 0 || g[2] < 0 || g[4] < 0 || g[6] < 0) throw smst::Error("clip loudness: negative segment offset or count");
		if ((long long)g[2] + g[6] > 0x7fffffff) throw smst::Error("clip loudness: the clip is too long");
		if (!smst::loudEntryOf(sampleRates[s], targetLufs, entries[s])) throw smst::Error("clip loudness: bad sample rate");
		if (range) {
			entries[s].meter = 1;
			for (int k = 0; range->capsLufs && k < 2; ++k) {
				const double cap = range->capsLufs[2*s + k];
				if (std::isnan(cap) || cap == -INFINITY) throw smst::Error("clip loudness: a cap is NaN or -inf");
				(k ? entries[s].Ps : entries[s].Pm) = std::isfinite(cap) ? std::pow(10.0, (cap + 0.691)/10) : double(INFINITY);
			}
		}
		for (int k = 0; k < 2; ++k) if (g[4*k + 2] > 0 && !g[4*k + 3]) end = std::max(end, g[4*k] + g[4*k + 2]);
		most = std::max(most, g[2] + g[6]);
		maxSub = std::max(maxSub, (g[2] + g[6])/entries[s].h + 1);
	}
	std::vector<float> w((size_t)smst::kMaxChannels, 0.0f);
	for (int c = 0; c < channels; ++c) {
		w[c] = weights ? weights[c] : 1.0f;
		if (!(std::isfinite(w[c]) && w[c] >= 0)) throw smst::Error("loudness: a channel weight is negative or not finite");
	}
	hip(hipSetDevice(device));
	const size_t imageBytes = end ? size_t((streams - 1)*imageSS + (channels - 1)*imageCS + end)*sizeof(float) : 0;
	const int maxChunks = std::max((most + smst::kLoudChunk - 1)/smst::kLoudChunk, 1);
	Buffer<unsigned char, false> dImage, dSegs, dEntries, dWeights;
	Buffer<double, false> dScratch, dRange;
	dImage.allocate(imageBytes + 32, "clip loudness");
	dSegs.allocate((size_t)2*streams*sizeof(smst::ClipSeg), "clip loudness");
	dEntries.allocate(entries.size()*sizeof(smst::LoudEntry), "clip loudness");
	dWeights.allocate(w.size()*sizeof(float), "clip loudness");
	dScratch.allocate(smst::loudScratchDoubles(streams, channels, maxChunks, maxSub), "clip loudness");
	if (range) dRange.allocate(smst::loudRangeDoubles(streams, maxSub), "clip loudness");
	unsigned char *i0 = dImage + reinterpret_cast<uintptr_t>(image)%16; // (as far behind a 16-byte boundary as the caller's image)
	if (imageBytes) hip(hipMemcpy(i0, image, imageBytes, hipMemcpyHostToDevice));
	hip(hipMemcpy(dSegs, segments, (size_t)2*streams*sizeof(smst::ClipSeg), hipMemcpyHostToDevice));
	hip(hipMemcpy(dEntries, entries.data(), entries.size()*sizeof(smst::LoudEntry), hipMemcpyHostToDevice));
	hip(hipMemcpy(dWeights, w.data(), w.size()*sizeof(float), hipMemcpyHostToDevice));
	const smst::LoudScratch at = smst::loudScratchAt(dScratch, streams, channels, maxChunks, maxSub);
	smst::launchClipLoudness(reinterpret_cast<const float *>(i0), imageSS, imageCS, reinterpret_cast<const smst::ClipSeg *>(dSegs.p), streams, channels,
	                         reinterpret_cast<const smst::LoudEntry *>(dEntries.p), reinterpret_cast<const float *>(dWeights.p), at, nullptr);
	const smst::LoudRangeScratch rangeAt = range ? smst::loudRangeAt(dRange, streams, maxSub) : smst::LoudRangeScratch{};
	if (range) smst::launchClipLoudnessRange(reinterpret_cast<const smst::ClipSeg *>(dSegs.p), streams, channels, reinterpret_cast<const smst::LoudEntry *>(dEntries.p),
	                                         reinterpret_cast<const float *>(dWeights.p), at, rangeAt, nullptr);
	hip(hipGetLastError());
	hip(hipStreamSynchronize(nullptr));
	if (range) {
		std::vector<double> m((size_t)4*streams);
		std::vector<int> k((size_t)2*streams);
		hip(hipMemcpy(m.data(), rangeAt.meters, m.size()*sizeof(double), hipMemcpyDeviceToHost));
		hip(hipMemcpy(k.data(), rangeAt.counts, k.size()*sizeof(int), hipMemcpyDeviceToHost));
		for (int s = 0; s < streams; ++s) {
			if (range->momentaryMax) range->momentaryMax[s] = m[4*s];
			if (range->shortTermMax) range->shortTermMax[s] = m[4*s + 1];
			if (range->low) range->low[s] = m[4*s + 2];
			if (range->high) range->high[s] = m[4*s + 3];
			if (range->shortBlocks) range->shortBlocks[s] = k[2*s];
			if (range->rangeBlocks) range->rangeBlocks[s] = k[2*s + 1];
			const int ns = std::min(k[2*s], maxBlocks);
			if (range->shortPowers && ns > 0) hip(hipMemcpy(range->shortPowers + (size_t)s*maxBlocks, rangeAt.st + (size_t)s*maxSub, (size_t)ns*sizeof(double), hipMemcpyDeviceToHost));
		}
	}
	std::vector<int> counts((size_t)2*streams);
	hip(hipMemcpy(counts.data(), at.counts, counts.size()*sizeof(int), hipMemcpyDeviceToHost));
	if (Z) hip(hipMemcpy(Z, at.Z, (size_t)streams*sizeof(double), hipMemcpyDeviceToHost));
	if (gains) hip(hipMemcpy(gains, at.gain, (size_t)streams*sizeof(float), hipMemcpyDeviceToHost));
	for (int s = 0; s < streams; ++s) {
		if (blocks) blocks[s] = counts[2*s];
		if (gated) gated[s] = counts[2*s + 1];
		const int *g = segments + 8*s;
		const int N = (g[3] || g[7]) ? 0 : g[2] + g[6], h = entries[s].h, nb = N >= 4*h ? (N - 4*h)/h + 1 : 0;
		if (blockPowers && std::min(nb, maxBlocks) > 0) hip(hipMemcpy(blockPowers + (size_t)s*maxBlocks, at.z + (size_t)s*maxSub, (size_t)std::min(nb, maxBlocks)*sizeof(double), hipMemcpyDeviceToHost));
	}
	return SMST_OK;
	SMST_CATCH
}
extern "C" {
int smst_debug_clip_loudness(int device, int streams, int channels, const int *segments, const float *image, long long imageSS, long long imageCS,
                             const double *sampleRates, const float *weights, double targetLufs, double *Z, int *blocks, int *gated, float *gains, double *blockPowers, int maxBlocks) {
	return debugClipLoudness(device, streams, channels, segments, image, imageSS, imageCS, sampleRates, weights, targetLufs, Z, blocks, gated, gains, blockPowers, maxBlocks, nullptr);
}
int smst_debug_clip_loudness_range(int device, int streams, int channels, const int *segments, const float *image, long long imageSS, long long imageCS,
                                   const double *sampleRates, const float *weights, double targetLufs, const double *capsLufs,
                                   double *momentaryMax, double *shortTermMax, double *low, double *high, int *shortBlocks, int *rangeBlocks,
                                   float *gains, double *shortPowers, int maxBlocks) {
	const DebugRange range{capsLufs, momentaryMax, shortTermMax, low, high, shortBlocks, rangeBlocks, shortPowers};
	return debugClipLoudness(device, streams, channels, segments, image, imageSS, imageCS, sampleRates, weights, targetLufs, nullptr, nullptr, nullptr, gains, nullptr, maxBlocks, &range);
}
// the true-peak pass alone, and kClipPeak beside it: see include/smst.h
int smst_debug_clip_true_peak(int device, int streams, int channels, const int *segments, const float *image, long long imageSS, long long imageCS,
                              float *truePeaks, float *samplePeaks, const int *flags) {
	SMST_TRY
	if (streams < 1 || channels < 1 || channels > smst::kMaxChannels || !segments || !image || imageSS < 0 || imageCS < 0) throw smst::Error("clip true peak: bad arguments");
	auto hip = [&](hipError_t err) { if (err != hipSuccess) throw smst::Error(std::string("clip true peak: ") + hipGetErrorString(err), true); };
	std::vector<smst::PcmLevel> level((size_t)streams);
	int end = 0, most = 0, mostSegment = 0;
	for (int s = 0; s < streams; ++s) {
		const int *g = segments + 8*s;
		if (g[0] < 0 || g[2] < 0 || g[4] < 0 || g[6] < 0) throw smst::Error("clip true peak: negative segment offset or count");
		if ((long long)g[2] + g[6] > 0x7fffffff) throw smst::Error("clip true peak: the clip is too long");
		for (int k = 0; k < 2; ++k) if (g[4*k + 2] > 0 && !g[4*k + 3]) end = std::max(end, g[4*k] + g[4*k + 2]);
		most = std::max(most, g[2] + g[6]);
		mostSegment = std::max(mostSegment, std::max(g[2], g[6]));
		level[s] = smst::PcmLevel{smst::kPcmLevelFixed, 1.0f, 1.0f, (!flags || flags[s]) ? smst::kPcmFlagTruePeak : 0u};
	}
	hip(hipSetDevice(device));
	const size_t imageBytes = end ? size_t((streams - 1)*imageSS + (channels - 1)*imageCS + end)*sizeof(float) : 0;
	Buffer<unsigned char, false> dImage, dSegs, dLevel;
	Buffer<int, false> dWords; // [2][streams]: true peaks, sample peaks
	dImage.allocate(imageBytes + 32, "clip true peak");
	dSegs.allocate((size_t)2*streams*sizeof(smst::ClipSeg), "clip true peak");
	dLevel.allocate(level.size()*sizeof(smst::PcmLevel), "clip true peak");
	dWords.allocate((size_t)2*streams, "clip true peak");
	unsigned char *i0 = dImage + reinterpret_cast<uintptr_t>(image)%16; // (as far behind a 16-byte boundary as the caller's image)
	if (imageBytes) hip(hipMemcpy(i0, image, imageBytes, hipMemcpyHostToDevice));
	hip(hipMemcpy(dSegs, segments, (size_t)2*streams*sizeof(smst::ClipSeg), hipMemcpyHostToDevice));
	hip(hipMemcpy(dLevel, level.data(), level.size()*sizeof(smst::PcmLevel), hipMemcpyHostToDevice));
	hip(hipMemset(dWords, 0, (size_t)2*streams*sizeof(int)));
	const smst::ClipSeg *segs = reinterpret_cast<const smst::ClipSeg *>(dSegs.p);
	smst::launchClipTruePeak(reinterpret_cast<const float *>(i0), imageSS, imageCS, segs, streams, channels, most, reinterpret_cast<const smst::PcmLevel *>(dLevel.p), dWords, nullptr);
	smst::launchClipPeak(reinterpret_cast<const float *>(i0), imageSS, imageCS, segs, streams, channels, mostSegment, dWords + streams, nullptr);
	hip(hipGetLastError());
	hip(hipStreamSynchronize(nullptr));
	if (truePeaks) hip(hipMemcpy(truePeaks, dWords, (size_t)streams*sizeof(float), hipMemcpyDeviceToHost));
	if (samplePeaks) hip(hipMemcpy(samplePeaks, dWords + streams, (size_t)streams*sizeof(float), hipMemcpyDeviceToHost));
	return SMST_OK;
	SMST_CATCH
}
// the stream meter's updates and readings alone, on a state of the hook's own: see include/smst.h
int smst_debug_pcm_stream_meter(int device, int streams, int channels, int calls, const int *counts, const int *readAfter, int form,
                                const float *image, long long imageSS, long long imageCS,
                                const double *sampleRates, const float *weights, const int *flags, int maxSubBlocks,
                                double *Z, int *blocks, int *gated, double *momentaryMax, double *shortTermMax, double *low, double *high,
                                int *shortBlocks, int *rangeBlocks, float *truePeaks, float *samplePeaks, long long *metered,
                                double *blockPowers, double *shortPowers, int maxBlocks) {
	SMST_TRY
	const int S = streams, Cn = channels;
	if (S < 1 || Cn < 1 || Cn > smst::kMaxChannels || calls < 1 || !counts || !image || imageSS < 0 || imageCS < 0 || !sampleRates || maxBlocks < 0) throw smst::Error("stream meter: bad arguments");
	if (form < 0 || form > 2) throw smst::Error("stream meter: unknown form (0: the library's choice, 1: the short-call form, 2: the chunk-scan form)");
	if (maxSubBlocks < 1) throw smst::Error("stream meter: maxSubBlocks is below 1");
	auto hip = [&](hipError_t err) { if (err != hipSuccess) throw smst::Error(std::string("stream meter: ") + hipGetErrorString(err), true); };
	PcmOutState state; // (the batch's own host side: settings, counters, a reading)
	state.S = S; state.C = Cn;
	state.streamMeter.assign((size_t)S, PcmOutState::StreamMeter());
	state.loudWeights.assign((size_t)Cn, 1.0f);
	for (int c = 0; c < Cn; ++c) {
		if (weights) state.loudWeights[c] = weights[c];
		if (!(std::isfinite(state.loudWeights[c]) && state.loudWeights[c] >= 0)) throw smst::Error("loudness: a channel weight is negative or not finite");
	}
	std::vector<int> starts((size_t)calls*S, 0);
	std::vector<long long> total((size_t)S, 0);
	for (int k = 0; k < calls; ++k)
		for (int s = 0; s < S; ++s) {
			if (total[s] > 0x7fffffffLL) throw smst::Error("stream meter: a stream's frames do not fit an int");
			starts[(size_t)k*S + s] = int(total[s]);
			total[s] += std::max(counts[(size_t)k*S + s], 0);
		}
	long long end = 0;
	for (int s = 0; s < S; ++s) end = std::max(end, total[s]);
	hip(hipSetDevice(device));
	const size_t imageBytes = end ? size_t((S - 1)*imageSS + (Cn - 1)*imageCS + end)*sizeof(float) : 0;
	Buffer<unsigned char, false> dImage;
	Buffer<int, false> dCounts;
	dImage.allocate(imageBytes + 32, "stream meter");
	dCounts.allocate((size_t)2*calls*S, "stream meter");
	unsigned char *i0 = dImage + reinterpret_cast<uintptr_t>(image)%16; // (as far behind a 16-byte boundary as the caller's image)
	if (imageBytes) hip(hipMemcpy(i0, image, imageBytes, hipMemcpyHostToDevice));
	hip(hipMemcpy(dCounts, counts, (size_t)calls*S*sizeof(int), hipMemcpyHostToDevice));
	hip(hipMemcpy(dCounts + (size_t)calls*S, starts.data(), (size_t)calls*S*sizeof(int), hipMemcpyHostToDevice));
	long long allocs = 0;
	for (int s = 0; s < S; ++s) state.setStreamMeter(device, nullptr, s, (!flags || flags[s]) ? 1 : 0, sampleRates[s], maxSubBlocks, allocs);
	int reading = 0;
	for (int k = 0; k < calls; ++k) {
		state.ensureStreamMeterScan(device, state.mostStreamMetered(counts + (size_t)k*S), form, allocs);
		state.meterStream(nullptr, reinterpret_cast<const float *>(i0), imageSS, imageCS, counts + (size_t)k*S, dCounts + (size_t)k*S, dCounts + (size_t)(calls + k)*S, form);
		if (readAfter ? readAfter[k] == 0 : k + 1 < calls) continue;
		PcmOutState::MeterReading r;
		hip(hipStreamSynchronize(nullptr));
		state.readStreamMeter(nullptr, r);
		const bool last = k + 1 == calls;
		for (int s = 0; s < S; ++s) {
			const size_t at = (size_t)reading*S + s;
			const PcmOutState::StreamMeter &m = state.streamMeter[s];
			if (Z) Z[at] = r.Z[s];
			if (blocks) blocks[at] = r.counts[2*s];
			if (gated) gated[at] = r.counts[2*s + 1];
			if (momentaryMax) momentaryMax[at] = r.range[4*s];
			if (shortTermMax) shortTermMax[at] = r.range[4*s + 1];
			if (low) low[at] = r.range[4*s + 2];
			if (high) high[at] = r.range[4*s + 3];
			if (shortBlocks) shortBlocks[at] = r.rangeCounts[2*s];
			if (rangeBlocks) rangeBlocks[at] = r.rangeCounts[2*s + 1];
			if (truePeaks) std::memcpy(truePeaks + at, &r.peaks[s], sizeof(float));
			if (samplePeaks) std::memcpy(samplePeaks + at, &r.peaks[(size_t)S + s], sizeof(float));
			if (metered) metered[at] = std::min(m.frames, m.cap);
			if (!last || !m.on) continue;
			const long long Tm = std::min(m.frames, m.cap);
			const int h = m.entry.h, nSub = Tm/4 >= h ? int(Tm/h) : 0, nb = std::min(nSub ? nSub - 3 : 0, maxBlocks), ns = std::min(nSub >= 30 ? nSub - 29 : 0, maxBlocks);
			if (blockPowers && nb > 0) hip(hipMemcpy(blockPowers + (size_t)s*maxBlocks, state.readBlockPowers(s), (size_t)nb*sizeof(double), hipMemcpyDeviceToHost));
			if (shortPowers && ns > 0) hip(hipMemcpy(shortPowers + (size_t)s*maxBlocks, state.readShortPowers(s), (size_t)ns*sizeof(double), hipMemcpyDeviceToHost));
		}
		++reading;
	}
	return SMST_OK;
	SMST_CATCH
}
// the limiter's two passes alone: see include/smst.h
int smst_debug_clip_limit(int device, int streams, int channels, const int *segments, const float *image, long long imageSS, long long imageCS,
                          const float *gains, const float *ceilings, const int *flags, int lookahead, float *need, float *r, int maxFrames,
                          float *minGain, long long *limitedFrames) {
	SMST_TRY
	if (streams < 1 || channels < 1 || channels > smst::kMaxChannels || !segments || !image || imageSS < 0 || imageCS < 0 || !gains || !ceilings || !flags || maxFrames < 0)
		throw smst::Error("clip limit: bad arguments");
	if (lookahead < 1 || lookahead > smst::kLimitMaxLookahead) throw smst::Error("clip limit: the lookahead is outside 1 ... " + std::to_string(smst::kLimitMaxLookahead) + " frames");
	auto hip = [&](hipError_t err) { if (err != hipSuccess) throw smst::Error(std::string("clip limit: ") + hipGetErrorString(err), true); };
	std::vector<smst::PcmLevel> level((size_t)streams);
	int end = 0, most = 0;
	for (int s = 0; s < streams; ++s) {
		const int *g = segments + 8*s;
		if (g[0] < 0 || g[2] < 0 || g[4] < 0 || g[6] < 0) throw smst::Error("clip limit: negative segment offset or count");
		if ((long long)g[2] + g[6] > maxFrames) throw smst::Error("clip limit: a clip is longer than maxFrames");
		if (!(ceilings[s] > 0)) throw smst::Error("clip limit: a ceiling is not above 0");
		for (int k = 0; k < 2; ++k) if (g[4*k + 2] > 0 && !g[4*k + 3]) end = std::max(end, g[4*k] + g[4*k + 2]);
		level[s] = smst::PcmLevel{smst::kPcmLevelProtect, gains[s], ceilings[s], unsigned(flags[s]) & (smst::kPcmFlagTruePeak | smst::kPcmFlagLimiter)};
		if (smst::pcmLimited(level[s]) && !g[3] && !g[7]) most = std::max(most, g[2] + g[6]);
	}
	hip(hipSetDevice(device));
	const size_t imageBytes = end ? size_t((streams - 1)*imageSS + (channels - 1)*imageCS + end)*sizeof(float) : 0;
	const size_t pitch = size_t(std::max(maxFrames, 1) + 3)/4*4, rows = (size_t)streams*pitch;
	Buffer<unsigned char, false> dImage, dSegs, dLevel;
	Buffer<float, false> dRows, dWin; // [2][streams][pitch]: need, r -- 1.0 where the passes write nothing
	Buffer<int, false> dMeters;       // [2][streams]
	dImage.allocate(imageBytes + 32, "clip limit");
	dSegs.allocate((size_t)2*streams*sizeof(smst::ClipSeg), "clip limit");
	dLevel.allocate(level.size()*sizeof(smst::PcmLevel), "clip limit");
	dRows.allocate(2*rows, "clip limit");
	dWin.allocate((size_t)2*lookahead + 1, "clip limit");
	dMeters.allocate((size_t)2*streams, "clip limit");
	unsigned char *i0 = dImage + reinterpret_cast<uintptr_t>(image)%16; // (as far behind a 16-byte boundary as the caller's image)
	if (imageBytes) hip(hipMemcpy(i0, image, imageBytes, hipMemcpyHostToDevice));
	hip(hipMemcpy(dSegs, segments, (size_t)2*streams*sizeof(smst::ClipSeg), hipMemcpyHostToDevice));
	hip(hipMemcpy(dLevel, level.data(), level.size()*sizeof(smst::PcmLevel), hipMemcpyHostToDevice));
	std::vector<float> ones(2*rows, 1.0f), win((size_t)2*lookahead + 1);
	smst::limitWindow(lookahead, win.data());
	hip(hipMemcpy(dRows, ones.data(), ones.size()*sizeof(float), hipMemcpyHostToDevice));
	hip(hipMemcpy(dWin, win.data(), win.size()*sizeof(float), hipMemcpyHostToDevice));
	hip(hipMemset(dMeters, 0, (size_t)2*streams*sizeof(int)));
	smst::PcmLevelIo io;
	io.table = reinterpret_cast<const smst::PcmLevel *>(dLevel.p);
	smst::launchClipLimit(reinterpret_cast<const float *>(i0), imageSS, imageCS, reinterpret_cast<const smst::ClipSeg *>(dSegs.p), streams, channels, most, io, lookahead, dWin,
	                      dRows, dRows + rows, (long long)pitch, dMeters, nullptr);
	hip(hipGetLastError());
	hip(hipStreamSynchronize(nullptr));
	hip(hipMemcpy(ones.data(), dRows, ones.size()*sizeof(float), hipMemcpyDeviceToHost));
	std::vector<int> words((size_t)2*streams);
	hip(hipMemcpy(words.data(), dMeters, words.size()*sizeof(int), hipMemcpyDeviceToHost));
	for (int s = 0; s < streams; ++s) {
		if (need) std::copy(ones.begin() + (size_t)s*pitch, ones.begin() + (size_t)s*pitch + maxFrames, need + (size_t)s*maxFrames);
		if (r) std::copy(ones.begin() + rows + (size_t)s*pitch, ones.begin() + rows + (size_t)s*pitch + maxFrames, r + (size_t)s*maxFrames);
		const int bits = 0x3f800000 - words[s];
		if (minGain) std::memcpy(minGain + s, &bits, sizeof(float));
		if (limitedFrames) limitedFrames[s] = words[(size_t)streams + s];
	}
	return SMST_OK;
	SMST_CATCH
}
int smst_debug_limiter_window(int lookahead, float *out) {
	if (!out) return fail("limiter window: null pointer");
	if (lookahead < 1 || lookahead > smst::kLimitMaxLookahead) return fail("limiter window: the lookahead is outside 1 ... 1024 frames");
	smst::limitWindow(lookahead, out);
	return SMST_OK;
}
// the stream limiter's output conversions, call after call with the carried lines: see include/smst.h
int smst_debug_pcm_stream_limit(int device, int streams, int channels, int calls, const int *counts, const float *image, long long imageSS, long long imageCS,
                                const float *gains, const float *ceilings, const int *flags, int lookahead, float *r, float *frames, int maxFrames,
                                float *minGain, long long *limitedFrames) {
	SMST_TRY
	if (streams < 1 || channels < 1 || channels > smst::kMaxChannels || calls < 0 || (calls && !counts) || !image || imageSS < 0 || imageCS < 0 || !gains || !ceilings || !flags || maxFrames < 0)
		throw smst::Error("stream limit: bad arguments");
	if (lookahead < 1 || lookahead > smst::kLimitMaxLookahead) throw smst::Error("stream limit: the lookahead is outside 1 ... " + std::to_string(smst::kLimitMaxLookahead) + " frames");
	auto hip = [&](hipError_t err) { if (err != hipSuccess) throw smst::Error(std::string("stream limit: ") + hipGetErrorString(err), true); };
	const int S = streams, Cn = channels, H = lookahead;
	int longest = 0;
	for (int s = 0; s < S; ++s) {
		long long total = 0;
		for (int k = 0; k < calls; ++k) { const int n = std::max(counts[(size_t)k*S + s], 0); total += n; longest = std::max(longest, n); }
		if (total > maxFrames) throw smst::Error("stream limit: a stream's calls add up to more than maxFrames");
		if (!(ceilings[s] > 0)) throw smst::Error("stream limit: a ceiling is NaN or not above 0");
		if (!std::isfinite(gains[s])) throw smst::Error("stream limit: a gain is not finite");
	}
	hip(hipSetDevice(device));
	const size_t len = size_t(std::max(longest, 1)), pitch = (len + 3)/4*4, set = smst::pcmStreamLimitSetFloats(S, Cn, H), setTruePeak = smst::pcmStreamLimitTruePeakSetFloats(S, Cn, H);
	bool anyTruePeak = false;
	for (int s = 0; s < S; ++s) anyTruePeak = anyTruePeak || (flags[s] & 3) == 3;
	const smst::PcmTableLayout at(S);
	const smst::PcmMeters meters(S);
	Buffer<unsigned char, false> dTable;
	Buffer<float, false> dImage, dOut, dLines, dTruePeakLines, dRows, dWin;
	Buffer<int, false> dWords, dLimitMeters;
	dTable.allocate(at.bytes(), "stream limit");
	dImage.allocate((size_t)S*Cn*len, "stream limit");
	dOut.allocate((size_t)S*len*Cn, "stream limit");
	dLines.allocate(2*set, "stream limit");
	if (anyTruePeak) dTruePeakLines.allocate(2*setTruePeak, "stream limit");
	dRows.allocate((size_t)S*(4*H + 2*pitch), "stream limit");
	dWin.allocate((size_t)2*H + 1, "stream limit");
	dWords.allocate(meters.words(), "stream limit");
	dLimitMeters.allocate((size_t)2*S, "stream limit");
	std::vector<float> win((size_t)2*H + 1), hImage((size_t)S*Cn*len), hOut((size_t)S*len*Cn), hR((size_t)S*pitch);
	std::vector<int> words(meters.words());
	std::vector<unsigned char> table(at.bytes());
	smst::limitWindow(H, win.data());
	meters.start(words.data());
	hip(hipMemcpy(dWin, win.data(), win.size()*sizeof(float), hipMemcpyHostToDevice));
	hip(hipMemcpy(dWords, words.data(), meters.bytes(), hipMemcpyHostToDevice));
	hip(hipMemset(dLimitMeters, 0, (size_t)2*S*sizeof(int)));
	smst::PcmStreamLimit lim;
	for (int k = 0; k < 2; ++k) { lim.need[k] = dLines + k*set; lim.frames[k] = dLines + k*set + (size_t)S*4*H; }
	if (anyTruePeak) for (int k = 0; k < 2; ++k) lim.truePeakFrames[k] = dTruePeakLines + k*setTruePeak;
	lim.meters = dLimitMeters;
	lim.needRow = dRows; lim.needPitch = (long long)(4*H + pitch);
	lim.rRow = dRows + (size_t)S*(4*H + pitch); lim.rPitch = (long long)pitch;
	lim.window = dWin; lim.H = H;
	smst::launchPcmLimitClear(lim, S, Cn, -1, nullptr);
	if (r) std::fill(r, r + (size_t)S*maxFrames, 1.0f);
	if (frames) std::fill(frames, frames + (size_t)S*maxFrames*Cn, 0.0f);
	std::vector<long long> done((size_t)S, 0);
	std::vector<unsigned char> whichSet((size_t)S, 0);
	const smst::PcmLevelIo io = meters.io(at.level(dTable.p), dWords);
	for (int k = 0; k < calls; ++k) {
		int most = 0, mostLimited = 0, mostPlain = 0, mostTruePeak = 0;
		for (int s = 0; s < S; ++s) {
			const int n = std::max(counts[(size_t)k*S + s], 0);
			const bool on = (flags[s] & 1) != 0, late = on && (flags[s] & 2) != 0;
			at.outCounts(table.data())[s] = n;
			at.level(table.data())[s] = smst::PcmLevel{smst::kPcmLevelFixed, gains[s], on ? ceilings[s] : 1.0f,
			                                           on ? smst::kPcmFlagStreamLimiter | (whichSet[s] ? smst::kPcmFlagStreamLimitSet : 0u) | (late ? smst::kPcmFlagStreamLimitTruePeak : 0u) : 0u};
			most = std::max(most, n);
			if (on) mostLimited = std::max(mostLimited, n);
			if (on) (late ? mostTruePeak : mostPlain) = std::max(late ? mostTruePeak : mostPlain, n);
			for (int c = 0; c < Cn; ++c) std::copy(image + s*imageSS + c*imageCS + done[s], image + s*imageSS + c*imageCS + done[s] + n, hImage.begin() + ((size_t)s*Cn + c)*len);
		}
		if (most < 1) continue;
		hip(hipMemcpy(dImage, hImage.data(), hImage.size()*sizeof(float), hipMemcpyHostToDevice));
		hip(hipMemcpy(dTable, table.data(), table.size(), hipMemcpyHostToDevice));
		if (mostLimited > 0) smst::launchPcmOutLimited(SMST_PCM_F32, dImage, (long long)(Cn*len), (long long)len, dOut, (long long)(len*Cn), Cn, at.outCounts(dTable.p), S, Cn, most, mostPlain, mostTruePeak, nullptr, nullptr, nullptr, io, lim);
		else smst::launchPcmOut(SMST_PCM_F32, dImage, (long long)(Cn*len), (long long)len, dOut, (long long)(len*Cn), Cn, at.outCounts(dTable.p), S, Cn, most, nullptr, nullptr, nullptr, io);
		hip(hipGetLastError());
		hip(hipStreamSynchronize(nullptr));
		hip(hipMemcpy(hOut.data(), dOut, hOut.size()*sizeof(float), hipMemcpyDeviceToHost));
		if (mostLimited > 0) hip(hipMemcpy(hR.data(), lim.rRow, hR.size()*sizeof(float), hipMemcpyDeviceToHost));
		for (int s = 0; s < S; ++s) {
			const int n = at.outCounts(table.data())[s];
			const bool on = (flags[s] & 1) != 0;
			if (frames) std::copy(hOut.begin() + (size_t)s*len*Cn, hOut.begin() + ((size_t)s*len + n)*Cn, frames + ((size_t)s*maxFrames + done[s])*Cn);
			if (r && on) std::copy(hR.begin() + (size_t)s*pitch, hR.begin() + (size_t)s*pitch + n, r + (size_t)s*maxFrames + done[s]);
			if (on && n > 0) whichSet[s] ^= 1;
			done[s] += n;
		}
	}
	hip(hipStreamSynchronize(nullptr));
	std::vector<int> limitWords((size_t)2*S);
	hip(hipMemcpy(limitWords.data(), dLimitMeters, limitWords.size()*sizeof(int), hipMemcpyDeviceToHost));
	for (int s = 0; s < S; ++s) {
		const int bits = 0x3f800000 - limitWords[s];
		if (minGain) std::memcpy(minGain + s, &bits, sizeof(float));
		if (limitedFrames) limitedFrames[s] = (long long)(unsigned)limitWords[(size_t)S + s];
	}
	return SMST_OK;
	SMST_CATCH
}
int smst_debug_true_peak_taps(float *out) {
	if (!out) return fail("true peak taps: null pointer");
	std::memcpy(out, smst::truePeakTable().c, sizeof(smst::TruePeakTable));
	return SMST_OK;
}
int smst_debug_resample_taps(int up, int down, float *out, int *taps) {
	SMST_TRY
	smst::resampleReduce(up, down);
	const smst::ResampleShape g = smst::resampleShapeOf(up, down);
	if (taps) *taps = g.T;
	if (out) {
		std::vector<float> table((size_t)g.L*g.pitch);
		smst::resampleTaps(g, table.data());
		for (int p = 0; p < g.L; ++p) std::copy(table.begin() + (size_t)p*g.pitch, table.begin() + (size_t)p*g.pitch + g.T, out + (size_t)p*g.T);
	}
	return SMST_OK;
	SMST_CATCH
}
// the resample kernel alone: see include/smst.h
int smst_debug_clip_resample(int device, int streams, int channels, const int *counts, const int *ratios, const float *image, long long imageSS, long long imageCS,
                             const int *segments, float *out, long long outSS, long long outCS) {
	SMST_TRY
	if (streams < 1 || channels < 1 || channels > smst::kMaxChannels || !counts || !ratios || !image || !segments || !out || imageSS < 0 || imageCS < 0 || outSS < 0 || outCS < 0)
		throw smst::Error("clip resample: bad arguments");
	auto hip = [&](hipError_t err) { if (err != hipSuccess) throw smst::Error(std::string("clip resample: ") + hipGetErrorString(err), true); };
	hip(hipSetDevice(device));
	std::vector<smst::ResampleEntry> entries((size_t)streams, smst::ResampleEntry{nullptr, 0, 0, 0, 0, 0, 0, 0, 0});
	std::vector<Buffer<float, false>> tables((size_t)streams); // (one per resampled stream: a hook's streams do not share them)
	int endIn = 0, endOut = 0, most = 0, maxSpanPitch = 4;
	for (int s = 0; s < streams; ++s) {
		const int *g = segments + 8*s;
		int up = ratios[2*s], down = ratios[2*s + 1];
		smst::resampleReduce(up, down);
		if (counts[s] < 0) throw smst::Error("clip resample: negative sample count");
		if (up == 1 && down == 1) continue; // not resampled: its rows of `out` are left alone
		const long long nr = smst::resampledLength(counts[s], up, down);
		if (nr > 0x7fffffffLL) throw smst::Error("clip resample: the resampled clip is too long");
		if (g[1] < 0 || g[2] < 0 || g[5] < 0 || g[6] < 0 || (long long)g[2] + g[6] != nr) throw smst::Error("clip resample: the two segments' counts do not add up to the resampled length");
		const smst::ResampleShape shape = smst::resampleShapeOf(up, down);
		std::vector<float> table((size_t)shape.L*shape.pitch);
		smst::resampleTaps(shape, table.data());
		tables[s].allocate(table.size(), "clip resample");
		hip(hipMemcpy(tables[s], table.data(), table.size()*sizeof(float), hipMemcpyHostToDevice));
		entries[s] = smst::ResampleEntry{tables[s].p, counts[s], int(nr), shape.L, shape.M, shape.H, shape.T, shape.pitch, 0};
		endIn = std::max(endIn, counts[s]);
		for (int k = 0; k < 2; ++k) if (g[4*k + 2] > 0) endOut = std::max(endOut, g[4*k + 1] + g[4*k + 2]);
		most = std::max(most, int(nr));
		maxSpanPitch = std::max(maxSpanPitch, smst::resampleSpanPitch(shape.L, shape.M, shape.T));
	}
	// host pointers are staged whole: every stream's rows, as far behind a 16-byte boundary as the caller's
	const size_t imageBytes = endIn ? size_t((streams - 1)*imageSS + (channels - 1)*imageCS + endIn)*sizeof(float) : 0;
	const size_t outBytes = endOut ? size_t((streams - 1)*outSS + (channels - 1)*outCS + endOut)*sizeof(float) : 0;
	Buffer<unsigned char, false> dImage, dOut, dSegs, dEntries;
	dImage.allocate(imageBytes + 32, "clip resample");
	dOut.allocate(outBytes + 32, "clip resample");
	dSegs.allocate((size_t)2*streams*sizeof(smst::ClipSeg), "clip resample");
	dEntries.allocate(entries.size()*sizeof(smst::ResampleEntry), "clip resample");
	unsigned char *i0 = dImage + reinterpret_cast<uintptr_t>(image)%16, *o0 = dOut + reinterpret_cast<uintptr_t>(out)%16;
	if (imageBytes) hip(hipMemcpy(i0, image, imageBytes, hipMemcpyHostToDevice));
	if (outBytes) hip(hipMemcpy(o0, out, outBytes, hipMemcpyHostToDevice));
	hip(hipMemcpy(dSegs, segments, (size_t)2*streams*sizeof(smst::ClipSeg), hipMemcpyHostToDevice));
	hip(hipMemcpy(dEntries, entries.data(), entries.size()*sizeof(smst::ResampleEntry), hipMemcpyHostToDevice));
	smst::launchClipResample(reinterpret_cast<const float *>(i0), imageSS, imageCS, reinterpret_cast<float *>(o0), outSS, outCS, reinterpret_cast<const smst::ClipSeg *>(dSegs.p),
	                         reinterpret_cast<const smst::ResampleEntry *>(dEntries.p), streams, channels, most, maxSpanPitch, nullptr);
	hip(hipGetLastError());
	hip(hipStreamSynchronize(nullptr));
	if (outBytes) hip(hipMemcpy(out, o0, outBytes, hipMemcpyDeviceToHost));
	return SMST_OK;
	SMST_CATCH
}
// the output-resample kernel alone: see include/smst.h
int smst_debug_clip_resample_out(int device, int streams, int channels, const int *counts, const int *ratios, const float *image, long long imageSS, long long imageCS,
                                 const int *srcSegments, const int *dstSegments, float *out, long long outSS, long long outCS) {
	SMST_TRY
	if (streams < 1 || channels < 1 || channels > smst::kMaxChannels || !counts || !ratios || !image || !srcSegments || !dstSegments || !out || imageSS < 0 || imageCS < 0 || outSS < 0 || outCS < 0)
		throw smst::Error("clip resample out: bad arguments");
	auto hip = [&](hipError_t err) { if (err != hipSuccess) throw smst::Error(std::string("clip resample out: ") + hipGetErrorString(err), true); };
	hip(hipSetDevice(device));
	std::vector<smst::ResampleOutEntry> entries((size_t)streams, smst::ResampleOutEntry{nullptr, 0, 0, 0, 0, 0, 0, 0, 0});
	std::vector<Buffer<float, false>> tables((size_t)streams); // (one per resampled stream: a hook's streams do not share them)
	int endIn = 0, endOut = 0, most = 0, maxSpanPitch = 4;
	for (int s = 0; s < streams; ++s) {
		const int *r = srcSegments + 8*s, *g = dstSegments + 8*s;
		int up = ratios[2*s], down = ratios[2*s + 1];
		smst::resampleReduce(up, down);
		if (counts[s] < 0) throw smst::Error("clip resample out: negative sample count");
		if (up == 1 && down == 1) continue; // not resampled: its rows of `out` are left alone
		const long long E = smst::resampleRenderLength(counts[s], up, down);
		if (E > 0x7fffffffLL) throw smst::Error("clip resample out: the rendered clip is too long");
		if (r[0] < 0 || r[2] < 0 || r[4] < 0 || r[6] < 0 || (long long)r[2] + r[6] != E) throw smst::Error("clip resample out: the two source segments' counts do not add up to the rendered length");
		if (g[1] < 0 || g[2] < 0 || g[5] < 0 || g[6] < 0 || (long long)g[2] + g[6] != counts[s]) throw smst::Error("clip resample out: the two destination segments' counts do not add up to the delivered length");
		const smst::ResampleShape shape = smst::resampleShapeOf(up, down);
		std::vector<float> table((size_t)shape.L*shape.pitch);
		smst::resampleTaps(shape, table.data());
		tables[s].allocate(table.size(), "clip resample out");
		hip(hipMemcpy(tables[s], table.data(), table.size()*sizeof(float), hipMemcpyHostToDevice));
		entries[s] = smst::ResampleOutEntry{tables[s].p, int(E), counts[s], shape.L, shape.M, shape.H, shape.T, shape.pitch, 0};
		for (int k = 0; k < 2; ++k) if (r[4*k + 2] > 0) endIn = std::max(endIn, r[4*k] + r[4*k + 2]);
		for (int k = 0; k < 2; ++k) if (g[4*k + 2] > 0) endOut = std::max(endOut, g[4*k + 1] + g[4*k + 2]);
		most = std::max(most, counts[s]);
		maxSpanPitch = std::max(maxSpanPitch, smst::resampleSpanPitch(shape.L, shape.M, shape.T));
	}
	// host pointers are staged whole: every stream's rows, as far behind a 16-byte boundary as the caller's
	const size_t imageBytes = endIn ? size_t((streams - 1)*imageSS + (channels - 1)*imageCS + endIn)*sizeof(float) : 0;
	const size_t outBytes = endOut ? size_t((streams - 1)*outSS + (channels - 1)*outCS + endOut)*sizeof(float) : 0;
	Buffer<unsigned char, false> dImage, dOut, dSrc, dDst, dEntries;
	dImage.allocate(imageBytes + 32, "clip resample out");
	dOut.allocate(outBytes + 32, "clip resample out");
	dSrc.allocate((size_t)2*streams*sizeof(smst::ClipSeg), "clip resample out");
	dDst.allocate((size_t)2*streams*sizeof(smst::ClipSeg), "clip resample out");
	dEntries.allocate(entries.size()*sizeof(smst::ResampleOutEntry), "clip resample out");
	unsigned char *i0 = dImage + reinterpret_cast<uintptr_t>(image)%16, *o0 = dOut + reinterpret_cast<uintptr_t>(out)%16;
	if (imageBytes) hip(hipMemcpy(i0, image, imageBytes, hipMemcpyHostToDevice));
	if (outBytes) hip(hipMemcpy(o0, out, outBytes, hipMemcpyHostToDevice));
	hip(hipMemcpy(dSrc, srcSegments, (size_t)2*streams*sizeof(smst::ClipSeg), hipMemcpyHostToDevice));
	hip(hipMemcpy(dDst, dstSegments, (size_t)2*streams*sizeof(smst::ClipSeg), hipMemcpyHostToDevice));
	hip(hipMemcpy(dEntries, entries.data(), entries.size()*sizeof(smst::ResampleOutEntry), hipMemcpyHostToDevice));
	smst::launchClipResampleOut(reinterpret_cast<const float *>(i0), imageSS, imageCS, reinterpret_cast<float *>(o0), outSS, outCS, reinterpret_cast<const smst::ClipSeg *>(dSrc.p),
	                            reinterpret_cast<const smst::ClipSeg *>(dDst.p), reinterpret_cast<const smst::ResampleOutEntry *>(dEntries.p), streams, channels, most, maxSpanPitch, nullptr);
	hip(hipGetLastError());
	hip(hipStreamSynchronize(nullptr));
	if (outBytes) hip(hipMemcpy(out, o0, outBytes, hipMemcpyDeviceToHost));
	return SMST_OK;
	SMST_CATCH
}
// the stream-resample kernel alone, call after call: see include/smst.h
int smst_debug_pcm_stream_resample(int device, int streams, int channels, int calls, const int *counts, const int *ratios, const long long *fed0,
                                   const float *image, long long imageSS, long long imageCS, float *out, long long outSS, long long outCS, int maxFrames, long long *made) {
	SMST_TRY
	if (streams < 1 || channels < 1 || channels > smst::kMaxChannels || calls < 0 || (calls > 0 && !counts) || !ratios || !image || !out || maxFrames < 0 || imageSS < 0 || imageCS < 0 || outSS < 0 || outCS < 0)
		throw smst::Error("stream resample: bad arguments");
	auto hip = [&](hipError_t err) { if (err != hipSuccess) throw smst::Error(std::string("stream resample: ") + hipGetErrorString(err), true); };
	hip(hipSetDevice(device));
	struct Stream { smst::ResampleShape g{0, 0, 0, 0, 0}; long long fed = 0, made = 0, at = 0, written = 0; int set = 0, fresh = 1; };
	std::vector<Stream> st((size_t)streams);
	std::vector<Buffer<float, false>> tables((size_t)streams); // (one per resampled stream: a hook's streams do not share them)
	long long endIn = 0;
	for (int s = 0; s < streams; ++s) {
		int up = ratios[2*s], down = ratios[2*s + 1];
		smst::resampleReduce(up, down);
		long long total = 0;
		for (int k = 0; k < calls; ++k) total += std::max(counts[(size_t)k*streams + s], 0);
		if (total > 0x7fffffffLL) throw smst::Error("stream resample: a stream's counts add up to more than 2147483647");
		if (up == 1 && down == 1) continue; // no setting: its rows of `out` are left alone
		endIn = std::max(endIn, total);
		st[s].g = smst::resampleShapeOf(up, down);
		if (fed0) {
			if (fed0[s] < 0 || fed0[s] > (1LL << 48)) throw smst::Error("stream resample: a starting position is negative or above 2^48");
			st[s].fed = fed0[s];
			st[s].made = smst::streamResampleDue(fed0[s] - st[s].g.H, up, down);
		}
		std::vector<float> table((size_t)st[s].g.L*st[s].g.pitch);
		smst::resampleTaps(st[s].g, table.data());
		tables[s].allocate(table.size(), "stream resample");
		hip(hipMemcpy(tables[s], table.data(), table.size()*sizeof(float), hipMemcpyHostToDevice));
	}
	// host pointers are staged whole: every stream's rows, as far behind a 16-byte boundary as the caller's
	const size_t imageBytes = endIn ? size_t((streams - 1)*imageSS + (channels - 1)*imageCS + endIn)*sizeof(float) : 0;
	const size_t outBytes = maxFrames ? size_t((streams - 1)*outSS + (channels - 1)*outCS + maxFrames)*sizeof(float) : 0;
	const size_t lineSet = (size_t)streams*channels*smst::kStreamResampleLine;
	Buffer<unsigned char, false> dImage, dOut, dEntries;
	Buffer<float, false> dLines;
	dImage.allocate(imageBytes + 32, "stream resample");
	dOut.allocate(outBytes + 32, "stream resample");
	dEntries.allocate((size_t)streams*sizeof(smst::StreamResampleEntry), "stream resample");
	dLines.allocate(2*lineSet, "stream resample");
	unsigned char *i0 = dImage + reinterpret_cast<uintptr_t>(image)%16, *o0 = dOut + reinterpret_cast<uintptr_t>(out)%16;
	if (imageBytes) hip(hipMemcpy(i0, image, imageBytes, hipMemcpyHostToDevice));
	if (outBytes) hip(hipMemcpy(o0, out, outBytes, hipMemcpyHostToDevice));
	hip(hipMemset(dLines, 0, 2*lineSet*sizeof(float)));
	std::vector<smst::StreamResampleEntry> entries((size_t)streams);
	for (int call = 0; call < calls; ++call) {
		int mostK = 0, mostN = 0;
		for (int s = 0; s < streams; ++s) {
			const int n = counts[(size_t)call*streams + s];
			entries[s] = smst::StreamResampleEntry{nullptr, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
			Stream &t = st[s];
			if (t.g.L < 1 || n < 1) continue; // no setting, no part, or no frame: the line stays
			const long long k = smst::streamResampleDue(t.fed + n - t.g.H, t.g.L, t.g.M) - t.made;
			if (t.written + k > maxFrames) throw smst::Error("stream resample: maxFrames is smaller than the frames a stream makes");
			entries[s] = smst::StreamResampleEntry{tables[s].p, t.fed, t.made, t.at, t.written, n, int(k), t.g.L, t.g.M, t.g.H, t.g.T, t.g.pitch, t.set, t.fresh, 0};
			t.fed += n; t.made += k; t.at += n; t.written += k; t.set ^= 1; t.fresh = 0;
			mostK = std::max(mostK, int(k)); mostN = std::max(mostN, n);
		}
		if (mostN < 1) continue;
		int maxSpanPitch = 4;
		for (int s = 0; s < streams; ++s) if (entries[s].L > 0) maxSpanPitch = std::max(maxSpanPitch, smst::resampleSpanPitchOf(entries[s].L, entries[s].M, entries[s].T, smst::streamResampleTileFrames(mostK)));
		hip(hipMemcpy(dEntries, entries.data(), entries.size()*sizeof(smst::StreamResampleEntry), hipMemcpyHostToDevice));
		smst::launchPcmStreamResample(reinterpret_cast<const float *>(i0), imageSS, imageCS, reinterpret_cast<float *>(o0), outSS, outCS, dLines, (long long)lineSet,
		                              reinterpret_cast<const smst::StreamResampleEntry *>(dEntries.p), streams, channels, mostK, maxSpanPitch, nullptr);
		hip(hipGetLastError());
		hip(hipStreamSynchronize(nullptr));
	}
	if (outBytes) hip(hipMemcpy(out, o0, outBytes, hipMemcpyDeviceToHost));
	if (made) for (int s = 0; s < streams; ++s) made[s] = st[s].written;
	return SMST_OK;
	SMST_CATCH
}
// the stream-output-resample kernel alone, call after call: see include/smst.h
int smst_debug_pcm_stream_resample_out(int device, int streams, int channels, int calls, const int *counts, const int *ratios, const long long *delivered0,
                                       const float *image, long long imageSS, long long imageCS, float *out, long long outSS, long long outCS, int maxFrames, long long *rendered) {
	SMST_TRY
	if (streams < 1 || channels < 1 || channels > smst::kMaxChannels || calls < 0 || (calls > 0 && !counts) || !ratios || !image || !out || maxFrames < 0 || imageSS < 0 || imageCS < 0 || outSS < 0 || outCS < 0)
		throw smst::Error("stream out resample: bad arguments");
	auto hip = [&](hipError_t err) { if (err != hipSuccess) throw smst::Error(std::string("stream out resample: ") + hipGetErrorString(err), true); };
	hip(hipSetDevice(device));
	struct Stream { smst::ResampleShape g{0, 0, 0, 0, 0}; long long delivered = 0, at = 0, written = 0, endIn = 0; int Dl = 0, set = 0, fresh = 1; };
	std::vector<Stream> st((size_t)streams);
	std::vector<Buffer<float, false>> tables((size_t)streams); // (one per resampled stream: a hook's streams do not share them)
	long long endIn = 0;
	for (int s = 0; s < streams; ++s) {
		int up = ratios[2*s], down = ratios[2*s + 1];
		smst::resampleReduce(up, down);
		if (up == 1 && down == 1) continue; // no setting: its rows of `out` are left alone
		Stream &t = st[s];
		t.g = smst::resampleShapeOf(up, down);
		t.Dl = smst::streamResampleOutLatency(up, down, t.g.H);
		if (delivered0) {
			if (delivered0[s] < 0 || delivered0[s] > (1LL << 48)) throw smst::Error("stream out resample: a starting position is negative or above 2^48");
			t.delivered = delivered0[s];
		}
		long long total = 0;
		for (int k = 0; k < calls; ++k) total += std::max(counts[(size_t)k*streams + s], 0);
		if (total > maxFrames) throw smst::Error("stream out resample: maxFrames is smaller than the frames a stream is delivered");
		t.endIn = smst::streamResampleOutDue(t.delivered + total, up, down) - smst::streamResampleOutDue(t.delivered, up, down); // the rendered frames the calls consume
		if (t.endIn > 0x7fffffffLL) throw smst::Error("stream out resample: a stream's rendered frames add up to more than 2147483647");
		endIn = std::max(endIn, t.endIn);
		std::vector<float> table((size_t)t.g.L*t.g.pitch);
		smst::resampleTaps(t.g, table.data());
		tables[s].allocate(table.size(), "stream out resample");
		hip(hipMemcpy(tables[s], table.data(), table.size()*sizeof(float), hipMemcpyHostToDevice));
	}
	// host pointers are staged whole: every stream's rows, as far behind a 16-byte boundary as the caller's
	const size_t imageBytes = endIn ? size_t((streams - 1)*imageSS + (channels - 1)*imageCS + endIn)*sizeof(float) : 0;
	const size_t outBytes = maxFrames ? size_t((streams - 1)*outSS + (channels - 1)*outCS + maxFrames)*sizeof(float) : 0;
	const size_t lineSet = (size_t)streams*channels*smst::kStreamResampleOutLine;
	Buffer<unsigned char, false> dImage, dOut, dEntries;
	Buffer<float, false> dLines;
	dImage.allocate(imageBytes + 32, "stream out resample");
	dOut.allocate(outBytes + 32, "stream out resample");
	dEntries.allocate((size_t)streams*sizeof(smst::StreamResampleOutEntry), "stream out resample");
	dLines.allocate(2*lineSet, "stream out resample");
	unsigned char *i0 = dImage + reinterpret_cast<uintptr_t>(image)%16, *o0 = dOut + reinterpret_cast<uintptr_t>(out)%16;
	if (imageBytes) hip(hipMemcpy(i0, image, imageBytes, hipMemcpyHostToDevice));
	if (outBytes) hip(hipMemcpy(o0, out, outBytes, hipMemcpyHostToDevice));
	hip(hipMemset(dLines, 0, 2*lineSet*sizeof(float)));
	std::vector<smst::StreamResampleOutEntry> entries((size_t)streams);
	for (int call = 0; call < calls; ++call) {
		int mostNd = 0;
		for (int s = 0; s < streams; ++s) {
			const int n = counts[(size_t)call*streams + s];
			entries[s] = smst::StreamResampleOutEntry{nullptr, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
			Stream &t = st[s];
			if (t.g.L < 1 || n < 1) continue; // no setting, no part, or no frame: the line stays
			const long long from = smst::streamResampleOutDue(t.delivered, t.g.L, t.g.M), E = smst::streamResampleOutDue(t.delivered + n, t.g.L, t.g.M) - from;
			entries[s] = smst::StreamResampleOutEntry{tables[s].p, t.delivered, from, t.at, t.written, n, int(E), t.Dl, t.g.L, t.g.M, t.g.H, t.g.T, t.g.pitch, t.set, t.fresh};
			t.delivered += n; t.at += E; t.written += n; t.set ^= 1; t.fresh = 0;
			mostNd = std::max(mostNd, n);
		}
		if (mostNd < 1) continue;
		int maxSpanPitch = 4;
		for (int s = 0; s < streams; ++s) if (entries[s].L > 0) maxSpanPitch = std::max(maxSpanPitch, smst::resampleSpanPitchOf(entries[s].L, entries[s].M, entries[s].T, smst::streamResampleTileFrames(mostNd)));
		hip(hipMemcpy(dEntries, entries.data(), entries.size()*sizeof(smst::StreamResampleOutEntry), hipMemcpyHostToDevice));
		smst::launchPcmStreamResampleOut(reinterpret_cast<const float *>(i0), imageSS, imageCS, reinterpret_cast<float *>(o0), outSS, outCS, dLines, (long long)lineSet,
		                                 reinterpret_cast<const smst::StreamResampleOutEntry *>(dEntries.p), streams, channels, mostNd, maxSpanPitch, nullptr);
		hip(hipGetLastError());
		hip(hipStreamSynchronize(nullptr));
	}
	if (outBytes) hip(hipMemcpy(out, o0, outBytes, hipMemcpyDeviceToHost));
	if (rendered) for (int s = 0; s < streams; ++s) rendered[s] = st[s].at;
	return SMST_OK;
	SMST_CATCH
}
int smst_batch_take_pcm_overs(smst_batch *b, long long *clamped, long long *nans) {
	BATCH_CALL({
		b->engine->synchronize();
		hipSetDevice(b->engine->device());
		b->pcmOut.takeOvers(clamped, nans);
	})
}
int smst_batch_take_pcm_peaks(smst_batch *b, float *peaks, float *gains) {
	BATCH_CALL({
		b->engine->synchronize();
		hipSetDevice(b->engine->device());
		b->pcmOut.takePeaks(peaks, gains);
	})
}

// ---------------------------------------------------------------------------------------------------------
// single-stream handle API (web/emscripten/main.cpp:15-77 with a handle instead of the global singleton)
// ---------------------------------------------------------------------------------------------------------
static std::string g_defaultDeviceError; // set once by smst_default_device() when SMST_DEVICE names no device of this process
int smst_create(smst_stretch **out, long seed, int device) {
	if (!out) return fail("null output pointer");
	SMST_TRY
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) throw smst::Error("hipGetDeviceCount: no HIP device available (the gfx950 path has no CPU fallback)", true);
	// (the SMST_DEVICE message only for the sentinel smst_default_device() returns when the variable named no device: an explicit ordinal
	// that is out of range has nothing to do with the default device)
	if (device == -1 && !g_defaultDeviceError.empty()) throw smst::Error(g_defaultDeviceError);
	if (device < 0 || device >= n) throw smst::Error("device ordinal " + std::to_string(device) + " out of range: this process sees " + std::to_string(n) + " device(s)");
	smst_stretch *h = new smst_stretch();
	h->seed = seed;
	h->device = device;
	*out = h;
	return SMST_OK;
	SMST_CATCH
}

// the device new single-stream handles are created on: SMST_DEVICE (validated against the device count, once) or the setter
static std::atomic<int> g_defaultDevice{-1};
// SMST_DEVICE that is no ordinal this process can see is an ERROR (one rank per GPU: a wrong ordinal or a mismatch with HIP_VISIBLE_DEVICES
// would put every rank on GPU 0 without a word): smst_default_device() reports it on stderr once and returns -1, and smst_create() on the
// default device fails with SMST_ERR_INVALID naming the value and the device count.
int smst_default_device(void) {
	int v = g_defaultDevice.load(std::memory_order_acquire);
	if (v == -1) {
		v = 0;
		if (const char *env = std::getenv("SMST_DEVICE")) {
			char *end = nullptr;
			const long asked = std::strtol(env, &end, 10);
			const int n = smst_device_count();
			if (end != env && *end == '\0' && asked >= 0 && (n <= 0 || asked < n)) {
				v = int(asked);
			} else {
				static std::once_flag once;
				std::call_once(once, [&] {
					g_defaultDeviceError = std::string("SMST_DEVICE=\"") + env + "\" is not a device ordinal of this process (" + std::to_string(n) + " device(s) visible)";
					std::fprintf(stderr, "libsmst_hip: %s\n", g_defaultDeviceError.c_str());
				});
				v = -2; // latched: invalid
			}
		}
		int expected = -1;
		if (!g_defaultDevice.compare_exchange_strong(expected, v, std::memory_order_acq_rel)) v = expected; // another thread (or the setter) was first
	}
	if (v == -2) { fail(g_defaultDeviceError.c_str()); return -1; }
	return v;
}
int smst_set_default_device(int device) {
	if (device < 0 || device >= smst_device_count()) return fail("device ordinal out of range");
	g_defaultDevice.store(device, std::memory_order_release);
	return SMST_OK;
}
// ---------------------------------------------------------------------------------------------------------
// pool (extension): the machinery.  The single-stream calls below go through engineOf() / slotOf(): an unattached handle's own
// one-stream engine and stream 0 -- what they always used -- or the member's slot of its group's engine.
// ---------------------------------------------------------------------------------------------------------
static Batch *engineOf(const smst_stretch *h) {
	if (!h) return nullptr;
	if (h->group) return h->group->batch->engine.get();
	return h->batch ? h->batch->engine.get() : nullptr;
}
static int slotOf(const smst_stretch *h) { return h->group ? h->slot : 0; }

static const int kPoolFirstSlots = 4;

static void sizeGroupScratch(PoolGroup &g) {
	const size_t S = size_t(g.batch->engine->streams());
	g.slots.resize(S, nullptr);
	g.nIn.assign(S, 0);
	g.nOut.assign(S, 0);
	g.active.assign(S, 0);
}
static std::unique_ptr<smst_batch> newGroupBatch(int streams, const Batch &like, int device) {
	std::unique_ptr<smst_batch> b(new smst_batch());
	b->engine.reset(new Batch(streams, like.channels(), like.blockSamples(), like.intervalSamples(), like.splitComputation(), device, 0));
	return b;
}
static void retireCounts(smst_pool *p, const smst_batch &b) { p->allocEvents += (long long)b.engine->allocationEvents() + b.stagingAllocs; }

// all members of the group into an engine of twice the slots, each into the slot it had: ONE launch moves them all (kMoveStreams)
static void growGroup(smst_pool *p, PoolGroup &g) {
	Batch &old = *g.batch->engine;
	const int S = old.streams();
	std::unique_ptr<smst_batch> b = newGroupBatch(2*S, old, p->device);
	std::vector<int> rows;
	for (int s = 0; s < S; ++s) if (g.slots[s]) rows.push_back(s);
	b->engine->moveStreamsFrom(old, rows.data(), rows.data(), int(rows.size()));
	retireCounts(p, *g.batch);
	++p->allocEvents;
	g.batch = std::move(b);
	sizeGroupScratch(g);
	for (int s = 2*S - 1; s >= S; --s) g.freeSlots.push_back(s);
	std::sort(g.freeSlots.begin(), g.freeSlots.end(), [](int a, int b2) { return a > b2; });
}

// a configured member (it owns a one-stream engine) into a slot of its geometry's group; the engine of its own goes
static void joinGroup(smst_pool *p, smst_stretch *h) {
	Batch &own = *h->batch->engine;
	PoolGroup *g = nullptr;
	for (auto &c : p->groups) {
		const Batch &e = *c->batch->engine;
		if (e.channels() == own.channels() && e.blockSamples() == own.blockSamples() && e.intervalSamples() == own.intervalSamples() && e.splitComputation() == own.splitComputation()) { g = c.get(); break; }
	}
	if (!g) {
		std::unique_ptr<PoolGroup> fresh(new PoolGroup());
		fresh->batch = newGroupBatch(kPoolFirstSlots, own, p->device);
		sizeGroupScratch(*fresh);
		for (int s = kPoolFirstSlots - 1; s >= 0; --s) fresh->freeSlots.push_back(s);
		++p->allocEvents;
		p->groups.push_back(std::move(fresh));
		g = p->groups.back().get();
	}
	if (g->freeSlots.empty()) growGroup(p, *g);
	const int slot = g->freeSlots.back();
	g->batch->engine->moveStreamFrom(own, 0, slot);
	g->freeSlots.pop_back();
	g->slots[slot] = h;
	++g->used;
	h->group = g;
	h->slot = slot;
	retireCounts(p, *h->batch);
	++p->allocEvents;
	h->batch.reset();
}
static void dropGroupIfEmpty(smst_pool *p, PoolGroup *g) {
	if (g->used > 0) return;
	for (size_t i = 0; i < p->groups.size(); ++i)
		if (p->groups[i].get() == g) { retireCounts(p, *g->batch); p->groups.erase(p->groups.begin() + long(i)); return; }
}
static void freeSlot(smst_stretch *h) {
	PoolGroup *g = h->group;
	g->slots[h->slot] = nullptr;
	g->freeSlots.push_back(h->slot);
	std::sort(g->freeSlots.begin(), g->freeSlots.end(), [](int a, int b) { return a > b; });
	--g->used;
	h->group = nullptr;
	h->slot = -1;
	dropGroupIfEmpty(h->pool, g);
}
// ... and back: a one-stream engine of its own with the slot's state (the handle stays registered with the pool)
static void leaveGroup(smst_stretch *h) {
	Batch &e = *h->group->batch->engine;
	std::unique_ptr<smst_batch> b(new smst_batch());
	b->engine.reset(new Batch(1, e.channels(), e.blockSamples(), e.intervalSamples(), e.splitComputation(), h->device, h->seed));
	b->engine->moveStreamFrom(e, h->slot, 0);
	++h->pool->allocEvents;
	h->batch = std::move(b);
	freeSlot(h);
}

// ONE engine call for the group's pending requests (only != null: that member's alone -- the synchronous smst_process of a member; its
// planes then are the whole staging image and every stream stride is 0).  Returns whether the engine was called; failures are thrown
// after every affected member has its status.
static bool runGroup(smst_pool *p, PoolGroup &g, smst_stretch *only) {
	smst_batch *b = g.batch.get();
	Batch &e = *b->engine;
	const int S = e.streams(), C = e.channels();
	int maxIn = 0, maxOut = 0, n = 0;
	bool all = true;
	for (int s = 0; s < S; ++s) {
		smst_stretch *m = g.slots[s];
		const bool on = m && m->pending && (!only || m == only);
		g.active[s] = on ? 1 : 0;
		g.nIn[s] = on ? m->reqIn_n : 0;
		g.nOut[s] = on ? m->reqOut_n : 0;
		if (!on) { all = false; continue; }
		++n;
		maxIn = std::max(maxIn, g.nIn[s]);
		maxOut = std::max(maxOut, g.nOut[s]);
	}
	if (!n) return false;
	maxIn = std::max(maxIn, 1);
	maxOut = std::max(maxOut, 1);
	const size_t rows = only ? size_t(C) : size_t(S)*C;
	auto row = [&](int s, int c) { return only ? size_t(c) : size_t(s)*C + c; };
	try {
		hipSetDevice(e.device());
		// gather -> one copy to the device
		g.hIn.ensure(rows*maxIn, e.device(), p->allocEvents, "pool staging");
		for (int s = 0; s < S; ++s) {
			if (!g.active[s] || g.nIn[s] <= 0) continue;
			const smst_stretch *m = g.slots[s];
			for (int c = 0; c < C; ++c) std::copy(m->reqIn[c], m->reqIn[c] + g.nIn[s], g.hIn + row(s, c)*maxIn);
		}
		ensureStage(b, b->dIn, rows*maxIn);
		ensureStage(b, b->dOut, rows*maxOut);
		if (hipMemcpyAsync(b->dIn, g.hIn, rows*maxIn*sizeof(float), hipMemcpyHostToDevice, e.stream()) != hipSuccess) throw smst::Error("hipMemcpyAsync (H2D) failed", true);
		if (hipStreamSynchronize(e.stream()) != hipSuccess) throw smst::Error("hipStreamSynchronize failed", true); // (the silence gate reads the input on another stream)
		e.process(b->dIn, only ? 0 : (long long)C*maxIn, maxIn, g.nIn.data(), b->dOut, only ? 0 : (long long)C*maxOut, maxOut, g.nOut.data(), all ? nullptr : g.active.data());
		// one copy back -> scatter
		g.hOut.ensure(rows*maxOut, e.device(), p->allocEvents, "pool staging");
		if (hipMemcpyAsync(g.hOut, b->dOut, rows*maxOut*sizeof(float), hipMemcpyDeviceToHost, e.stream()) != hipSuccess) throw smst::Error("hipMemcpyAsync (D2H) failed", true);
		if (hipStreamSynchronize(e.stream()) != hipSuccess) throw smst::Error("hipStreamSynchronize failed", true);
		for (int s = 0; s < S; ++s) {
			if (!g.active[s]) continue;
			smst_stretch *m = g.slots[s];
			for (int c = 0; c < C && g.nOut[s] > 0; ++c) std::copy(g.hOut + row(s, c)*maxOut, g.hOut + row(s, c)*maxOut + g.nOut[s], m->reqOut[c]);
			m->pending = false;
			m->reqStatus = SMST_OK;
			m->reqError.clear();
		}
	} catch (const std::exception &err) {
		const smst::Error *own = dynamic_cast<const smst::Error *>(&err);
		for (int s = 0; s < S; ++s) {
			if (!g.active[s]) continue;
			smst_stretch *m = g.slots[s];
			m->pending = false;
			m->reqStatus = (own && own->device) ? SMST_ERR_DEVICE : SMST_ERR_INVALID;
			m->reqError = err.what();
		}
		throw;
	}
	return true;
}
static int runPool(smst_pool *p) {
	int rc = SMST_OK;
	for (size_t i = 0; i < p->groups.size(); ++i) {
		try {
			if (runGroup(p, *p->groups[i], nullptr)) ++p->engineCalls;
		} catch (const smst::Error &e) {
			g_lastError = e.what();
			if (rc == SMST_OK) rc = e.device ? SMST_ERR_DEVICE : SMST_ERR_INVALID;
		} catch (const std::exception &e) {
			g_lastError = e.what();
			if (rc == SMST_OK) rc = SMST_ERR_INVALID;
		}
	}
	return rc;
}
// program order per object: a call that reads or changes a member's state runs the pool first if the member's request is still pending
static void settle(const smst_stretch *h) {
	if (h && h->pool && h->pending) runPool(h->pool);
}
static void unregister(smst_stretch *h) {
	smst_pool *p = h->pool;
	p->members.erase(std::remove(p->members.begin(), p->members.end(), h), p->members.end());
	h->pool = nullptr;
}

int smst_pool_create(smst_pool **out, int device) {
	if (!out) return fail("null output pointer");
	SMST_TRY
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) throw smst::Error("hipGetDeviceCount: no HIP device available (the gfx950 path has no CPU fallback)", true);
	if (device < 0 || device >= n) throw smst::Error("device ordinal " + std::to_string(device) + " out of range: this process sees " + std::to_string(n) + " device(s)");
	smst_pool *p = new smst_pool();
	p->device = device;
	*out = p;
	return SMST_OK;
	SMST_CATCH
}
void smst_pool_destroy(smst_pool *p) {
	if (!p) return;
	runPool(p); // (a failure stays with the members it affected: smst_process_end reports it)
	while (!p->members.empty()) {
		smst_stretch *h = p->members.back();
		if (h->group) {
			try {
				leaveGroup(h);
			} catch (const std::exception &e) { // no engine of its own could be made: the handle survives, unconfigured
				g_lastError = e.what();
				freeSlot(h);
			}
		}
		unregister(h);
	}
	delete p;
}
int smst_pool_attach(smst_pool *p, smst_stretch *h) {
	if (!p || !h) return fail("null pointer");
	if (h->pool) return fail(h->pool == p ? "the handle is already attached to this pool" : "the handle is already attached to another pool");
	if (h->device != p->device) return fail("the handle lives on another device than the pool");
	SMST_TRY
	p->members.push_back(h);
	h->pool = p;
	h->pending = false;
	if (h->batch) {
		try {
			joinGroup(p, h);
		} catch (...) {
			unregister(h);
			throw;
		}
	}
	return SMST_OK;
	SMST_CATCH
}
int smst_pool_detach(smst_stretch *h) {
	if (!h) return fail("null handle");
	if (!h->pool) return fail("the handle is not attached to a pool");
	SMST_TRY
	settle(h);
	if (h->group) leaveGroup(h);
	unregister(h);
	return SMST_OK;
	SMST_CATCH
}
int smst_pool_members(const smst_pool *p) { return p ? int(p->members.size()) : fail("null pool"); }
int smst_pool_pending(const smst_pool *p) {
	if (!p) return fail("null pool");
	int n = 0;
	for (const smst_stretch *h : p->members) n += h->pending ? 1 : 0;
	return n;
}
int smst_pool_run(smst_pool *p) {
	if (!p) return fail("null pool");
	return runPool(p);
}
long long smst_pool_debug_engine_calls(const smst_pool *p) { return p ? p->engineCalls : fail("null pool"); }
long long smst_pool_debug_allocation_events(const smst_pool *p) {
	if (!p) return fail("null pool");
	long long n = p->allocEvents;
	for (const auto &g : p->groups) n += (long long)g->batch->engine->allocationEvents() + g->batch->stagingAllocs;
	return n;
}

void smst_destroy(smst_stretch *h) {
	if (h && h->pool) {
		settle(h);
		if (h->group) freeSlot(h);
		unregister(h);
	}
	delete h;
}

int smst_clone(smst_stretch **out, const smst_stretch *src) {
	if (!out || !src) return fail("null pointer");
	SMST_TRY
	settle(src);
	std::unique_ptr<smst_stretch> h(new smst_stretch());
	h->seed = src->seed; h->device = src->device;
	h->transposeFactor = src->transposeFactor; h->tonalityLimit = src->tonalityLimit; h->transposeSet = src->transposeSet;
	h->formantFactor = src->formantFactor; h->formantComp = src->formantComp; h->formantBase = src->formantBase;
	h->mapTable = src->mapTable;
	if (Batch *ep = engineOf(src)) {
		Batch &e = *ep;
		std::unique_ptr<smst_batch> b(new smst_batch());
		b->engine.reset(new Batch(1, e.channels(), e.blockSamples(), e.intervalSamples(), e.splitComputation(), src->device, src->seed, e.halfPrecisionState()));
		if (src->group) b->engine->moveStreamFrom(e, src->slot, 0); // (the slot's rows stay as they are: the member goes on, the clone is unattached)
		else b->engine->copyStateFrom(e);
		h->batch = std::move(b);
	}
	*out = h.release();
	return SMST_OK;
	SMST_CATCH
}

static void applyParams(smst_stretch *h) {
	Batch &e = *h->batch->engine;
	if (h->transposeSet) e.setTransposeFactor(0, h->transposeFactor, h->tonalityLimit);
	e.setFormantFactor(0, h->formantFactor, h->formantComp);
	e.setFormantBase(0, h->formantBase);
	if (!h->mapTable.empty()) e.setFreqMapTable(0, h->mapTable.data(), int(h->mapTable.size()));
}
int smst_configure(smst_stretch *h, int channels, int block, int interval, int split) {
	if (!h) return fail("null handle");
	SMST_TRY
	// a member is configured as an unattached handle is, on an engine of its own, and then takes a slot in its new geometry's group
	smst_pool *pool = h->pool;
	if (pool) {
		settle(h);
		if (h->group) leaveGroup(h);
	}
	struct Rejoin { // (also when the new geometry is refused: the member keeps its old one)
		smst_pool *pool; smst_stretch *h;
		~Rejoin() { if (pool && h->batch && !h->group) { try { joinGroup(pool, h); } catch (...) {} } }
	} rejoin{pool, h};
	std::unique_ptr<smst_batch> b(new smst_batch());
	b->engine.reset(new Batch(1, channels, block, interval, split != 0, h->device, h->seed));
	if (h->batch) b->engine->inheritAcrossConfigure(*h->batch->engine); // configure() does not reseed the engine (:38-39, :71-94)
	h->batch = std::move(b);
	applyParams(h);
	return SMST_OK;
	SMST_CATCH
}
int smst_preset_default(smst_stretch *h, int channels, float sampleRate, int split) {
	return smst_configure(h, channels, int(sampleRate*0.12), int(sampleRate*0.03), split < 0 ? 0 : split);
}
int smst_preset_cheaper(smst_stretch *h, int channels, float sampleRate, int split) {
	return smst_configure(h, channels, int(sampleRate*0.1), int(sampleRate*0.04), split < 0 ? 1 : split);
}

#define STRETCH_Q(name, expr) int name(const smst_stretch *h) { const Batch *ep = engineOf(h); if (!ep) return fail("unconfigured handle"); const Batch &e = *ep; return (expr); }
STRETCH_Q(smst_block_samples, e.blockSamples())
STRETCH_Q(smst_interval_samples, e.intervalSamples())
STRETCH_Q(smst_input_latency, e.inputLatency())
STRETCH_Q(smst_output_latency, e.outputLatency())
STRETCH_Q(smst_split_computation, e.splitComputation() ? 1 : 0)
STRETCH_Q(smst_seek_length, e.seekLength())
int smst_block_steps(const smst_stretch *h) { settle(h); const Batch *e = engineOf(h); if (!e) return fail("unconfigured handle"); return e->lastBlockSteps(slotOf(h)); }
int smst_blocks_started(const smst_stretch *h) { settle(h); const Batch *e = engineOf(h); if (!e) return fail("unconfigured handle"); return e->lastCallBlocks(slotOf(h)); }
int smst_output_seek_length(const smst_stretch *h, float rate) { const Batch *e = engineOf(h); if (!e) return fail("unconfigured handle"); return e->outputSeekLength(rate); }

#define STRETCH_CALL(body) if (!h) return fail("null handle"); SMST_TRY settle(h); body; return SMST_OK; SMST_CATCH

int smst_reset(smst_stretch *h) {
	STRETCH_CALL({
		if (h->group) h->group->batch->engine->resetStream(h->slot);
		else if (h->batch) h->batch->engine->reset();
	})
}
int smst_set_transpose_factor(smst_stretch *h, float m, float t) {
	STRETCH_CALL({
		h->transposeFactor = m; h->tonalityLimit = t; h->transposeSet = true; h->mapTable.clear();
		if (Batch *e = engineOf(h)) e->setTransposeFactor(slotOf(h), m, t);
	})
}
int smst_set_transpose_semitones(smst_stretch *h, float st, float t) { return smst_set_transpose_factor(h, float(std::pow(2, st/12)), t); }
int smst_set_formant_factor(smst_stretch *h, float m, int comp) {
	STRETCH_CALL({
		h->formantFactor = m; h->formantComp = comp != 0;
		if (Batch *e = engineOf(h)) e->setFormantFactor(slotOf(h), m, comp != 0);
	})
}
int smst_set_formant_semitones(smst_stretch *h, float st, int comp) { return smst_set_formant_factor(h, float(std::pow(2, st/12)), comp); }
int smst_set_formant_base(smst_stretch *h, float f) {
	STRETCH_CALL({
		h->formantBase = f;
		if (Batch *e = engineOf(h)) e->setFormantBase(slotOf(h), f);
	})
}
int smst_set_freq_map_table(smst_stretch *h, const float *table, int n) {
	STRETCH_CALL({
		if (table && n > 0) h->mapTable.assign(table, table + n); else h->mapTable.clear();
		if (Batch *e = engineOf(h)) e->setFreqMapTable(slotOf(h), table, n);
	})
}

// planar pointer arrays -> dense host image [C][n] (the reference indexes buffers[c][i], README.md:46)
static void gatherPlanes(const float *const *planes, int C, int n, std::vector<float> &dense) {
	dense.resize((size_t)C*std::max(n, 1));
	for (int c = 0; c < C; ++c) if (n > 0) std::copy(planes[c], planes[c] + n, dense.begin() + (size_t)c*n);
}
static void scatterPlanes(const std::vector<float> &dense, float *const *planes, int C, int n) {
	for (int c = 0; c < C; ++c) if (n > 0) std::copy(dense.begin() + (size_t)c*n, dense.begin() + (size_t)(c + 1)*n, planes[c]);
}

// The synchronous calls on a MEMBER: the engine call of the unattached handle, on the member's slot alone (an `active` mask of one; the
// member's planes are the whole staging image, every stream stride 0).
static bool badPlanes(const void *const *planes, int C, int n) {
	if (n <= 0) return false;
	if (!planes) return true;
	for (int c = 0; c < C; ++c) if (!planes[c]) return true;
	return false;
}
static int memberSeek(smst_stretch *h, const float *const *inputs, int n, double rate) {
	SMST_TRY
	smst_batch *b = h->group->batch.get();
	Batch &e = *b->engine;
	const int S = e.streams(), C = e.channels(), len = std::max(n, 1);
	if (n < 0 || badPlanes(reinterpret_cast<const void *const *>(inputs), C, n)) throw smst::Error("null buffers with a non-zero sample count");
	std::vector<float> in;
	gatherPlanes(inputs, C, n, in);
	std::vector<int> counts(S, 0);
	std::vector<double> rates(S, 1.0);
	std::vector<unsigned char> mask(S, 0);
	counts[h->slot] = n; rates[h->slot] = rate; mask[h->slot] = 1;
	ensureStage(b, b->dIn, (size_t)C*len);
	hipSetDevice(e.device());
	if (hipMemcpy(b->dIn, in.data(), (size_t)C*len*sizeof(float), hipMemcpyHostToDevice) != hipSuccess) throw smst::Error("hipMemcpy (H2D) failed", true);
	e.seek(b->dIn, 0, len, counts.data(), rates.data(), mask.data());
	e.synchronize();
	return SMST_OK;
	SMST_CATCH
}
static int memberFlush(smst_stretch *h, float *const *outputs, int n, float rate) {
	SMST_TRY
	smst_batch *b = h->group->batch.get();
	Batch &e = *b->engine;
	const int S = e.streams(), C = e.channels(), len = std::max(n, 1);
	if (n < 0 || badPlanes(reinterpret_cast<const void *const *>(outputs), C, n)) throw smst::Error("null buffers with a non-zero sample count");
	std::vector<int> counts(S, 0);
	std::vector<float> rates(S, 0.0f);
	std::vector<unsigned char> mask(S, 0);
	counts[h->slot] = n; rates[h->slot] = rate; mask[h->slot] = 1;
	ensureStage(b, b->dOut, (size_t)C*len);
	e.flush(b->dOut, 0, len, counts.data(), rates.data(), mask.data());
	e.synchronize();
	std::vector<float> out((size_t)C*len);
	if (hipMemcpy(out.data(), b->dOut, out.size()*sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) throw smst::Error("hipMemcpy (D2H) failed", true);
	scatterPlanes(out, outputs, C, n);
	return SMST_OK;
	SMST_CATCH
}
static int reportRequest(const smst_stretch *h) {
	if (h->reqStatus != SMST_OK) g_lastError = h->reqError;
	return h->reqStatus;
}
static int recordRequest(smst_stretch *h, const float *const *inputs, int inputSamples, float *const *outputs, int outputSamples) {
	const int C = h->group->batch->engine->channels();
	if (inputSamples < 0 || outputSamples < 0) return fail("negative sample count");
	if (badPlanes(reinterpret_cast<const void *const *>(inputs), C, inputSamples) || badPlanes(reinterpret_cast<const void *const *>(outputs), C, outputSamples))
		return fail("null buffers with a non-zero sample count");
	h->reqIn = inputs; h->reqIn_n = inputSamples; h->reqOut = outputs; h->reqOut_n = outputSamples;
	h->pending = true;
	return SMST_OK;
}
static int memberProcess(smst_stretch *h, const float *const *inputs, int inputSamples, float *const *outputs, int outputSamples) {
	int rc = recordRequest(h, inputs, inputSamples, outputs, outputSamples);
	if (rc != SMST_OK) return rc;
	SMST_TRY
	runGroup(h->pool, *h->group, h);
	return SMST_OK;
	SMST_CATCH
}

int smst_process_begin(smst_stretch *h, const float *const *inputs, int inputSamples, float *const *outputs, int outputSamples) {
	if (!h) return fail("null handle");
	if (!h->pool) { // not attached: the synchronous call, its status kept for smst_process_end
		h->reqStatus = smst_process(h, inputs, inputSamples, outputs, outputSamples);
		h->reqError = h->reqStatus != SMST_OK ? g_lastError : std::string();
		return h->reqStatus;
	}
	settle(h); // a second begin without an end: the first request runs now
	if (!h->group) return fail("unconfigured handle");
	return recordRequest(h, inputs, inputSamples, outputs, outputSamples);
}
int smst_process_end(smst_stretch *h) {
	if (!h) return fail("null handle");
	if (h->pool && h->pending) {
		runPool(h->pool);
		if (h->pending) { h->pending = false; h->reqStatus = SMST_ERR_INVALID; h->reqError = "the request did not run"; } // (cannot happen: a pending member sits in a group)
	}
	return reportRequest(h);
}

int smst_seek(smst_stretch *h, const float *const *inputs, int inputSamples, double playbackRate) {
	settle(h);
	if (!engineOf(h)) return fail("unconfigured handle");
	if (h->group) return memberSeek(h, inputs, inputSamples, playbackRate);
	std::vector<float> in;
	gatherPlanes(inputs, h->batch->engine->channels(), inputSamples, in);
	return smst_batch_seek(h->batch.get(), in.data(), 0, std::max(inputSamples, 1), &inputSamples, &playbackRate, SMST_MEM_HOST);
}
int smst_process(smst_stretch *h, const float *const *inputs, int inputSamples, float *const *outputs, int outputSamples) {
	settle(h);
	if (!engineOf(h)) return fail("unconfigured handle");
	if (h->group) return memberProcess(h, inputs, inputSamples, outputs, outputSamples);
	const int C = h->batch->engine->channels();
	std::vector<float> in, out((size_t)C*std::max(outputSamples, 1));
	gatherPlanes(inputs, C, inputSamples, in);
	int rc = smst_batch_process(h->batch.get(), in.data(), 0, std::max(inputSamples, 1), &inputSamples, out.data(), 0, std::max(outputSamples, 1), &outputSamples, SMST_MEM_HOST);
	if (rc == SMST_OK) scatterPlanes(out, outputs, C, outputSamples);
	return rc;
}
int smst_flush(smst_stretch *h, float *const *outputs, int outputSamples, float playbackRate) {
	settle(h);
	if (!engineOf(h)) return fail("unconfigured handle");
	if (h->group) return memberFlush(h, outputs, outputSamples, playbackRate);
	const int C = h->batch->engine->channels();
	std::vector<float> out((size_t)C*std::max(outputSamples, 1));
	int rc = smst_batch_flush(h->batch.get(), out.data(), 0, std::max(outputSamples, 1), &outputSamples, &playbackRate, SMST_MEM_HOST);
	if (rc == SMST_OK) scatterPlanes(out, outputs, C, outputSamples);
	return rc;
}
int smst_output_seek(smst_stretch *h, const float *const *inputs, int inputLength) {
	settle(h);
	if (!engineOf(h)) return fail("unconfigured handle");
	if (h->group) {
		// outputSeek() is reset + seek + a pre-roll process + a fold-back over the whole engine (Batch::outputSeek has no stream mask): the
		// member does it on an engine of its own and returns to its group -- two slot moves around a call that is rare and slow anyway
		smst_pool *pool = h->pool;
		SMST_TRY
		leaveGroup(h);
		struct Rejoin { smst_pool *pool; smst_stretch *h; ~Rejoin() { if (h->batch && !h->group) { try { joinGroup(pool, h); } catch (...) {} } } } rejoin{pool, h};
		std::vector<float> in;
		gatherPlanes(inputs, h->batch->engine->channels(), inputLength, in);
		return smst_batch_output_seek(h->batch.get(), in.data(), 0, std::max(inputLength, 1), &inputLength, SMST_MEM_HOST);
		SMST_CATCH
	}
	std::vector<float> in;
	gatherPlanes(inputs, h->batch->engine->channels(), inputLength, in);
	return smst_batch_output_seek(h->batch.get(), in.data(), 0, std::max(inputLength, 1), &inputLength, SMST_MEM_HOST);
}
int smst_exact(smst_stretch *h, const float *const *inputs, int inputSamples, float *const *outputs, int outputSamples) {
	// signalsmith-stretch.h:468-491
	settle(h);
	if (!engineOf(h)) return fail("unconfigured handle");
	Batch &e = *engineOf(h);
	const int C = e.channels();
	const Batch::ExactLengths l = e.exactLengths(inputSamples, outputSamples); // (the lengths smst_batch_exact cuts every stream's clip by)
	const float playbackRate = l.rate;
	const int seekLength = l.seekLength, outputIndex = l.outputIndex;
	if (l.tooShort) {
		for (int c = 0; c < C; ++c) std::fill(outputs[c], outputs[c] + outputSamples, 0.0f);
		g_lastError = kShortMessage;
		return SMST_ERR_SHORT;
	}
	int rc = smst_output_seek(h, inputs, seekLength);
	if (rc != SMST_OK) return rc;
	std::vector<const float *> inOff(C);
	std::vector<float *> outOff(C);
	for (int c = 0; c < C; ++c) inOff[c] = inputs[c] + seekLength;
	rc = smst_process(h, inOff.data(), inputSamples - seekLength, outputs, outputIndex);
	if (rc != SMST_OK) return rc;
	for (int c = 0; c < C; ++c) outOff[c] = outputs[c] + outputIndex;
	return smst_flush(h, outOff.data(), outputSamples - outputIndex, playbackRate);
}

} // extern "C"
