// The tables of a frame-format (_pcm) call's conversions, host side only -- no kernel translation unit includes this.
//
// PcmTableLayout   the per-call table, pinned host staging with a device twin (smst_staging.h).  Six sections of a batch of S streams, in order:
//                    inCounts   [S] int            frames each stream feeds     (uploaded on its own, by the input side)
//                    outCounts  [S] int            frames each stream emits
//                    dither     [S] PcmDither      mode, hash, index of the call's first frame
//                    level      [S] PcmLevel       mode, gain, ceiling
//                    loud       [S] LoudEntry      filter, gate, target, meter flag and caps of a measured stream (h == 0: not measured)
//                    weights    [kMaxChannels] float
//                  What a call's output side needs is a run of neighbouring sections: ONE copy (upload()).
// PcmMeters        the batch's [3][S] meter words, device: the peaks since the last take (float bits), the gains the newest conversions
//                  applied, the clip peaks of the newest exact call (kClipPeak's; stream-ordered, so one set serves calls in flight)
// PcmDebugBlock    what a levelled debug hook uploads in front of its launch: the table's dither and level sections, then the meter words
// PcmOutCall       where one call's output conversion finds all of that on the device
// ResampleTableLayout  the table a whole-clip call with a resampled stream adds on the input side (the engine's; two sets as the above)
// StreamResampleTableLayout  the table a streaming call adds on the input side where a stream has the stream-resample setting
// ResampleOutTableLayout  the table a whole-clip call with an out-resampled stream adds on the output side (the engine's; two sets)
// StreamResampleOutTableLayout  the table a streaming call adds on the output side where a stream has the stream-output-resample setting
#pragma once
#include "smst_device.h"
#include <cstddef>
#include <cstring>

namespace smst {

// null members: not in this call (dither: the call does not dither; level.table: not a levelled batch; loud: no stream is measured -- none in the loudness mode, none with the meter flag)
struct PcmOutCall {
	unsigned *overs = nullptr; // [S][2] counters: clamped, NaN
	const PcmDither *dither = nullptr;
	PcmLevelIo level;
	const LoudEntry *loud = nullptr;
	const float *loudWeights = nullptr;
};

// the T at `offset` bytes behind `base`: the one cast of this header
template <typename T> inline T *pcmTableAt(void *base, size_t offset) { return reinterpret_cast<T *>(static_cast<unsigned char *>(base) + offset); }

struct PcmTableLayout {
	size_t S;
	explicit PcmTableLayout(int streams) : S(size_t(streams)) {}
	// byte offsets of the sections, and of the end
	size_t inCounts() const { return 0; }
	size_t outCounts() const { return inCounts() + S*sizeof(int); }
	size_t dither() const { return outCounts() + S*sizeof(int); }
	size_t level() const { return dither() + S*sizeof(PcmDither); }
	size_t loud() const { return level() + S*sizeof(PcmLevel); }
	size_t weights() const { return loud() + S*sizeof(LoudEntry); }
	size_t bytes() const { return weights() + kMaxChannels*sizeof(float); }
	// a section of the table at `base`: the pinned host copy or the device twin
	int *inCounts(void *base) const { return pcmTableAt<int>(base, inCounts()); }
	int *outCounts(void *base) const { return pcmTableAt<int>(base, outCounts()); }
	PcmDither *dither(void *base) const { return pcmTableAt<PcmDither>(base, dither()); }
	PcmLevel *level(void *base) const { return pcmTableAt<PcmLevel>(base, level()); }
	LoudEntry *loud(void *base) const { return pcmTableAt<LoudEntry>(base, loud()); }
	float *weights(void *base) const { return pcmTableAt<float>(base, weights()); }
	// The bytes the output side of a call uploads: from the output counts where they ride along, else from the dither entries, to the end of
	// the last section the call reads.  A levelled batch's calls carry the dither entries in front of the level entries whether they dither
	// or not; only a levelled batch has a measured stream
	struct Range { size_t offset, bytes; };
	Range upload(bool withOutCounts, bool dithered, bool levelled, bool loudness) const {
		const size_t first = withOutCounts ? outCounts() : dither();
		const size_t end = levelled ? (loudness ? bytes() : loud()) : dithered ? level() : dither();
		return Range{first, end - first};
	}
};
// Every section begins on a multiple of its element's alignment, for every S, where the table does (hipMalloc and hipHostMalloc give 16 bytes
// and more): the bytes one stream adds in front of a section are a multiple of that alignment
static_assert(sizeof(PcmDither) == 16 && sizeof(PcmLevel) == 16, "the table's entries are 16 bytes");
static_assert(alignof(PcmDither) <= sizeof(int) && alignof(PcmLevel) <= sizeof(int) && alignof(float) <= sizeof(int), "counts in front of entries of 4-byte members");
static_assert(alignof(LoudEntry) <= 16 && (2*sizeof(int) + sizeof(PcmDither) + sizeof(PcmLevel)) % alignof(LoudEntry) == 0, "the loudness entries' doubles are 8-byte aligned");
static_assert(sizeof(LoudEntry) % alignof(float) == 0 && sizeof(LoudEntry) % sizeof(int) == 0, "the channel weights are aligned, and the table is whole ints");

// ResampleTableLayout: what a whole-clip call with a resampled stream adds (include/smst.h, "Resample"), a table of its own beside the one
// above -- pinned host staging with a device twin, as that one, and uploaded in ONE copy.  Three sections of a batch of S streams, in order:
//   rawSegs  [S][2] ClipSeg        kClipIn's segments into the raw image: a resampled stream's whole clip, N frames from frame 0 to column 0
//   dstSegs  [S][2] ClipSeg        where kClipResample puts the stream's Nr frames in the input image: the call's two input segments
//   entries  [S]    ResampleEntry  N, Nr, the reduced ratio, its shape and where its table lies in device memory (L == 0: not resampled)
struct ResampleTableLayout {
	size_t S;
	explicit ResampleTableLayout(int streams) : S(size_t(streams)) {}
	size_t rawSegs() const { return 0; }
	size_t dstSegs() const { return rawSegs() + 2*S*sizeof(ClipSeg); }
	size_t entries() const { return dstSegs() + 2*S*sizeof(ClipSeg); }
	size_t bytes() const { return entries() + S*sizeof(ResampleEntry); }
	ClipSeg *rawSegs(void *base) const { return pcmTableAt<ClipSeg>(base, rawSegs()); }
	ClipSeg *dstSegs(void *base) const { return pcmTableAt<ClipSeg>(base, dstSegs()); }
	ResampleEntry *entries(void *base) const { return pcmTableAt<ResampleEntry>(base, entries()); }
};
static_assert(sizeof(ClipSeg) == 16 && alignof(ResampleEntry) <= 16, "the entries begin on a 16-byte boundary where the table does");

// StreamResampleTableLayout: what a streaming call adds on the input side where a stream of the batch has the setting of include/smst.h,
// "Stream resample" -- a table of its own beside the two above, pinned host staging with a device twin, uploaded in ONE copy.  Three sections
// of a batch of S streams, in order:
//   plainCounts  [S] int                  kPcmIn's counts into the engine's input image: the call's frames of a stream without the setting, 0 for one with it
//   rawCounts    [S] int                  kPcmIn's counts into the raw image: the call's frames of a stream with the setting, 0 for one without
//   entries      [S] StreamResampleEntry  taps, shape, n, k, fed, made and the set of lines the call reads (L == 0: no setting)
struct StreamResampleTableLayout {
	size_t S;
	explicit StreamResampleTableLayout(int streams) : S(size_t(streams)) {}
	size_t plainCounts() const { return 0; }
	size_t rawCounts() const { return plainCounts() + S*sizeof(int); }
	size_t entries() const { return rawCounts() + S*sizeof(int); }
	size_t bytes() const { return entries() + S*sizeof(StreamResampleEntry); }
	int *plainCounts(void *base) const { return pcmTableAt<int>(base, plainCounts()); }
	int *rawCounts(void *base) const { return pcmTableAt<int>(base, rawCounts()); }
	StreamResampleEntry *entries(void *base) const { return pcmTableAt<StreamResampleEntry>(base, entries()); }
};
static_assert(alignof(StreamResampleEntry) <= 2*sizeof(int) && sizeof(StreamResampleEntry)%8 == 0, "the entries' 64-bit members are aligned behind two runs of S ints");

// ResampleOutTableLayout: what a whole-clip call with an out-resampled stream adds (include/smst.h, "Output resample"), a table of its own --
// pinned host staging with a device twin, uploaded in ONE copy.  Three sections of a batch of S streams, in order:
//   srcSegs  [S][2] ClipSeg           where the stream's E rendered frames lie in the output image: the main process's frames, then the flush's
//   dstSegs  [S][2] ClipSeg           where kClipResampleOut puts the stream's Nd delivered frames in the same image: one segment, at the third column
//   entries  [S]    ResampleOutEntry  E, Nd, the reduced ratio, its shape and where its table lies in device memory (L == 0: no ratio)
struct ResampleOutTableLayout {
	size_t S;
	explicit ResampleOutTableLayout(int streams) : S(size_t(streams)) {}
	size_t srcSegs() const { return 0; }
	size_t dstSegs() const { return srcSegs() + 2*S*sizeof(ClipSeg); }
	size_t entries() const { return dstSegs() + 2*S*sizeof(ClipSeg); }
	size_t bytes() const { return entries() + S*sizeof(ResampleOutEntry); }
	ClipSeg *srcSegs(void *base) const { return pcmTableAt<ClipSeg>(base, srcSegs()); }
	ClipSeg *dstSegs(void *base) const { return pcmTableAt<ClipSeg>(base, dstSegs()); }
	ResampleOutEntry *entries(void *base) const { return pcmTableAt<ResampleOutEntry>(base, entries()); }
};
static_assert(alignof(ResampleOutEntry) <= 16, "the entries begin on a 16-byte boundary where the table does");

// StreamResampleOutTableLayout: what a streaming call adds on the output side where a stream of the batch has the setting of include/smst.h,
// "Stream output resample" -- a table of its own, pinned host staging with a device twin, uploaded in ONE copy.  One section:
//   entries  [S] StreamResampleOutEntry  taps, shape, Nd, E, Dl, delivered, rendered and the set of lines the call reads (L == 0: no setting)
struct StreamResampleOutTableLayout {
	size_t S;
	explicit StreamResampleOutTableLayout(int streams) : S(size_t(streams)) {}
	size_t entries() const { return 0; }
	size_t bytes() const { return entries() + S*sizeof(StreamResampleOutEntry); }
	StreamResampleOutEntry *entries(void *base) const { return pcmTableAt<StreamResampleOutEntry>(base, entries()); }
};
static_assert(alignof(StreamResampleOutEntry) <= 16 && sizeof(StreamResampleOutEntry)%8 == 0, "the entries begin on a 16-byte boundary where the table does");

struct PcmMeters {
	size_t S;
	explicit PcmMeters(int streams) : S(size_t(streams)) {}
	size_t words() const { return 3*S; }
	size_t bytes() const { return words()*sizeof(int); }
	// as a batch begins with them: no peak, gain 1, no clip peak
	void start(int *words) const {
		const float one = 1.0f;
		std::memset(words, 0, bytes());
		for (size_t s = 0; s < S; ++s) std::memcpy(words + S + s, &one, sizeof one);
	}
	PcmLevelIo io(const PcmLevel *table, int *words) const {
		PcmLevelIo l;
		l.table = table; l.peaks = words; l.applied = reinterpret_cast<float *>(words + S); l.clipPeak = words + 2*S;
		return l;
	}
	// a take reads the peaks and the applied gains, which lie in front, and clears the peaks
	size_t takeBytes() const { return 2*S*sizeof(int); }
	size_t clearBytes() const { return S*sizeof(int); }
	void taken(const int *words, float *peaks, float *applied) const {
		if (peaks) std::memcpy(peaks, words, S*sizeof(float));
		if (applied) std::memcpy(applied, words + S, S*sizeof(float));
	}
};

struct PcmDebugBlock {
	PcmTableLayout table;
	PcmMeters meters;
	explicit PcmDebugBlock(int streams) : table(streams), meters(streams) {}
	size_t level() const { return table.level() - table.dither(); }
	size_t words() const { return table.loud() - table.dither(); }
	size_t bytes() const { return words() + meters.bytes(); }
	// the sections of a block at `base`
	PcmDither *dither(void *base) const { return pcmTableAt<PcmDither>(base, 0); }
	PcmLevel *level(void *base) const { return pcmTableAt<PcmLevel>(base, level()); }
	int *words(void *base) const { return pcmTableAt<int>(base, words()); }
};

} // namespace smst
