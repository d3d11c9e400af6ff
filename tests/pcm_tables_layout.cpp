// The layout types of csrc/smst_pcm_tables.h against the formulas the C API wrote out by hand before the header existed.  Stand-alone: built
// and run by tests/test_pcm_tables_layout.py (g++ -I tests/emu, with the sanitizers where the compiler has them); exit status 0 = all held.
#include "smst_pcm_tables.h"
#include <cstdint>
#include <cstdio>
#include <vector>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d (S = %d): %s\n", __FILE__, __LINE__, S, #cond); ++failures; } } while (0)

int main() {
	for (int S : {1, 2, 3, 5, 64}) {
		const smst::PcmTableLayout at(S);
		const size_t n = size_t(S);
		// the sections, in order, and the size
		CHECK(at.inCounts() == 0);
		CHECK(at.outCounts() == n*4);
		CHECK(at.dither() == 2*n*4);
		CHECK(at.level() == 2*n*4 + n*16);
		CHECK(at.loud() == 2*n*4 + n*16 + n*16);
		CHECK(at.weights() == 2*n*4 + n*16 + n*16 + n*sizeof(smst::LoudEntry));
		CHECK(at.bytes() == 2*n*4 + n*16 + n*16 + n*sizeof(smst::LoudEntry) + 16*4);
		// ... which is the count of ints the tables were allocated with
		CHECK(at.bytes() == (2*n + n*((sizeof(smst::PcmDither) + sizeof(smst::PcmLevel) + sizeof(smst::LoudEntry))/sizeof(int)) + smst::kMaxChannels)*sizeof(int));
		// the views over a 16-byte-aligned base: at the offsets, aligned for their elements, writable from end to end
		std::vector<unsigned char> store(at.bytes() + 16);
		unsigned char *base = store.data() + (16 - reinterpret_cast<uintptr_t>(store.data())%16)%16;
		auto offsetOf = [&](const void *p) { return size_t(static_cast<const unsigned char *>(p) - base); };
		auto aligned = [](const void *p, size_t a) { return reinterpret_cast<uintptr_t>(p)%a == 0; };
		CHECK(offsetOf(at.inCounts(base)) == at.inCounts() && aligned(at.inCounts(base), alignof(int)));
		CHECK(offsetOf(at.outCounts(base)) == at.outCounts() && aligned(at.outCounts(base), alignof(int)));
		CHECK(offsetOf(at.dither(base)) == at.dither() && aligned(at.dither(base), alignof(smst::PcmDither)));
		CHECK(offsetOf(at.level(base)) == at.level() && aligned(at.level(base), alignof(smst::PcmLevel)));
		CHECK(offsetOf(at.loud(base)) == at.loud() && aligned(at.loud(base), alignof(smst::LoudEntry)) && aligned(at.loud(base), 8));
		CHECK(offsetOf(at.weights(base)) == at.weights() && aligned(at.weights(base), alignof(float)));
		for (int s = 0; s < S; ++s) {
			at.inCounts(base)[s] = at.outCounts(base)[s] = s;
			at.dither(base)[s] = smst::PcmDither{1u, 2u, 3u, 4u};
			at.level(base)[s] = smst::PcmLevel{0u, 1.0f, 1.0f, 0u};
			at.loud(base)[s] = smst::LoudEntry{};
		}
		for (int k = 0; k < smst::kMaxChannels; ++k) at.weights(base)[k] = 1.0f;
		CHECK(offsetOf(at.weights(base) + smst::kMaxChannels) == at.bytes());
		// the upload: what the call before the header computed, for all eight combinations (a stream is in the loudness mode only in a
		// levelled batch: the flag counted only there)
		for (int flags = 0; flags < 8; ++flags) for (int withOutCounts = 0; withOutCounts < 2; ++withOutCounts) {
			const bool dithered = flags & 1, levelled = flags & 2, anyLoud = flags & 4;
			const bool loud = levelled && anyLoud;
			const size_t first = withOutCounts ? n : 2*n; // in ints
			const size_t bytes = (2*n - first)*sizeof(int) + (levelled ? n*(sizeof(smst::PcmDither) + sizeof(smst::PcmLevel)) : dithered ? n*sizeof(smst::PcmDither) : 0)
			                     + (loud ? n*sizeof(smst::LoudEntry) + smst::kMaxChannels*sizeof(float) : 0);
			const smst::PcmTableLayout::Range r = at.upload(withOutCounts != 0, dithered, levelled, anyLoud);
			CHECK(r.offset == first*sizeof(int));
			CHECK(r.bytes == bytes);
			CHECK(r.offset + r.bytes <= at.bytes());
		}
		// the meter words: [3][S]; no peak, gain 1, no clip peak
		const smst::PcmMeters meters(S);
		CHECK(meters.words() == 3*n && meters.bytes() == 3*n*sizeof(int));
		CHECK(meters.takeBytes() == 2*n*sizeof(int) && meters.clearBytes() == n*sizeof(int));
		std::vector<int> words(meters.words(), -1);
		meters.start(words.data());
		const smst::PcmLevelIo io = meters.io(at.level(base), words.data());
		CHECK(io.table == at.level(base) && io.peaks == words.data() && io.clipPeak == words.data() + 2*n && io.loudGain == nullptr);
		CHECK(static_cast<void *>(io.applied) == static_cast<void *>(words.data() + n));
		std::vector<float> peaks(n, -1.0f), applied(n, -1.0f);
		meters.taken(words.data(), peaks.data(), applied.data());
		for (int s = 0; s < S; ++s) {
			CHECK(io.peaks[s] == 0 && io.clipPeak[s] == 0 && io.applied[s] == 1.0f);
			CHECK(peaks[s] == 0.0f && applied[s] == 1.0f);
		}
		// a levelled debug hook's block: S dither entries, S level entries, the meter words
		const smst::PcmDebugBlock block(S);
		CHECK(block.level() == n*sizeof(smst::PcmDither));
		CHECK(block.words() == n*(sizeof(smst::PcmDither) + sizeof(smst::PcmLevel)));
		CHECK(block.bytes() == n*(sizeof(smst::PcmDither) + sizeof(smst::PcmLevel)) + 3*n*sizeof(int));
		std::vector<unsigned char> blockStore(block.bytes() + 16);
		unsigned char *b0 = blockStore.data() + (16 - reinterpret_cast<uintptr_t>(blockStore.data())%16)%16;
		CHECK(static_cast<void *>(block.dither(b0)) == b0 && static_cast<void *>(block.level(b0)) == b0 + block.level() && static_cast<void *>(block.words(b0)) == b0 + block.words());
		block.meters.start(block.words(b0));
		for (int s = 0; s < S; ++s) {
			block.dither(b0)[s] = smst::PcmDither{};
			block.level(b0)[s] = smst::PcmLevel{};
		}
		CHECK(block.words(b0)[n] == 0x3f800000 && block.words(b0)[3*n - 1] == 0);
	}
	std::printf(failures ? "%d check(s) failed\n" : "pcm_tables_layout: all checks held\n", failures);
	return failures ? 1 : 0;
}
