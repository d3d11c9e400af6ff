// Which form of the bin recurrence a tile takes: ONE function (recurrenceForm, smst_vocoder.hip) from the batch's geometry and switches and what the
// tile's hops need, asked once per tile by the engine (Batch::runTilesRange) and handed to the analysis (`twisted`), to the choice of the record pass
// (`fused()`) and to the one launcher of the recurrence.  Host only.
#pragma once
#include "smst_device.h"

namespace smst {
enum class RecurrenceKernel {
	CHAIN_UNFUSED, // kPredictB + kChain: records through HBM (9-16 channels, vertical steps the fused kernels do not cover, SMST_NO_FUSE)
	ONE,           // kVocoderOne: a tile in which no stream has more than one hop, one chain per stream
	ACROSS,        // kVocoder ACROSS: such a tile, mono / stereo -- lanes of the recurrence wave = streams
	MANY,          // kVocoderN: 3-8 channels
	GATHER,        // kVocoder, mono / stereo, producers that gather from HBM: mapped tiles, random time factors, a start bin, vertical steps 6 / 7
	STAGED,        // kVocoder, producers with per-row windows in LDS: plain bounded tiles, L <= 5
	ALIGNED,       // kVocoder, line-aligned producers: plain bounded tiles, L = 4 (SMST_ALIGN_ALL: L <= 4), fp32 state, whole lines
	CONTINUOUS,    // kVocoderCont: a run of two or more tiles that would each be ALIGNED, as one wavefront (SMST_CONTINUOUS; Batch::continuousApplies)
};
struct RecurrenceForm {
	RecurrenceKernel kernel; // (never CONTINUOUS: that is a run of tiles, launchVocoderContinuous)
	bool twisted;  // ALIGNED: the tile's Xprev rows take the finished previous-hop twists from the analysis pass instead of Band.prevInput
	bool interior; // ALIGNED: some producer wave of the launch runs interior blocks (what the kernel decides per wave; the launch counter)
	bool rotInLds; // GATHER / ACROSS, mapped tiles: the hop rotation table beside the rings, where the CU's LDS holds both
	bool fused() const { return kernel != RecurrenceKernel::CHAIN_UNFUSED; } // the records stay in LDS: no record pass, the producers read the carried feed-forward state
};
// the engine's switches that take part in the decision (smst_switches.h; those of the producers travel in DevBatch)
struct FormSwitches { bool noFuse, noSingleHop, noAcross, continuous; };

// tileHops: the most hops the call has left for this tile, over all streams (at most kTileHops); nStreams: streams of the sub-batch;
// pendingRun: the run of split-computation blocks in flight (Batch::runPendingBlocks)
RecurrenceForm recurrenceForm(const DevBatch &d, const TileSummary &th, int tileHops, int nStreams, bool pendingRun, const FormSwitches &sw);
// Whether some tile of the batch can take `kernel` -- what the allocations ask.  CHAIN_UNFUSED: every tile does (the records need a place in
// memory); CONTINUOUS: the third workspace; ONE: every one-hop tile takes ONE or ACROSS (a call of such tiles keeps one hop descriptor per stream).
bool formReachable(const DevBatch &d, const FormSwitches &sw, RecurrenceKernel kernel);
// plain: the tile has neither a frequency map nor formants (TileSummary::plain)
void launchRecurrence(const DevBatch &d, const RecurrenceForm &form, int sBase, int nStreams, int hopBase, bool plain, hipStream_t st);

} // namespace smst
