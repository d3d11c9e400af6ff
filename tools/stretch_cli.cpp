// Command-line front-end over the C ABI (include/smst.h): the same job as the reference's example CLI
// (cmd/main.cpp:11-86 -- WAV in, outputSeek / process / flush, WAV out; same flags and defaults), plus a batch mode
// that renders MANY files with one geometry in a single batched GPU call (the data-parallel axis of this
// implementation).
//
//   stretch_cli [--semitones=S] [--formant=S] [--formant-comp] [--formant-base=Hz] [--tonality=Hz] [--time=F]
//               [--split-computation] [--device=N] [--out-format=s16|s24|f32] [--dither=none|tpdf|tpdf-hp] [--dither-seed=N]
//               [--exact] [--gain=dB] [--protect=dBFS | --normalize=dBFS] [--loudness=LUFS] [--true-peak]
//               [--limit] [--limit-lookahead=ms] [--loudness-range] [--max-short-term=LUFS] [--max-momentary=LUFS] [--rate=HZ]
//               [--out-rate=source|HZ]
//               in.wav out.wav [in2.wav out2.wav ...]
//
// --out-format (also "--out-format s24"): the samples of the files written -- 16-bit (the default, as the reference's CLI writes), 24-bit by the
// library's rounding rule for SMST_PCM_S24, or float32.
// --dither: TPDF dither of the 16-bit / 24-bit samples written (include/smst.h, "Dither"): white (tpdf) or with its power moved towards
// Nyquist (tpdf-hp); none, the default, is the tool as it was.  --dither-seed=N (default 0): file k is stream k, hence seed N + k.  With
// dither the main process and the flush run through smst_batch_process_pcm / smst_batch_flush_pcm, which quantise on the GPU -- the flush
// goes on with the frame counter --, and the frames are written as they come back.  Those calls take their input in the output's format:
// an input that format cannot hold exactly (24-bit or float input with --out-format=s16) is refused rather than rounded.
// --exact: every file is rendered by smst_batch_exact_pcm -- the reference's exact(): its seams instead of the three stages of cmd/main.cpp --
// on frames of the output's format, with the same refusal of an input that format cannot hold.
// --gain=dB: a fixed output gain (include/smst.h, "Level"), in either flow; in the default one it sends the process stage and the flush
// through the _pcm calls, as --dither does.  --protect=dBFS and --normalize=dBFS (one of them; both imply --exact): the gain comes from the
// rendered clip's own peak -- lowered (from --gain, or 0 dB) only where the clip would exceed the ceiling, or set so that the peak meets
// it.  INTEGRATION.md says which ceiling keeps an integer format free of clamped samples.  dB -> linear: float(pow(10, dB/20)).  With any
// of the three, one line per file: "level: <file> peak=<%.9g> gain=<%.9g> overs=<clamped samples>" -- the peak before the gain.
// --loudness=LUFS (implies --exact; not with --normalize): every rendered clip is brought to that integrated loudness (ITU-R BS.1770-4,
// measured on the GPU at the files' sample rate; include/smst.h, "Loudness"), with --protect=dBFS as the ceiling that limits the gain
// (none without it; --gain is not used).  The line then reads "level: <file> loudness=<%.4f> peak=... gain=... overs=...": the measured
// loudness in LUFS before the gain, -inf for a clip that has none (shorter than 400 ms, silent).
// --true-peak (needs the exact flow: --exact, or one of --protect / --normalize / --loudness, which imply it): every rendered clip's true
// peak is measured on the GPU (a 4x interpolation between the samples; include/smst.h, "True peak") and the ceilings of --protect,
// --normalize and --loudness are dBTP: the gain comes from the true peak instead of the sample peak.  Alone it only meters.  The line of a
// file then ends in " true-peak=<%.4f>": the true peak before the gain, in dBTP (-inf for silence).
// --limit (needs --protect or --loudness; refused with --normalize, which meets its ceiling by construction): the --protect ceiling no
// longer lowers the gain of the whole file -- the file keeps --gain, or reaches its --loudness target -- and a lookahead limiter on the GPU
// (include/smst.h, "Limiter") brings down the frames that would exceed it; with --true-peak, the frames whose inter-sample values would.
// --limit-lookahead=ms (default 1.5) is converted to frames with the batch's sample rate; a short lookahead weakens a dBTP ceiling.  The
// line of a file then ends in " limit=<%.4f> limited=<frames>": the deepest gain reduction in dB (0 where nothing was limited) and the
// number of frames that were reduced.
// --loudness-range (needs the exact flow, as --true-peak does): every rendered clip's maximum momentary loudness, maximum short-term
// loudness and loudness range (EBU Tech 3341 / 3342; include/smst.h, "Loudness range") are measured on the GPU at the files' sample rate,
// before the gain, and printed: "range: <file> momentary-max=<%.4f> short-term-max=<%.4f> lra=<%.4f>", the maxima in LUFS (-inf for
// silence and for a clip too short to have one), the range in LU.  Alone it only meters.
// --max-short-term=LUFS and --max-momentary=LUFS (they need --loudness): caps on the two maxima of the file as written (EBU R 128 s1) --
// the gain is the lowest of the target's and the caps'.
// --rate=HZ (needs --exact, or a flag that implies it): the batch is created, and the files are written, at HZ; an input file of another
// integer rate is resampled on the GPU on its way in (include/smst.h, "Resample"; the ratio comes from smst_resample_ratio), so files of
// different rates form one batch.  A file's output length is round(Nr*time), today's rule on its length at HZ.  One line per file:
// "resample: <file> <its rate> Hz -> <HZ> Hz ratio=<up>/<down>".
// --out-rate=source|HZ (needs --rate): every file is written at its own input rate (source) or at HZ instead of the batch's rate -- the
// rendered clip is resampled on the GPU behind the engine (include/smst.h, "Output resample"; the ratio comes from
// smst_resample_ratio(batch rate, delivery rate)), in front of the loudness, true-peak, limiter and dither stages, which therefore see the
// samples that are written: --loudness and --loudness-range measure at each file's delivery rate.  A file's output length is
// round(N*time*delivery rate/its own rate), from its own length N.  --limit-lookahead stays one count of frames for the batch, converted
// at the batch's rate.  One more line per file: "out-resample: <file> <batch rate> Hz -> <rate> Hz ratio=<up>/<down>".
// Files given together must share sample rate and channel count (they form one batch); lengths may differ.  With --rate only the channel
// count must be shared.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../include/smst.h"
#include "wav_io.h"

static double flagValue(int argc, char **argv, const char *name, double fallback) {
	const std::string prefix = std::string("--") + name + "=";
	for (int i = 1; i < argc; ++i) if (!std::strncmp(argv[i], prefix.c_str(), prefix.size())) return std::atof(argv[i] + prefix.size());
	return fallback;
}
static bool hasValue(int argc, char **argv, const char *name) {
	const std::string prefix = std::string("--") + name + "=";
	for (int i = 1; i < argc; ++i) if (!std::strncmp(argv[i], prefix.c_str(), prefix.size())) return true;
	return false;
}
static float fromDecibels(double dB) { return float(std::pow(10.0, dB/20.0)); }
static bool hasFlag(int argc, char **argv, const char *name) {
	const std::string flag = std::string("--") + name;
	for (int i = 1; i < argc; ++i) if (flag == argv[i]) return true;
	return false;
}
// --name=value or --name value; consumed[i] marks the arguments that are no file names
static std::string flagText(int argc, char **argv, const char *name, const char *fallback, std::vector<bool> &consumed) {
	const std::string flag = std::string("--") + name, prefix = flag + "=";
	std::string value = fallback;
	for (int i = 1; i < argc; ++i) {
		if (!std::strncmp(argv[i], prefix.c_str(), prefix.size())) value = argv[i] + prefix.size();
		else if (flag == argv[i] && i + 1 < argc) { value = argv[i + 1]; consumed[i + 1] = true; }
	}
	return value;
}
#define CHECK(call) do { if ((call) != SMST_OK) { std::fprintf(stderr, "%s: %s\n", #call, smst_last_error()); return 1; } } while (0)

int main(int argc, char **argv) {
	if (hasFlag(argc, argv, "v")) { int v[3]; smst_reference_version(v); std::printf("%d.%d.%d\n", v[0], v[1], v[2]); return 0; }
	const double semitones = flagValue(argc, argv, "semitones", 0), formants = flagValue(argc, argv, "formant", 0);
	const double formantBase = flagValue(argc, argv, "formant-base", 100), tonality = flagValue(argc, argv, "tonality", 8000);
	const double time = flagValue(argc, argv, "time", 1);
	const bool formantComp = hasFlag(argc, argv, "formant-comp"), split = hasFlag(argc, argv, "split-computation");
	const int device = int(flagValue(argc, argv, "device", 0));
	std::vector<bool> consumed(argc, false);
	const std::string outFormat = flagText(argc, argv, "out-format", "s16", consumed);
	if (outFormat != "s16" && outFormat != "s24" && outFormat != "f32") {
		std::fprintf(stderr, "--out-format is s16, s24 or f32\n");
		return 2;
	}
	const std::string ditherName = flagText(argc, argv, "dither", "none", consumed);
	const int dither = ditherName == "none" ? SMST_DITHER_NONE : ditherName == "tpdf" ? SMST_DITHER_TPDF : ditherName == "tpdf-hp" ? SMST_DITHER_TPDF_HP : -1;
	const long long ditherSeed = std::strtoll(flagText(argc, argv, "dither-seed", "0", consumed).c_str(), nullptr, 10);
	if (dither < 0) {
		std::fprintf(stderr, "--dither is none, tpdf or tpdf-hp\n");
		return 2;
	}
	if (dither != SMST_DITHER_NONE && outFormat == "f32") {
		std::fprintf(stderr, "--dither applies to --out-format s16 and s24: float32 samples are not quantised\n");
		return 2;
	}
	const bool hasGain = hasValue(argc, argv, "gain"), protect = hasValue(argc, argv, "protect"), normalize = hasValue(argc, argv, "normalize");
	if (protect && normalize) {
		std::fprintf(stderr, "--protect and --normalize exclude each other\n");
		return 2;
	}
	const bool loudness = hasValue(argc, argv, "loudness");
	if (loudness && normalize) {
		std::fprintf(stderr, "--loudness and --normalize exclude each other\n");
		return 2;
	}
	const bool truePeak = hasFlag(argc, argv, "true-peak");
	const bool exact = hasFlag(argc, argv, "exact") || protect || normalize || loudness, levelled = hasGain || protect || normalize || loudness || truePeak;
	if (truePeak && !exact) {
		std::fprintf(stderr, "--true-peak needs --exact (or --protect, --normalize or --loudness, which imply it): whole clips only\n");
		return 2;
	}
	const bool limit = hasFlag(argc, argv, "limit");
	if (limit && normalize) {
		std::fprintf(stderr, "--limit and --normalize exclude each other: a normalised file meets its ceiling by construction\n");
		return 2;
	}
	if (limit && !protect && !loudness) {
		std::fprintf(stderr, "--limit needs --protect=dBFS (its ceiling) or --loudness=LUFS\n");
		return 2;
	}
	const bool loudnessRange = hasFlag(argc, argv, "loudness-range"), capShortTerm = hasValue(argc, argv, "max-short-term"), capMomentary = hasValue(argc, argv, "max-momentary");
	if (loudnessRange && !exact) {
		std::fprintf(stderr, "--loudness-range needs --exact (or --protect, --normalize or --loudness, which imply it): whole clips only\n");
		return 2;
	}
	if ((capShortTerm || capMomentary) && !loudness) {
		std::fprintf(stderr, "--max-short-term and --max-momentary need --loudness=LUFS: they cap the gain that reaches its target\n");
		return 2;
	}
	const bool resample = hasValue(argc, argv, "rate");
	const double rate = flagValue(argc, argv, "rate", 0);
	if (resample && !exact) {
		std::fprintf(stderr, "--rate needs --exact (or --protect, --normalize or --loudness, which imply it): whole clips only\n");
		return 2;
	}
	const std::string outRateText = flagText(argc, argv, "out-rate", "", consumed);
	const bool outResample = !outRateText.empty(), outRateSource = outRateText == "source";
	if (outResample && !resample) {
		std::fprintf(stderr, "--out-rate needs --rate=HZ: it delivers each file at a rate other than the batch's\n");
		return 2;
	}
	if (outResample && !outRateSource && !(std::atof(outRateText.c_str()) >= 1)) {
		std::fprintf(stderr, "--out-rate is source or a sample rate in Hz\n");
		return 2;
	}
	const double limitLookaheadMs = flagValue(argc, argv, "limit-lookahead", 1.5);
	const float gain = fromDecibels(flagValue(argc, argv, "gain", 0)), ceiling = fromDecibels(flagValue(argc, argv, protect ? "protect" : "normalize", 0));
	std::vector<std::string> files;
	for (int i = 1; i < argc; ++i) if (std::strncmp(argv[i], "--", 2) && !consumed[i]) files.push_back(argv[i]);
	if (files.size() < 2 || files.size()%2) {
		std::fprintf(stderr, "usage: %s [flags] in.wav out.wav [in2.wav out2.wav ...]\n", argv[0]);
		return 2;
	}
	const int S = int(files.size()/2);
	std::vector<WavData> inputs(S);
	std::string error;
	for (int s = 0; s < S; ++s) {
		if (!readWav(files[2*s], inputs[s], error)) { std::fprintf(stderr, "%s\n", error.c_str()); return 1; }
		if ((!resample && inputs[s].sampleRate != inputs[0].sampleRate) || inputs[s].channels != inputs[0].channels) {
			std::fprintf(stderr, "all files of a batch must share sample rate and channel count\n");
			return 1;
		}
		std::printf("%s -> %s\n", files[2*s].c_str(), files[2*s + 1].c_str());
	}
	const int C = int(inputs[0].channels);
	const double batchRate = resample ? rate : double(inputs[0].sampleRate); // the rate of the batch and of the files written
	const float sr = float(batchRate);

	smst_batch *batch = nullptr;
	CHECK(smst_batch_create_preset(&batch, S, C, 0, sr, split ? 1 : 0, device, 0)); // presetDefault, cmd/main.cpp:45
	CHECK(smst_batch_set_transpose_semitones(batch, -1, float(semitones), float(tonality/sr)));  // :46
	CHECK(smst_batch_set_formant_semitones(batch, -1, float(formants), formantComp));             // :47
	CHECK(smst_batch_set_formant_base(batch, -1, float(formantBase/sr)));                         // :48
	if (resample) for (int s = 0; s < S; ++s) { // the files' ratios: HZ over each file's own rate
		int up = 1, down = 1;
		CHECK(smst_resample_ratio(double(inputs[s].sampleRate), rate, &up, &down));
		CHECK(smst_batch_set_pcm_resample(batch, s, up, down));
		std::printf("resample: %s %d Hz -> %.0f Hz ratio=%d/%d\n", files[2*s].c_str(), int(inputs[s].sampleRate), rate, up, down);
	}
	std::vector<double> deliveryRate(S, batchRate); // the rate each file is written at
	if (outResample) for (int s = 0; s < S; ++s) { // the files' output ratios: each file's delivery rate over HZ
		deliveryRate[s] = outRateSource ? double(inputs[s].sampleRate) : std::atof(outRateText.c_str());
		int up = 1, down = 1;
		CHECK(smst_resample_ratio(batchRate, deliveryRate[s], &up, &down));
		CHECK(smst_batch_set_pcm_out_resample(batch, s, up, down));
		std::printf("out-resample: %s %.0f Hz -> %.0f Hz ratio=%d/%d\n", files[2*s].c_str(), batchRate, deliveryRate[s], up, down);
	}
	const int inLat = smst_batch_input_latency(batch), outLat = smst_batch_output_latency(batch), interval = smst_batch_interval_samples(batch);

	// per-stream lengths of the three stages, exactly as cmd/main.cpp:55-82 computes them
	const int seekLength = smst_batch_output_seek_length(batch, float(1/time));
	std::vector<int> outLen(S), outIndex(S), inIndex(S), procIn(S), tail(S), seekLens(S, seekLength);
	int maxIn = 0, maxOut = 0;
	for (int s = 0; s < S; ++s) {
		const int n = int(inputs[s].length());
		long long atRate = n; // the file's length at the batch's rate
		if (resample && (atRate = smst_batch_resampled_length(batch, s, n)) < 0) { std::fprintf(stderr, "%s: %s\n", files[2*s].c_str(), smst_last_error()); return 1; }
		outLen[s] = outResample ? int(std::round(n*time*deliveryRate[s]/double(inputs[s].sampleRate))) : int(std::round(atRate*time));
		outIndex[s] = std::max(0, outLen[s] - interval);
		const int outputPos = outIndex[s] + outLat;
		const int inputPos = int(std::round(outputPos/time));
		inIndex[s] = std::max(inputPos + inLat, seekLength);
		procIn[s] = inIndex[s] - seekLength;
		tail[s] = outLen[s] - outIndex[s];
		maxIn = std::max(maxIn, std::max(inIndex[s], n));
		maxOut = std::max(maxOut, outLen[s]);
	}
	maxIn = std::max(maxIn, 1); maxOut = std::max(maxOut, 1);
	std::vector<float> in((size_t)S*C*maxIn, 0.0f), out((size_t)S*C*maxOut, 0.0f); // zero padding = inWav.resize(inputIndex), :73
	for (int s = 0; s < S; ++s) for (int c = 0; c < C; ++c)
		std::copy(inputs[s].samples[c].begin(), inputs[s].samples[c].end(), in.begin() + ((size_t)s*C + c)*maxIn);
	const long long iss = (long long)C*maxIn, ics = maxIn, oss = (long long)C*maxOut, ocs = maxOut;

	if (!exact) CHECK(smst_batch_output_seek(batch, in.data(), iss, ics, seekLens.data(), SMST_MEM_HOST));                        // :58-59
	if (dither != SMST_DITHER_NONE || levelled || exact) {
		// frames of the output's format, quantised (dithered: stream s has seed ditherSeed + s; levelled) by the library
		const int format = outFormat == "s24" ? SMST_PCM_S24 : outFormat == "f32" ? SMST_PCM_F32 : SMST_PCM_S16, bits = outFormat == "s24" ? 24 : outFormat == "f32" ? 32 : 16;
		const size_t esz = size_t(bits/8);
		const float scale = bits == 24 ? 8388608.0f : 32768.0f;
		if (dither != SMST_DITHER_NONE) CHECK(smst_batch_set_pcm_dither(batch, -1, dither, ditherSeed));
		if (loudness && outResample) { for (int s = 0; s < S; ++s) CHECK(smst_batch_set_pcm_loudness(batch, s, flagValue(argc, argv, "loudness", 0), protect ? ceiling : INFINITY, deliveryRate[s])); }
		else if (loudness) CHECK(smst_batch_set_pcm_loudness(batch, -1, flagValue(argc, argv, "loudness", 0), protect ? ceiling : INFINITY, batchRate));
		else if (levelled) CHECK(smst_batch_set_pcm_level(batch, -1, protect ? SMST_LEVEL_PROTECT : normalize ? SMST_LEVEL_NORMALISE : SMST_LEVEL_FIXED, gain, ceiling));
		if (truePeak) CHECK(smst_batch_set_pcm_true_peak(batch, -1, 1));
		if (limit) {
			CHECK(smst_batch_set_pcm_limiter_lookahead(batch, int(std::lround(limitLookaheadMs*1e-3*batchRate))));
			CHECK(smst_batch_set_pcm_limiter(batch, -1, 1));
		}
		if (loudnessRange && outResample) { for (int s = 0; s < S; ++s) CHECK(smst_batch_set_pcm_loudness_range(batch, s, 1, deliveryRate[s])); }
		else if (loudnessRange) CHECK(smst_batch_set_pcm_loudness_range(batch, -1, 1, batchRate));
		if (capShortTerm || capMomentary) CHECK(smst_batch_set_pcm_loudness_caps(batch, -1, flagValue(argc, argv, "max-momentary", INFINITY), flagValue(argc, argv, "max-short-term", INFINITY)));
		// `count` samples of file s from sample `first` on as frames at `frames`; false: one of them is no value of the format
		auto toFrames = [&](int s, int first, int count, unsigned char *frames) {
			for (int i = 0; i < count; ++i) for (int c = 0; c < C; ++c) {
				const float v = in[((size_t)s*C + c)*maxIn + first + i];
				unsigned char *p = frames + ((size_t)i*C + c)*esz;
				if (format == SMST_PCM_F32) { std::memcpy(p, &v, 4); continue; }
				const float q = std::fmin(scale - 1.0f, std::fmax(-scale, std::round(v*scale)));
				if (!(q/scale == v)) {
					std::fprintf(stderr, "%s: sample %d is no %d-bit value: frames need an input that --out-format holds exactly\n", files[2*s].c_str(), first + i, bits);
					return false;
				}
				const uint32_t code = uint32_t(int32_t(q));
				for (size_t k = 0; k < esz; ++k) p[k] = (unsigned char)(code >> (8*k));
			}
			return true;
		};
		std::vector<unsigned char> outFrames((size_t)S*maxOut*C*esz, 0);
		if (exact) {
			std::vector<int> inLen(S), status(S, SMST_OK);
			for (int s = 0; s < S; ++s) inLen[s] = int(inputs[s].length());
			std::vector<unsigned char> inFrames((size_t)S*maxIn*C*esz, 0);
			for (int s = 0; s < S; ++s) if (!toFrames(s, 0, inLen[s], inFrames.data() + (size_t)s*maxIn*C*esz)) return 1;
			CHECK(smst_batch_exact_pcm(batch, inFrames.data(), (long long)maxIn*C, C, inLen.data(), outFrames.data(), (long long)maxOut*C, C, outLen.data(), status.data(), format, SMST_MEM_HOST));
			for (int s = 0; s < S; ++s) if (status[s] != SMST_OK) {
				std::fprintf(stderr, "%s: too short for --exact at this rate\n", files[2*s].c_str());
				return 1;
			}
		} else {
			int maxProc = 1;
			for (int s = 0; s < S; ++s) maxProc = std::max(maxProc, procIn[s]);
			const int tailLen = std::max(interval, 1);
			std::vector<unsigned char> inFrames((size_t)S*maxProc*C*esz, 0), tailFrames((size_t)S*tailLen*C*esz, 0);
			for (int s = 0; s < S; ++s) if (!toFrames(s, seekLength, procIn[s], inFrames.data() + (size_t)s*maxProc*C*esz)) return 1;
			CHECK(smst_batch_process_pcm(batch, inFrames.data(), (long long)maxProc*C, C, procIn.data(), outFrames.data(), (long long)maxOut*C, C, outIndex.data(), format, SMST_MEM_HOST));
			CHECK(smst_batch_flush_pcm(batch, tailFrames.data(), (long long)tailLen*C, C, tail.data(), nullptr, format, SMST_MEM_HOST));
			for (int s = 0; s < S; ++s)
				std::copy(tailFrames.begin() + (size_t)s*tailLen*C*esz, tailFrames.begin() + ((size_t)s*tailLen + tail[s])*C*esz, outFrames.begin() + ((size_t)s*maxOut + outIndex[s])*C*esz);
		}
		if (levelled) {
			std::vector<long long> clamped(S, 0);
			std::vector<float> peaks(S, 0.0f), gains(S, 1.0f);
			CHECK(smst_batch_take_pcm_overs(batch, clamped.data(), nullptr));
			CHECK(smst_batch_take_pcm_peaks(batch, peaks.data(), gains.data()));
			std::vector<double> lufs(S, 0.0);
			if (loudness) CHECK(smst_batch_take_pcm_loudness(batch, lufs.data(), nullptr, nullptr));
			std::vector<float> truePeaks(S, 0.0f);
			if (truePeak) CHECK(smst_batch_take_pcm_true_peaks(batch, truePeaks.data()));
			std::vector<float> minGains(S, 1.0f);
			std::vector<long long> limitedFrames(S, 0);
			if (limit) CHECK(smst_batch_take_pcm_limiter(batch, minGains.data(), limitedFrames.data()));
			for (int s = 0; s < S; ++s) {
				std::printf("level: %s ", files[2*s + 1].c_str());
				if (loudness) std::printf("loudness=%.4f ", lufs[s]);
				std::printf("peak=%.9g gain=%.9g overs=%lld", peaks[s], gains[s], clamped[s]);
				if (truePeak) std::printf(" true-peak=%.4f", 20.0*std::log10(double(truePeaks[s])));
				if (limit) std::printf(" limit=%.4f limited=%lld", 20.0*std::log10(double(minGains[s])), limitedFrames[s]);
				std::printf("\n");
			}
		}
		if (loudnessRange) {
			std::vector<double> momentary(S, 0.0), shortTerm(S, 0.0), range(S, 0.0);
			CHECK(smst_batch_take_pcm_loudness_range(batch, momentary.data(), shortTerm.data(), range.data(), nullptr, nullptr, nullptr, nullptr));
			for (int s = 0; s < S; ++s) std::printf("range: %s momentary-max=%.4f short-term-max=%.4f lra=%.4f\n", files[2*s + 1].c_str(), momentary[s], shortTerm[s], range[s]);
		}
		for (int s = 0; s < S; ++s) {
			if (!writeWavFrames(files[2*s + 1], resample ? unsigned(deliveryRate[s]) : inputs[s].sampleRate, inputs[s].channels, bits, outFrames.data() + (size_t)s*maxOut*C*esz, size_t(outLen[s]), error, format == SMST_PCM_F32)) {
				std::fprintf(stderr, "%s\n", error.c_str());
				return 1;
			}
		}
		smst_batch_destroy(batch);
		return 0;
	}
	CHECK(smst_batch_process(batch, in.data() + seekLength, iss, ics, procIn.data(), out.data(), oss, ocs, outIndex.data(), SMST_MEM_HOST)); // :77-78
	// flush writes at each stream's own output offset: stage through a second buffer and splice
	std::vector<float> tails((size_t)S*C*std::max(interval, 1), 0.0f);
	CHECK(smst_batch_flush(batch, tails.data(), (long long)C*std::max(interval, 1), std::max(interval, 1), tail.data(), nullptr, SMST_MEM_HOST)); // :81-82
	for (int s = 0; s < S; ++s) for (int c = 0; c < C; ++c)
		std::copy(tails.begin() + ((size_t)s*C + c)*std::max(interval, 1), tails.begin() + ((size_t)s*C + c)*std::max(interval, 1) + tail[s],
		          out.begin() + ((size_t)s*C + c)*maxOut + outIndex[s]);

	for (int s = 0; s < S; ++s) {
		WavData result;
		result.sampleRate = inputs[s].sampleRate;
		result.channels = inputs[s].channels;
		result.samples.assign(C, std::vector<float>(outLen[s]));
		for (int c = 0; c < C; ++c) std::copy(out.begin() + ((size_t)s*C + c)*maxOut, out.begin() + ((size_t)s*C + c)*maxOut + outLen[s], result.samples[c].begin());
		const bool written = outFormat == "s24" ? writeWav24(files[2*s + 1], result, error) : outFormat == "f32" ? writeWavFloat32(files[2*s + 1], result, error) : writeWav16(files[2*s + 1], result, error);
		if (!written) { std::fprintf(stderr, "%s\n", error.c_str()); return 1; }
	}
	smst_batch_destroy(batch);
	return 0;
}
