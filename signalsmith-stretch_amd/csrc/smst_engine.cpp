// Host-side engine implementation.  See smst_engine.h.
#include "smst_engine.h"
#include "smst_switches.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <complex>
#include <cstdlib>
#include <cstring>

namespace smst {

#define SMST_HIP(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) throw Error(std::string(#expr) + ": " + hipGetErrorString(e_), true); } while (0)

void throwDeviceError(const char *call, hipError_t e) { throw Error(std::string(call) + ": " + hipGetErrorString(e), true); }

static constexpr float kNoiseFloor = 1e-15f;     // signalsmith-stretch.h:508
static constexpr float kMaxCleanStretch = 2.0f;  // :509
static constexpr unsigned long long kEngineModulus = 2147483647ull; // 2^31 - 1: the random engine is libstdc++'s minstd_rand0 (:616; smst_kernels_common.h: engineDraw)

// fftSamples chosen by the L1 layer: 2*fastSizeAbove(ceil(block/2)) with fast sizes {4,5,6,8}*2^k
// (probe-verified for 5760/5292/4800/9600/11520).
static int fastSizeAbove(int size) {
	int power2 = 1;
	while (power2*8 < size) power2 *= 2;
	int multiple = (size + power2 - 1)/power2;
	if (multiple == 7) ++multiple;
	return multiple*power2;
}

static FftPlan makePlan(int H, int N) {
	FftPlan plan{};
	plan.H = H;
	plan.N = N;
	int rem = H, odd = 1;
	while (rem%3 == 0) { rem /= 3; odd *= 3; }
	while (rem%5 == 0) { rem /= 5; odd *= 5; }
	int log2 = 0;
	while (rem%2 == 0) { rem /= 2; ++log2; }
	if (rem != 1 || (odd != 1 && odd != 3 && odd != 5)) throw Error("unsupported FFT size (need 2^k * {1,3,5})");
	int n = 0;
	for (int i = 0; i < log2/2; ++i) plan.radix[n++] = 4;
	if (log2%2) plan.radix[n++] = 2;
	if (odd > 1) plan.radix[n++] = odd;
	if (n > kMaxFftPasses) throw Error("FFT too long");
	plan.npass = n;
	return plan;
}

// Kaiser window, heuristic-optimal bandwidth, forced to perfect reconstruction
static std::vector<float> makeWindow(int B, int I) {
	auto bessel0 = [](double x) {
		double result = 0, term = 1, m = 0;
		while (term > 1e-4) {
			result += term;
			++m;
			term *= (x*x)/(4*m*m);
		}
		return result;
	};
	std::vector<float> w(B);
	double bandwidth = double(B)/double(I);
	double bw = bandwidth + 8/((bandwidth + 3)*(bandwidth + 3)) + 0.25*std::max(3 - bandwidth, 0.0);
	bw = std::max(bw, 2.0);
	double beta = M_PI*std::sqrt(bw*bw*0.25 - 1);
	double invB0 = 1/bessel0(beta);
	for (int i = 0; i < B; ++i) {
		double r = (2*double(i) + 1)/double(B) - 1;
		double arg = std::sqrt(std::max(0.0, 1 - r*r));
		w[i] = float(bessel0(beta*arg)*invB0);
	}
	for (int j = 0; j < I && j < B; ++j) {
		float sum2 = 0;
		for (int i = j; i < B; i += I) sum2 += w[i]*w[i];
		float gain = 1/std::sqrt(sum2);
		for (int i = j; i < B; i += I) w[i] *= gain;
	}
	return w;
}

template <typename T> T *Batch::devAlloc(size_t count) {
	void *p = nullptr;
	if (count == 0) count = 1;
	SMST_HIP(hipMalloc(&p, count*sizeof(T)));
	allocations.push_back(p);
	++allocEvents;
	return static_cast<T *>(p);
}
template <typename T> T *Batch::pinnedAlloc(size_t count) {
	void *p = nullptr;
	if (count == 0) count = 1;
	SMST_HIP(hipHostMalloc(&p, count*sizeof(T), hipHostMallocDefault));
	pinned.push_back(p);
	++allocEvents;
	return static_cast<T *>(p);
}
void Batch::pinnedFree(void *p) {
	if (!p) return;
	auto it = std::find(pinned.begin(), pinned.end(), p);
	if (it != pinned.end()) pinned.erase(it);
	hipHostFree(p);
}
void Batch::devFree(void *p) {
	if (!p) return;
	auto it = std::find(allocations.begin(), allocations.end(), p);
	if (it != allocations.end()) allocations.erase(it);
	hipFree(p);
}

Batch::Batch(int streams, int channels, int block, int interval, bool splitComputation, int device, long seed, bool halfPrecisionState)
	: S(streams), C(channels), B(block), I(interval), split(splitComputation), halfState(halfPrecisionState), dev(device) {
	// geometry first: nothing below may throw before the HIP objects exist, and everything after is covered by the
	// clean-up in the catch block (a throwing constructor does not run the destructor)
	if (S < 1 || C < 1 || C > kMaxChannels || B < 4 || I < 1 || I > B) throw Error("invalid configuration (need 1.." + std::to_string(kMaxChannels) + " channels, interval <= block)");
	N = 2*fastSizeAbove((B + 1)/2);
	M = N/2;
	if (M > kMaxBands) throw Error("block too long: " + std::to_string(M) + " bands, at most 16384 (one FFT buffer of bands*8 bytes must fit a CU's LDS; up to 9600 bands both buffers do, beyond that the second one lives in memory)");
	L = int(std::round(float(N)/float(I))); // longVerticalStep, signalsmith-stretch.h:636-637
	if (L < 1) L = 1;
	{
		int ring = 4;
		while (ring < L + 2) ring *= 2;
		if (ring > 64) throw Error("interval too small relative to the FFT size (vertical step too long)");
		// kChain (9-16 channels, a vertical step the fused kernels do not take, or SMST_NO_FUSE -- so any channel count) keeps a ring of
		// `ring` bins per channel and lane in LDS: up to 4 channels the vertical step may be 62, 5-9 channels 30, 10-16 channels 14
		if (chainLdsBytes(C, ring) > kLdsBytesPerCU)
			throw Error("vertical step round(fftSamples/interval) = " + std::to_string(L) + " too long for " + std::to_string(C) +
			            " channels: at most 62 for 1-4 channels, 30 for 5-9, 14 for 10-16 (the un-fused recurrence keeps a history ring per channel in LDS)");
	}
	const FftPlan plan = makePlan(M, N);
	try {
		construct(plan, seed);
	} catch (...) {
		releaseAll();
		throw;
	}
}

void Batch::construct(const FftPlan &plan, long seed) {
	SMST_HIP(hipSetDevice(dev));
	createStreamsAndEvents();
	readSwitches(plan);
	uploadConstantTables();
	allocateCarriedState();
	allocateCallTables();
	initHostRows(seed);
	allocateWorkspace();
	allocateSplitTables();
	SMST_HIP(hipDeviceSynchronize()); // the hipMemset calls above are ordered with the null stream only; the engine's streams are non-blocking
	reset();
}

void Batch::createStreamsAndEvents() {
	SMST_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
	{ // the recurrence is latency-bound with few waves: give its stream the highest priority so its workgroups are
	  // dispatched ahead of the bulk kernels' when they share the machine (raising the analysis stream as well makes
	  // the recurrence wait for CUs: measured 1.9 ms instead of 1.2 ms per launch)
		int lo = 0, hi = 0;
		SMST_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
		SMST_HIP(hipStreamCreateWithPriority(&stChain, hipStreamNonBlocking, hi));
	}
	SMST_HIP(hipStreamCreateWithFlags(&stSynth, hipStreamNonBlocking));
	SMST_HIP(hipStreamCreateWithFlags(&stGate, hipStreamNonBlocking));
	callSets.create();
	stageSets.create();
	for (CallSet &cs : callSets.sets) SMST_HIP(hipEventCreateWithFlags(&cs.tables, hipEventDisableTiming));
	SMST_HIP(hipEventCreateWithFlags(&evStart, hipEventDisableTiming));
	SMST_HIP(hipEventCreateWithFlags(&evOrder, hipEventDisableTiming));
	for (int i = 0; i < 3; ++i) {
		SMST_HIP(hipEventCreateWithFlags(&evFeed[i], hipEventDisableTiming));
		SMST_HIP(hipEventCreateWithFlags(&evChain[i], hipEventDisableTiming));
		SMST_HIP(hipEventCreateWithFlags(&evOut[i], hipEventDisableTiming));
		SMST_HIP(hipEventCreateWithFlags(&evSynth[i], hipEventDisableTiming));
	}
}

void Batch::readSwitches(const FftPlan &plan) { // ... and the geometry, into `d`
	// the cross-check switches: one struct, one table, read once (smst_switches.h)
	const Switches sw = Switches::fromEnvironment();
	overlap = sw.overlap; formSwitches = FormSwitches{sw.noFuse, sw.noSingleHop, sw.noAcross, sw.continuous}; carriedEmit = sw.carriedEmit != 0; checkLaunches = sw.checkLaunches; contWriterWave = sw.contWriterWave;
	workspaceGiB = sw.workspaceGiB;
	subStreamsAsked = sw.subStreams;

	d.S = S; d.C = C; d.B = B; d.I = I; d.M = M; d.N = N; d.L = L; d.T = kTileHops;
	d.histLen = B + I;
	d.carryLen = B + I;
	d.delta = split ? I : 0;
	d.lag = L + 1;
	int ring = 4;
	while (ring < d.lag + 1) ring *= 2;
	d.ringSlots = ring;
	d.plan = plan;
	d.mapTableLen = 0;
	d.halfState = halfState ? 1 : 0;
	d.debugMode = sw.debugMode;
	d.noFeedFusion = sw.noFeedFusion;
	d.noStage = sw.noStage;
	d.vocNWide = sw.vocNWide;
	d.vocWide = sw.vocWide;
	d.vocNHalfLines = sw.vocNHalfLines;
	d.noAlign = sw.noAlign;
	d.vocInterior = sw.vocInterior;
	d.alignAll = sw.alignAll;
	d.noFastFft = sw.noFastFft;
	// lean FFT tables (8-byte window entries + generated modulation, six stage twiddles instead of fifteen) are OPT-IN: they take 0.2 ms
	// off a 16.3-ms step, and their one extra rounding per element (spectra 1.2e-7 away from the full tables') flipped a peak decision
	// of a noise stream in tests/test_parity_gpu.py::test_batch_ragged -- parity first
	d.fftLean = sw.fftLean ? 1 : 0;
	d.feedSerial = sw.feedSerial;
	d.fftTeams = sw.fftTeams;
	d.analysePairs = sw.analysePairs;
	d.vocTwist = sw.vocTwist;
	d.synthEmit = sw.synthEmit;
	{
		int cus = 0;
		SMST_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
		d.teamsGrid = std::max(8, cus/8*8);
	}
}

void Batch::uploadConstantTables() {
	std::vector<float2> tw(M), half(M), rot(M);
	for (int j = 0; j < M; ++j) {
		double a = -2*M_PI*double(j)/double(M);
		tw[j] = make_float2(float(std::cos(a)), float(std::sin(a)));
		double h = -M_PI*double(j)/double(N);
		half[j] = make_float2(float(std::cos(h)), float(std::sin(h)));
	}
	{ // hop rotation, evaluated with the reference's own fp32 recurrence (signalsmith-stretch.h:647-655)
		const float f0 = (0.0f + 0.5f)/float(N), f1 = (1.0f + 0.5f)/float(N);
		std::complex<float> r = std::polar(1.0f, f0*float(I)*float(2*M_PI));
		const float freqStep = f1 - f0;
		const std::complex<float> step = std::polar(1.0f, freqStep*float(I)*float(2*M_PI));
		for (int b = 0; b < M; ++b) {
			rot[b] = make_float2(r.real(), r.imag());
			r = std::complex<float>(r.real()*step.real() - r.imag()*step.imag(), r.real()*step.imag() + r.imag()*step.real());
		}
	}
	std::vector<float> win = makeWindow(B, I), wprod(B);
	for (int i = 0; i < B; ++i) wprod[i] = win[i]*win[i]*float(N);
	// reset(0.1) window-product seed: three phantom blocks at weight 0.1, read position one interval in
	{
		std::vector<float> wp(B, 0.0f);
		for (int i = 0; i < B; ++i) wp[i] += wprod[i];
		for (int i = B - I - 1; i >= 0; --i) wp[i] += wp[i + I];
		for (auto &v : wp) v = v*0.1f + 1e-30f;
		seedCarryWp.assign(d.carryLen, 1e-30f);
		for (int r = 0; r + I < B; ++r) seedCarryWp[r] = wp[r + I];
	}

	auto upload = [&](const void *src, size_t bytes) {
		void *p = devAlloc<unsigned char>(bytes);
		SMST_HIP(hipMemcpy(p, src, bytes, hipMemcpyHostToDevice));
		return p;
	};
	d.twH = static_cast<float2 *>(upload(tw.data(), M*sizeof(float2)));
	d.halfTw = static_cast<float2 *>(upload(half.data(), M*sizeof(float2)));
	d.rot = static_cast<float2 *>(upload(rot.data(), M*sizeof(float2)));
	{
		std::vector<unsigned> pw(2*(size_t)M);
		unsigned long long x = 1;
		for (size_t j = 0; j < pw.size(); ++j) {
			x = x*16807ull % kEngineModulus;
			pw[j] = unsigned(x);
		}
		lcgHopJump = pw[2*(size_t)M - 3]; // 16807^(2M - 2): the draws of one randomised hop
		d.lcgPow = static_cast<unsigned *>(upload(pw.data(), pw.size()*sizeof(unsigned)));
	}
	d.window = static_cast<float *>(upload(win.data(), B*sizeof(float)));
	{ // folded analysis tables and, for H = 256*R3, the stage twiddles of the register-blocked FFT
		const int halfB = B/2;
		std::vector<float2> wa(M), wb(M);
		for (int m = 0; m < M; ++m) {
			float a = (m < B - halfB) ? win[m + halfB] : 0.0f;
			float b = (m >= M - halfB) ? win[m - M + halfB] : 0.0f;
			wa[m] = make_float2(a*half[m].x, a*half[m].y);        // w * e^{-i pi m/N}
			wb[m] = make_float2(-b*half[m].y, b*half[m].x);       // i * w * e^{-i pi m/N}
		}
		d.winA = static_cast<float2 *>(upload(wa.data(), M*sizeof(float2)));
		d.winB = static_cast<float2 *>(upload(wb.data(), M*sizeof(float2)));
		std::vector<float4> w4(M), st4(M);
		for (int m = 0; m < M; ++m) {
			w4[m] = make_float4(wa[m].x, wa[m].y, wb[m].x, wb[m].y);
			st4[m] = make_float4(half[m].x, half[m].y, (m < B - halfB) ? win[m + halfB] : 0.0f, (m >= M - halfB) ? win[m - M + halfB] : 0.0f);
		}
		d.win4 = static_cast<float4 *>(upload(w4.data(), M*sizeof(float4)));
		d.synTab = static_cast<float4 *>(upload(st4.data(), M*sizeof(float4)));
		{ // lean tables: the window samples alone (the modulation e^{-i pi m/N} is generated from halfTw[t] and constants)
			std::vector<float2> w2(M);
			for (int m = 0; m < M; ++m) w2[m] = make_float2((m < B - halfB) ? win[m + halfB] : 0.0f, (m >= M - halfB) ? win[m - M + halfB] : 0.0f);
			d.win2 = static_cast<float2 *>(upload(w2.data(), M*sizeof(float2)));
		}
		d.twA4 = d.twB4 = d.twA6 = nullptr;
		if (isFastSize(M)) { // the register-blocked FFT's sizes: 16 x 16 x R3
			const int R3 = M/256, MA = 16*R3;
			std::vector<float2> ta((size_t)15*MA), tb((size_t)15*R3); // w^(n p), rows [n - 1][p]: host only, paired into the tables below
			for (int n = 1; n < 16; ++n) {
				for (int p = 0; p < MA; ++p) {
					double a = -2*M_PI*double(p*n)/double(M);
					ta[(size_t)(n - 1)*MA + p] = make_float2(float(std::cos(a)), float(std::sin(a)));
				}
				for (int p = 0; p < R3; ++p) {
					double a = -2*M_PI*double(p*n)/double(MA);
					tb[(size_t)(n - 1)*R3 + p] = make_float2(float(std::cos(a)), float(std::sin(a)));
				}
			}
			std::vector<float4> ta4((size_t)8*MA), tb4((size_t)8*R3);
			for (int i = 0; i < 8; ++i) {
				for (int p = 0; p < MA; ++p) {
					const float2 lo = ta[(size_t)(2*i)*MA + p], hi = (2*i + 1 < 15) ? ta[(size_t)(2*i + 1)*MA + p] : make_float2(1.f, 0.f);
					ta4[(size_t)i*MA + p] = make_float4(lo.x, lo.y, hi.x, hi.y);
				}
				for (int p = 0; p < R3; ++p) {
					const float2 lo = tb[(size_t)(2*i)*R3 + p], hi = (2*i + 1 < 15) ? tb[(size_t)(2*i + 1)*R3 + p] : make_float2(1.f, 0.f);
					tb4[(size_t)i*R3 + p] = make_float4(lo.x, lo.y, hi.x, hi.y);
				}
			}
			std::vector<float4> ta6((size_t)3*MA);
			for (int p = 0; p < MA; ++p) {
				auto tw = [&](int n) { return ta[(size_t)(n - 1)*MA + p]; };
				ta6[p] = make_float4(tw(1).x, tw(1).y, tw(2).x, tw(2).y);
				ta6[(size_t)MA + p] = make_float4(tw(3).x, tw(3).y, tw(4).x, tw(4).y);
				ta6[(size_t)2*MA + p] = make_float4(tw(8).x, tw(8).y, tw(12).x, tw(12).y);
			}
			d.twA6 = static_cast<float4 *>(upload(ta6.data(), ta6.size()*sizeof(float4)));
			d.twA4 = static_cast<float4 *>(upload(ta4.data(), ta4.size()*sizeof(float4)));
			d.twB4 = static_cast<float4 *>(upload(tb4.data(), tb4.size()*sizeof(float4)));
		}
	}
	d.wprod = static_cast<float *>(upload(wprod.data(), B*sizeof(float)));

}

// The one list of the carried device arrays (CarriedArray, smst_engine.h).  The typed pointers of the narrowed arrays address half-sized
// allocations; every access goes through the accessors at the top of smst_kernels_common.h.
std::array<Batch::CarriedArray, Batch::kCarriedArrays> Batch::carriedArrays() {
	const size_t band = (size_t)C*M, word = sizeof(float), stored = halfState ? sizeof(half_t) : sizeof(float);
	auto at = [](auto *&p) { return reinterpret_cast<void **>(&p); };
	auto single = [&](auto *&p, size_t rowBytes) { return CarriedArray{{at(p), nullptr}, nullptr, rowBytes, false, false, 0, false}; };
	auto twice = [&](auto *(&p)[2], const int &cur, size_t rowBytes) { return CarriedArray{{at(p[0]), at(p[1])}, &cur, rowBytes, false, false, 0, false}; };
	std::array<CarriedArray, kCarriedArrays> a{};
	a[kStInput] = single(d.stInput, band*2*word);
	a[kStPrev] = single(d.stPrev, band*2*word);
	a[kStOut] = single(d.stOut, band*2*stored);
	a[kStEnergy] = single(d.stEnergy, band*stored);
	a[kStEnergy].slack = 16; // (PrevEnergy::at reads 8 bytes at an element)
	a[kStEnergy].zeroed = true;
	a[kHist] = single(d.hist, (size_t)C*d.histPitch*word);
	a[kHistBase] = twice(d.histBase, d.histCur, sizeof(int));
	a[kCarryBase] = twice(d.carryBase, d.carryCur, sizeof(int)); // (a row of the overlap-add carry moves with its carryBase entry: the window keeps its place in the row)
	a[kHistBase].zeroed = a[kCarryBase].zeroed = true;
	a[kCarrySum] = twice(d.carrySum, d.carryCur, (size_t)C*d.carryPitch*stored);
	a[kCarryWp] = twice(d.carryWp, d.carryCur, (size_t)d.carryPitch*word);
	a[kStFreq] = single(d.stFreq, 2*word);
	// the block in flight: its spectra, Band.input and (re-analysed) Band.prevInput (PendingBlock, smst_engine.h)
	a[kPendIn] = single(dPendIn, (size_t)C*d.Mp*2*word);
	a[kPendPrev] = single(dPendPrev, (size_t)C*d.Mp*2*word);
	a[kPendIn].splitOnly = a[kPendPrev].splitOnly = true;
	a[kPendIn].zeroed = a[kPendPrev].zeroed = true;
	a[kStOut].narrowed = a[kStEnergy].narrowed = a[kCarrySum].narrowed = halfState;
	return a;
}
void Batch::allocateCarried(int first, int last) { // entries [first, last) of the list, double-buffered ones half by half
	const auto list = carriedArrays();
	for (int h = 0; h < 2; ++h)
		for (int i = first; i < last; ++i) {
			const CarriedArray &a = list[i];
			if (h >= a.halves()) continue;
			const size_t bytes = (size_t)S*a.rowBytes + a.slack;
			*a.ptr[h] = devAlloc<unsigned char>(bytes);
			if (a.zeroed) SMST_HIP(hipMemset(*a.ptr[h], 0, bytes));
		}
}

void Batch::allocateCarriedState() {
	d.histPitch = 2*d.histLen;
	d.carryPitch = d.carryLen + 2*I;
	allocateCarried(kStInput, kHistBase);
	dZeroEmit = devAlloc<EmitDesc>(S); // (settleCarry)
	SMST_HIP(hipMemset(dZeroEmit, 0, (size_t)S*sizeof(EmitDesc)));
	allocateCarried(kHistBase, kStFreq);
	d.wpHeadLen = ((B + I - 1)/I + 2)*I;
	d.wpHead = devAlloc<float>((size_t)S*d.wpHeadLen);
	allocateCarried(kStFreq, kPendIn);
}

void Batch::allocateCallTables() {
	dParams = devAlloc<StreamParams>(S);
	hParams = pinnedAlloc<StreamParams>(S);
	d.params = d.paramsPeaks = d.paramsForm0 = d.paramsForm2 = dParams;
	dEnergy = devAlloc<float>((size_t)S*kEnergyParts);
	for (CallSet &cs : callSets.sets) {
		cs.inSamples = devAlloc<int>(S);
		cs.outSamples = devAlloc<int>(S);
		cs.flags = devAlloc<int>(S);
		cs.hInSamples = pinnedAlloc<int>(S);
		cs.hOutSamples = pinnedAlloc<int>(S);
		cs.hFlags = pinnedAlloc<int>(S);
		cs.hEnergy = pinnedAlloc<float>((size_t)S*kEnergyParts);
		cs.resetBits = devAlloc<int>(S);
		cs.hResetBits = pinnedAlloc<int>(S);
		if (split) {
			cs.pendHops = devAlloc<HopDesc>(S);
			cs.hPendHops = pinnedAlloc<HopDesc>(S);
		}
	}
	for (StageSet &t : stageSets.sets) {
		t.host = pinnedAlloc<int>((size_t)kStageColumns*S);
		t.dev = devAlloc<int>((size_t)kStageColumns*S);
		t.hEnergy = pinnedAlloc<float>((size_t)S*kEnergyParts);
	}
	dSeedWp = devAlloc<float>(d.carryLen);
	SMST_HIP(hipMemcpy(dSeedWp, seedCarryWp.data(), d.carryLen*sizeof(float), hipMemcpyHostToDevice));
	hopFirst.assign(S, 0);
	hopCount.assign(S, 0);
	leavesPendingV.assign(S, 0);
	ridesV.assign(S, 0);
	dInSamples = callSets.sets[0].inSamples;
	dOutSamples = callSets.sets[0].outSamples;
	dFlags = callSets.sets[0].flags;
	for (std::vector<int> *v : {&flushV.blockOut, &flushV.blockIn, &flushV.synthChannels, &outputSeekV.seekSamples, &outputSeekV.surplus, &outputSeekV.preOut, &outputSeekV.done,
	                            &exactV.seekLen, &exactV.rest, &exactV.procOut, &exactV.flushN, &exactV.frames, &exactV.render}) v->assign(S, 0);
	resampleSlot.assign(S, -1);
	streamResampleSlot.assign(S, -1);
	outResampleSlot.assign(S, -1);
	streamOutResampleSlot.assign(S, -1);
	for (std::vector<unsigned char> *v : {&flushV.runBlock, &flushV.on, &outputSeekV.mask, &exactV.run}) v->assign(S, 0);
	outputSeekV.rates.assign(S, 1.0);
	exactV.rates.assign(S, 0.0f);
}

void Batch::initHostRows(long seed) {
	sched.assign(S, StreamSched());
	lastHop.assign(S, LastHop());
	// std::default_random_engine (libstdc++: minstd_rand0) of a reference instance constructed with seed + s (:39; smst_kernels_common.h: engineDraw)
	for (int s = 0; s < S; ++s) {
		const unsigned long long u = (unsigned long long)(seed + s); // `long` -> the engine's unsigned 64-bit result_type
		sched[s].seed = unsigned(u % kEngineModulus);
		if (sched[s].seed == 0) sched[s].seed = 1;
	}
	StreamParams p{};
	p.freqMultiplier = 1; p.freqTonalityLimit = 0.5f; // :513
	p.formantMultiplier = 1; p.invFormantMultiplier = 1; p.formantBaseFreq = 0; p.formantCompensation = 0; p.hasCustomMap = 0;
	params.assign(S, p);
	paramsDirty = true;
	pend.assign(S, PendingBlock());
	lastSteps.assign(S, 0);
	lastStarts.assign(S, 0);
	histBase.assign(S, 0);
	carryBase.assign(S, 0);
}

void Batch::allocateSplitTables() { // the block in flight: its spectra, and the tables of the run that completes it
	if (!split) return;
	allocateCarried(kPendIn, kCarriedArrays);
	const int nSub = (S + subS - 1)/subS;
	pendSets.create();
	for (PendSet &ps : pendSets.sets) {
		ps.hops = devAlloc<HopDesc>(S + kTileHops); ps.hHops = pinnedAlloc<HopDesc>(S); // (+ a tile's worth: the wavefront kernels cache a blind row of 64 descriptors per stream, hopStride 1)
		SMST_HIP(hipMemset(ps.hops, 0, (size_t)(S + kTileHops)*sizeof(HopDesc)));
		ps.emit = devAlloc<EmitDesc>(S); ps.hEmit = pinnedAlloc<EmitDesc>(S);
		ps.tileInfo = devAlloc<int>((size_t)nSub*2*subS); ps.hTileInfo = pinnedAlloc<int>((size_t)nSub*2*subS);
		ps.bits = devAlloc<int>(S); ps.hBits = pinnedAlloc<int>(S);
		ps.synthChannels = devAlloc<int>(S); ps.hSynthChannels = pinnedAlloc<int>(S);
		for (int j = 0; j < 3; ++j) { ps.prm[j] = devAlloc<StreamParams>(S); ps.hPrm[j] = pinnedAlloc<StreamParams>(S); }
	}
	dZeroCounts = devAlloc<int>(S);
	SMST_HIP(hipMemset(dZeroCounts, 0, S*sizeof(int)));
	pendList.reserve(S);
	pendTileHas.assign(nSub, TileSummary{});
	pendMaxSpan.assign(nSub, 0);
}

Batch::~Batch() { releaseAll(); }

void Batch::releaseAll() {
	hipSetDevice(dev);
	if (st) hipStreamSynchronize(st);
	if (stChain) hipStreamSynchronize(stChain);
	if (stSynth) hipStreamSynchronize(stSynth);
	if (stGate) hipStreamSynchronize(stGate);
	for (auto &e : livePool) { hipEventDestroy(e.first); hipEventDestroy(e.second); }
	livePool.clear();
	liveEvents.clear();
	for (void *p : allocations) hipFree(p);
	allocations.clear();
	for (void *p : pinned) hipHostFree(p);
	pinned.clear();
	if (evStart) hipEventDestroy(evStart);
	if (evOrder) hipEventDestroy(evOrder);
	evStart = evOrder = nullptr;
	for (int i = 0; i < 3; ++i) {
		if (evFeed[i]) hipEventDestroy(evFeed[i]);
		if (evChain[i]) hipEventDestroy(evChain[i]);
		if (evOut[i]) hipEventDestroy(evOut[i]);
		if (evSynth[i]) hipEventDestroy(evSynth[i]);
		evFeed[i] = evChain[i] = evOut[i] = evSynth[i] = nullptr;
	}
	if (stGate) hipStreamDestroy(stGate);
	if (stChain) hipStreamDestroy(stChain);
	if (stSynth) hipStreamDestroy(stSynth);
	if (st) hipStreamDestroy(st);
	st = stChain = stSynth = stGate = nullptr;
}

void Batch::allocateWorkspace() {
	// Per (stream, hop, channel): 3 complex rows + 1 float4 row of M bins + one B-sample frame, plus (3-8 channels only) the
	// skewed records and (SMST_FEED_SERIAL only) the serial feed's scratch.  Sub-batch the streams so one tile workspace
	// stays under a budget.  Default: a third of the HBM that is free when the batch is created, per workspace (there are
	// two), at most 96 GiB and never more than 40 % of what is free -- fewer, larger sub-batches keep the one-wave-per-stream
	// kernels of the 3-8 channel path at more than one wave per CU (config 5: 2 sub-batches instead of 7).  If an
	// allocation still fails (another batch or torch took the memory meanwhile) the sub-batch is halved and tried again.
	double budgetGiB = 24;
	{
		size_t freeB = 0, totalB = 0;
		if (hipMemGetInfo(&freeB, &totalB) == hipSuccess && freeB > 0) {
			const double freeGiB = double(freeB)/(1024.0*1024.0*1024.0);
			budgetGiB = std::min(std::min(96.0, std::max(8.0, freeGiB/3.0)), 0.4*freeGiB);
		}
	}
	if (workspaceGiB > 0) budgetGiB = std::max(0.0005, workspaceGiB); // SMST_WORKSPACE_GIB (smst_switches.h)
	const bool needRecords = formReachable(d, formSwitches, RecurrenceKernel::CHAIN_UNFUSED); // the fused recurrence keeps its records in LDS
	const size_t recChunks = (size_t(recordFloats(C)) + 3)/4;
	d.recSteps = ((M + d.lag*(d.T - 1) + 63)/64)*64 + 8;
	d.recPitch = int(recChunks*64 + 16);
	d.Mp = (M + 32 + 15) & ~15; // rows start on 128-byte lines (the recurrence's writer stores aligned 64-byte groups)
	const size_t perStream = (size_t)d.T*((size_t)C*((size_t)d.Mp*(3*sizeof(float2) + sizeof(PredEntry)) + (size_t)B*sizeof(float))
	                                      + (size_t)M*(sizeof(float2) + sizeof(float)) + 3*sizeof(float))
	                         + (size_t)C*64*sizeof(float2)
	                         + (needRecords ? (size_t)d.recSteps*d.recPitch*sizeof(float4) : 0)
	                         + (d.feedSerial ? (size_t)M*64*2*sizeof(float) + (size_t)(M/2 + 2)*64*sizeof(float2) : 0);
	size_t maxStreams = size_t(budgetGiB*1024.0*1024.0*1024.0/double(perStream));
	if (maxStreams < 1) maxStreams = 1;
	subS = int(std::min<size_t>(S, maxStreams));
	if (subStreamsAsked > 0) subS = std::min(subS, subStreamsAsked);
	for (;;) {
		const size_t mark = allocations.size();
		try {
			const size_t rows = (size_t)subS*d.T*C*d.Mp;
			// two complete tile workspaces: tile i+1's feed-forward kernels run while tile i is still in the recurrence /
			// synthesis (the budget above is per workspace)
			for (int i = 0; i < 2; ++i) {
				TileBuffers &w = slots[i];
				w = TileBuffers{};
				w.Xcur = devAlloc<float2>(rows);
				w.Xprev = devAlloc<float2>(rows);
				w.PE = devAlloc<PredEntry>(rows + 2); // (+2 entries: PrevEnergy::at reads 8 bytes at an entry's third float)
				w.OUT = devAlloc<float2>(rows);
				if (needRecords) {
					w.REC = devAlloc<float4>((size_t)subS*d.recSteps*d.recPitch);
					SMST_HIP(hipMemset(w.REC, 0, (size_t)subS*d.recSteps*d.recPitch*sizeof(float4)));
				}
				w.dump = devAlloc<float2>((size_t)subS*C*64);
				w.map = devAlloc<float2>((size_t)subS*d.T*M);
				w.ratio = devAlloc<float>((size_t)subS*d.T*M);
				if (d.noFeedFusion) w.envelope = devAlloc<float>((size_t)subS*d.T*M); // (test hook: smst_batch_debug_get_formants)
				if (d.feedSerial) {
					w.energyT = devAlloc<float>((size_t)subS*M*64);
					w.smoothT = devAlloc<float>((size_t)subS*M*64);
					w.peaksT = devAlloc<float2>((size_t)subS*(M/2 + 2)*64);
				}
				w.est = devAlloc<float>((size_t)subS*d.T*2);
				w.freqEst = devAlloc<float>((size_t)subS*d.T);
				w.frames = devAlloc<float>((size_t)subS*d.T*C*B);
				if (fftNeedsScratch(M)) w.fftScratch = devAlloc<float2>(rows); // (the synthesis frames' second FFT buffer: smst_device.h)
			}
			// The continuous wavefront (kVocoderCont) finishes tile t in launch t+1, so tile t+1's analysis needs a third place to write to:
			// the spectra, the results and the frames of a PLAIN tile only, and only where that form can run at all (one sub-batch)
			slots[2] = TileBuffers{};
			dContSave = nullptr;
			if (formReachable(d, formSwitches, RecurrenceKernel::CONTINUOUS) && subS == S) {
				TileBuffers &w = slots[2];
				w.Xcur = devAlloc<float2>(rows);
				w.Xprev = devAlloc<float2>(rows);
				w.OUT = devAlloc<float2>(rows);
				w.frames = devAlloc<float>((size_t)subS*d.T*C*B);
				if (fftNeedsScratch(M)) w.fftScratch = devAlloc<float2>(rows);
				dContSave = devAlloc<float2>((size_t)S*8*C*64);
			}
			break;
		} catch (const Error &) {
			while (allocations.size() > mark) { hipFree(allocations.back()); allocations.pop_back(); }
			(void)hipGetLastError();
			if (subS <= 1) throw;
			subS = (subS + 1)/2;
		}
	}
	wsBytes = 2*perStream*subS + (slots[2].Xcur ? (size_t)subS*d.T*C*((size_t)d.Mp*3*sizeof(float2) + (size_t)B*sizeof(float)) : 0);
}

void Batch::uploadParams() {
	if (!paramsDirty) return;
	std::copy(params.begin(), params.end(), hParams); // (pinned; the synchronise below makes it free to rewrite)
	SMST_HIP(hipMemcpyAsync(dParams, hParams, S*sizeof(StreamParams), hipMemcpyHostToDevice, st));
	SMST_HIP(hipStreamSynchronize(st));
	paramsDirty = false;
}

// The kernels outside the tile pipeline (flush tail, pre-roll, the reset that keeps the samples of a split interval, the debug accessors) index
// the overlap-add carry from the front of its rows: a call without hops may have left the windows further in (kEmitCarried) -- one
// emission of nothing moves them back.
void Batch::settleCarry() {
	bool moved = false;
	for (int s = 0; s < S && !moved; ++s) moved = carryBase[s] != 0;
	if (!moved) return;
	DevBatch dd = d;
	dd.emit = dZeroEmit;
	dd.emitStride = 1;
	const IoArgs io{nullptr, nullptr, 0, 0, 0, 0, nullptr, nullptr};
	launchEmit(dd, io, 0, S, 0, 0, st);
	d.carryCur ^= 1;
	std::fill(carryBase.begin(), carryBase.end(), 0);
}

void Batch::uploadStage(const StageSet &t, int columns) { // a stage's ONE upload: its columns are contiguous
	SMST_HIP(hipMemcpyAsync(t.dev, t.host, (size_t)columns*S*sizeof(int), hipMemcpyHostToDevice, st));
}

// stft.reset(0.1) / Band clearing for the streams that pick(s) names (bit masks, see kResetStreams): one upload + one launch, instead of
// six API calls per stream.  A stage set of its own turn: column 0 the masks, column 1 (keepAhead: flush() with split computation) how many
// samples of the stashed ring each stream keeps -- what is left of its interval.
template <typename Pick> void Batch::resetStreams(Pick pick, int bits, bool keepAhead) {
	if (keepAhead) settleCarry();
	StageSet &t = stageSets.begin();
	int *mask = t.host, *keep = t.host + S;
	for (int s = 0; s < S; ++s) {
		mask[s] = pick(s) ? bits : 0;
		keep[s] = (mask[s] && keepAhead) ? aheadOffset(s) : 0;
		if (mask[s] & RESET_STFT) histBase[s] = carryBase[s] = 0; // (the host's copies of DevBatch::histBase / carryBase)
	}
	uploadStage(t, keepAhead ? 2 : 1);
	launchResetStreams(d, t.dev, 0, dSeedWp, st, keepAhead ? t.dev + S : nullptr);
	stageSets.end(st);
}

void Batch::reset() { // signalsmith-stretch.h:49-60
	SMST_HIP(hipSetDevice(dev));
	const CarriedArray freq = carriedArrays()[kStFreq];
	SMST_HIP(hipMemsetAsync(freq.current(), 0, (size_t)S*freq.rowBytes, st));
	launchResetStreams(d, nullptr, RESET_STFT | RESET_INPUT | RESET_PREV | RESET_OUTPUT, dSeedWp, st); // (every stream: no table)
	std::fill(histBase.begin(), histBase.end(), 0);
	std::fill(carryBase.begin(), carryBase.end(), 0);
	d.histCur = 0;
	d.carryCur = 0;
	for (int s = 0; s < S; ++s) clearHostRow(s);
}
void Batch::clearHostRow(int s) { // (histBase / carryBase: resetStreams)
	const unsigned seed = seedAfterDroppedBlock(s); // reset() leaves the reference's randomEngine alone; a block in flight is dropped with the draws it has made
	pend[s] = PendingBlock(); // blockProcess = {}
	sched[s] = StreamSched();
	sched[s].seed = seed;
	lastHop[s] = LastHop();
	lastSteps[s] = 0;
	lastStarts[s] = 0;
}
void Batch::takeHostRow(const Batch &o, int from, int to) {
	sched[to] = o.sched[from];
	params[to] = o.params[from];
	pend[to] = o.pend[from];
	lastSteps[to] = o.lastSteps[from]; // smst_block_steps of a clone = the original's newest block
	lastStarts[to] = o.lastStarts[from];
	histBase[to] = o.histBase[from];
	carryBase[to] = o.carryBase[from];
	lastHop[to] = LastHop();
	paramsDirty = true;
}

template <typename Pick> void Batch::resetPicked(Pick pick) { // reset() for the picked streams; kResetStreams writes both halves of the double buffers, so which half is current does not matter
	SMST_HIP(hipSetDevice(dev));
	SMST_HIP(hipStreamSynchronize(st)); // (orders nothing that the masks need any more -- their set's event does; kept: EXPERIMENTS.md, "One per-call table set")
	resetStreams(pick, RESET_STFT | RESET_INPUT | RESET_PREV | RESET_OUTPUT | RESET_FREQ);
	for (int s = 0; s < S; ++s) if (pick(s)) clearHostRow(s);
}
void Batch::resetStream(int s) { // reset() for one stream
	if (s < 0 || s >= S) throw Error("stream index out of range");
	resetPicked([s](int t) { return t == s; });
}
void Batch::resetStreamsMasked(const unsigned char *active) { resetPicked([active](int s) { return active[s] != 0; }); }

// ---- parameters ------------------------------------------------------------------------------------------
template <typename F> static void forStreams(int S, int stream, F &&f) {
	if (stream < 0) { for (int s = 0; s < S; ++s) f(s); }
	else if (stream < S) f(stream);
	else throw Error("stream index out of range");
}
void Batch::setTransposeFactor(int stream, float multiplier, float tonalityLimit) { // :107-115
	forStreams(S, stream, [&](int s) {
		freezePendingParams(s);
		params[s].freqMultiplier = multiplier;
		params[s].freqTonalityLimit = (tonalityLimit > 0) ? tonalityLimit/std::sqrt(multiplier) : 1.0f;
		params[s].hasCustomMap = 0;
	});
	paramsDirty = true;
}
void Batch::setTransposeSemitones(int stream, float semitones, float tonalityLimit) { // :116-118
	setTransposeFactor(stream, float(std::pow(2, semitones/12)), tonalityLimit);
}
void Batch::setFormantFactor(int stream, float multiplier, bool compensatePitch) { // :124-128
	forStreams(S, stream, [&](int s) {
		freezePendingParams(s);
		params[s].formantMultiplier = multiplier;
		params[s].invFormantMultiplier = 1/multiplier;
		params[s].formantCompensation = compensatePitch ? 1 : 0;
	});
	paramsDirty = true;
}
void Batch::setFormantSemitones(int stream, float semitones, bool compensatePitch) { // :129-131
	setFormantFactor(stream, float(std::pow(2, semitones/12)), compensatePitch);
}
void Batch::setFormantBase(int stream, float baseFreq) { // :133-135
	forStreams(S, stream, [&](int s) { freezePendingParams(s); params[s].formantBaseFreq = baseFreq; });
	paramsDirty = true;
}
void Batch::setFreqMapTable(int stream, const float *table, int n) { // table form of :120-122
	// Split computation: the steps of a block in flight that have already run keep the map they saw -- flag, length AND knots: every stream
	// has kMapSlots table rows, StreamParams.mapSlot names the live one, and a new table goes to a row that neither findPeaks' (:874) nor
	// updateFormants step 2's (:1020) latched parameters of the block in flight refer to (freezePendingParams).  The reference replaces its
	// std::function as a whole (:120-122): a step that ran before the call evaluated the old function, a step that runs after it the new one.
	forStreams(S, stream, [&](int s) { freezePendingParams(s); });
	if (n <= 0 || !table) {
		forStreams(S, stream, [&](int s) { params[s].hasCustomMap = 0; });
		paramsDirty = true;
		return;
	}
	if (n < 2) throw Error("frequency-map table needs at least 2 points");
	if (stream >= S) throw Error("stream index out of range");
	SMST_HIP(hipSetDevice(dev));
	// Every stream keeps ITS OWN table, knot for knot (StreamParams.mapLen points, linear between them, extrapolated beyond: the
	// reference evaluates each instance's own function, :874, :1020); the batch's array only has one row pitch, the longest table
	// seen so far -- a longer table makes the array grow and the existing rows are copied as they are.  (Rounds 2-3 re-evaluated the
	// stored rows on the longer table's grid, which cuts the corner at every old knot: a stream's map could change because ANOTHER
	// stream was given a longer table.)  When no stream holds a table any more the next one starts afresh.
	auto latched = [&](int s, int slot) { // a step of the stream's block in flight ran with the table in this row
		if (!split || !pend[s].valid) return false;
		const PendingBlock &pb = pend[s];
		return (pb.frozenPeaks && pb.peaks.hasCustomMap && pb.peaks.mapSlot == slot) || (pb.frozenForm2 && pb.form2.hasCustomMap && pb.form2.mapSlot == slot);
	};
	bool anyCustom = false;
	for (int s = 0; s < S; ++s) {
		anyCustom = anyCustom || params[s].hasCustomMap;
		for (int slot = 0; slot < kMapSlots; ++slot) anyCustom = anyCustom || latched(s, slot);
	}
	if (!anyCustom) d.mapTableLen = 0;
	if (n > d.mapTableLen) {
		SMST_HIP(hipStreamSynchronize(st)); // kernels of earlier calls may still read the old array
		growMapTable(n);
	}
	const int pitch = d.mapTableLen;
	forStreams(S, stream, [&](int s) {
		int slot = 0;
		while (slot < kMapSlots - 1 && latched(s, slot)) ++slot; // at most two rows are latched: one is always free
		std::copy(table, table + n, hostMapTable.begin() + ((size_t)s*kMapSlots + slot)*pitch);
		params[s].hasCustomMap = 1;
		params[s].mapLen = n;
		params[s].mapSlot = slot;
	});
	SMST_HIP(hipStreamSynchronize(st)); // kernels of earlier calls may still read the old table
	uploadMapTable();
	paramsDirty = true;
}
// hostMapTable is [S][kMapSlots][d.mapTableLen] throughout; the caller has synchronised `st` (the old array is freed)
void Batch::growMapTable(int pitch) {
	const size_t rows = (size_t)S*kMapSlots, have = (size_t)d.mapTableLen;
	std::vector<float> grown(rows*pitch, 0.0f);
	for (size_t row = 0; row < rows && have > 0; ++row) // (rows that hold no table are zeros either way)
		std::copy(hostMapTable.begin() + row*have, hostMapTable.begin() + (row + 1)*have, grown.begin() + row*pitch);
	if (dMapTable) devFree(dMapTable);
	dMapTable = devAlloc<float>(grown.size());
	hostMapTable.swap(grown);
	d.mapTableLen = pitch;
	d.mapTable = dMapTable;
}
void Batch::uploadMapTable() {
	SMST_HIP(hipMemcpy(dMapTable, hostMapTable.data(), hostMapTable.size()*sizeof(float), hipMemcpyHostToDevice));
}

void Batch::checkLaunch(const char *what) {
	if (!checkLaunches) return;
	const hipError_t e = hipGetLastError();
	if (e != hipSuccess) throw Error(std::string("launch failed (") + what + "): " + hipGetErrorString(e), true);
}

template <typename F> void Batch::timed(double &acc, F &&f) {
	if (!profiling) { f(); return; }
	hipEvent_t a, b;
	SMST_HIP(hipEventCreate(&a));
	SMST_HIP(hipEventCreate(&b));
	SMST_HIP(hipEventRecord(a, st));
	f();
	SMST_HIP(hipEventRecord(b, st));
	SMST_HIP(hipEventSynchronize(b));
	float ms = 0;
	SMST_HIP(hipEventElapsedTime(&ms, a, b));
	acc += ms;
	hipEventDestroy(a);
	hipEventDestroy(b);
}
void Batch::growLivePool(size_t pairs) {
	// timing events WITHOUT the default system-scope fences: those drain and flush at every record and slowed the
	// recurrence from 1.2 to 1.7 ms per launch (and the step by 7 %)
	while (livePool.size() < pairs) {
		hipEvent_t a = nullptr, b = nullptr;
		SMST_HIP(hipEventCreateWithFlags(&a, hipEventDisableSystemFence));
		SMST_HIP(hipEventCreateWithFlags(&b, hipEventDisableSystemFence));
		livePool.emplace_back(a, b);
	}
}
void Batch::enableProfiling(int mode) {
	profiling = mode == 1;
	liveTiming = mode == 2;
	if (liveTiming) {
		SMST_HIP(hipSetDevice(dev));
		growLivePool(1024); // 128 steps of the headline workload between two takeTimings(): no event is created inside process()
	}
}
BatchTimings Batch::takeTimings() {
	if (!liveEvents.empty()) {
		SMST_HIP(hipSetDevice(dev));
		SMST_HIP(hipStreamSynchronize(st));
		for (auto &e : liveEvents) {
			float ms = 0;
			SMST_HIP(hipEventElapsedTime(&ms, e.first, e.second));
			timings.chainLiveMs += ms;
			++timings.chainLiveLaunches;
		}
		liveEvents.clear(); // the pairs go back to the pool
	}
	BatchTimings t = timings;
	timings = BatchTimings();
	return t;
}
void Batch::synchronize() {
	SMST_HIP(hipSetDevice(dev));
	SMST_HIP(hipStreamSynchronize(st));
}

// ---- process ----------------------------------------------------------------------------------------------
template <typename T> static void ensureSize(std::vector<T> &v, size_t n, long &events) {
	if (n > v.capacity()) ++events;
	v.resize(n);
}

void Batch::waitForStream(hipStream_t other) {
	SMST_HIP(hipSetDevice(dev));
	SMST_HIP(hipEventRecord(evOrder, other));
	SMST_HIP(hipStreamWaitEvent(st, evOrder, 0));
	SMST_HIP(hipStreamWaitEvent(stGate, evOrder, 0));
}
void Batch::signalStream(hipStream_t other) {
	SMST_HIP(hipSetDevice(dev));
	SMST_HIP(hipEventRecord(evOrder, st));
	SMST_HIP(hipStreamWaitEvent(other, evOrder, 0));
}

// ---- split computation: the reference's step schedule -----------------------------------------------------
StepLayout Batch::stepLayout(unsigned flags) const { // the order of signalsmith-stretch.h:332-400 / :642-812, counted as :304-318 / :620-632 count it
	StepLayout l;
	int i = 0;
	const bool nw = (flags & HOP_NEW_SPECTRUM) != 0;
	if (nw) {
		if (flags & HOP_REANALYSE_PREV) { l.reanalyse0 = i; i += C + 1; } // analyseSteps() = one per channel (pinned by tests/golden/split_events), + the copy
		l.analyse0 = i; i += C;
		l.copyIn = i; i += 1;
		i += C; // rotation
	}
	if (flags & HOP_MAPPED) { i += 3; l.peaks = i; i += 1; } // smoothEnergy x 3, findPeaks
	i += 1;                                                   // output map
	if (flags & HOP_FORMANTS) { l.form0 = i; l.form2 = i + 2; i += 3; }
	i += C;                                                   // preliminary prediction
	l.main0 = i; i += 8;                                     // splitMainPrediction
	if (nw) { l.prevCopy = i; i += 1; }
	l.spectrum = i; i += 1;
	l.synth0 = i; i += C;                                     // synthesiseSteps() = one per channel, the first adds the window product
	l.steps = i;
	return l;
}
size_t Batch::stepsExecuted(size_t steps, size_t k) const { // after k samples of the interval, :321-325 (fp32 as there)
	const float processRatio = float(k)/float(size_t(I));
	return std::min<size_t>(steps, size_t((float(steps) + 0.999f)*processRatio));
}
// The random engine and the block in flight (:616, :749, :769): a block beyond 2x draws its 2M - 2 time factors inside the chunks of the main
// prediction, in bin order, WHEN those chunks run.  So the stream's engine moves on by a whole block when the block in flight finally runs, and
// -- if reset(), a silent call or configure() drops it (blockProcess = {}) -- by the draws of the chunks that had run by then only.
static unsigned lcgPower(unsigned long long n) { // 16807^n mod (2^31 - 1)
	unsigned long long r = 1, b = 16807;
	while (n) {
		if (n & 1) r = r*b % kEngineModulus;
		b = b*b % kEngineModulus;
		n >>= 1;
	}
	return unsigned(r);
}
unsigned Batch::seedAfterDroppedBlock(int s) const {
	const PendingBlock &pb = pend[s];
	const unsigned seed = sched[s].seed;
	if (!split || !pb.valid || !(pb.flags & HOP_RANDOM_TF)) return seed;
	const StepLayout l = stepLayout(pb.flags);
	const size_t e = stepsExecuted(size_t(l.steps), sched[s].samplesSinceLast);
	const size_t chunks = e > size_t(l.main0) ? std::min<size_t>(8, e - size_t(l.main0)) : 0;
	const size_t b0 = size_t(M)*chunks/8; // bins [0, b0) have drawn: one draw per bin for b > 0, one for b < M - 1
	if (b0 == 0) return seed;
	const unsigned long long draws = (b0 >= size_t(M)) ? 2ull*M - 2 : 2ull*b0 - 1;
	return unsigned((unsigned long long)seed*lcgPower(draws) % kEngineModulus);
}
unsigned Batch::advanceOneHop(unsigned seed) const { return unsigned((unsigned long long)seed*lcgHopJump % kEngineModulus); }

// A setter is about to change params[s]: the steps of the block in flight that have already run saw the OLD values (:874, :982, :1020)
void Batch::freezePendingParams(int s) {
	if (!split) return;
	PendingBlock &pb = pend[s];
	if (!pb.valid) return;
	const StepLayout l = stepLayout(pb.flags);
	const size_t e = stepsExecuted(size_t(l.steps), sched[s].samplesSinceLast);
	if (l.peaks >= 0 && e > size_t(l.peaks) && !pb.frozenPeaks) { pb.peaks = params[s]; pb.frozenPeaks = true; }
	if (l.form0 >= 0 && e > size_t(l.form0) && !pb.frozenForm0) { pb.form0 = params[s]; pb.frozenForm0 = true; }
	if (l.form2 >= 0 && e > size_t(l.form2) && !pb.frozenForm2) { pb.form2 = params[s]; pb.frozenForm2 = true; }
}

// The block in flight of stream s as the hop that completes it: its spectra come from the pending buffers, and its frame lands where its
// interval ends -- it began samplesSinceLast samples ago (outPos < 0; split computation delays every frame by one interval, :292-296)
void Batch::pendingHop(int s, HopDesc &hd) const {
	const PendingBlock &pb = pend[s];
	hd.flags = pb.flags | HOP_PREANALYSED;
	hd.timeFactor = pb.timeFactor;
	hd.seed = pb.seed;
	hd.startBin = pb.startBin; // (> 0 only in runPendingBlocks(): gateAndCount() sends such a block there; one that rides as a call's hop 0 has 0)
	hd.outPos = -int(sched[s].samplesSinceLast);
	const bool nw = (pb.flags & HOP_NEW_SPECTRUM) != 0;
	hd.inSrc = nw ? 0 : SRC_STATE;
	hd.prevSrc = (nw && (pb.flags & HOP_REANALYSE_PREV)) ? SRC_REANALYSED : SRC_STATE;
}
void Batch::noteLastHop(int s, int slot, int local, unsigned flags) { // where the stream's newest hop sits in the tile workspaces (debugGetMap)
	lastHop[s] = LastHop{slot, local, s%subS, (flags & HOP_MAPPED) != 0, (flags & HOP_FORMANTS) != 0};
}

// The blocks in flight of the streams in `pendList` run to their end: one tile of one hop per stream whose spectra come from the
// pending buffers; it consumes no input and emits no sample -- the frame goes into the overlap-add ring at the point where the block's
// interval ends (outPos = -samples since the block began; split computation delays every frame by one interval, :292-296).
// synthChannels (host, per stream, may be null): a flush() caught the block between two synthesis steps (:397-399).
void Batch::runPendingBlocks(const int *synthChannels) {
	if (pendList.empty()) return;
	uploadParams();
	PendSet &ps = pendSets.begin();
	const int nSub = (S + subS - 1)/subS;
	std::memset(ps.hHops, 0, S*sizeof(HopDesc));
	std::memset(ps.hEmit, 0, S*sizeof(EmitDesc));
	std::memset(ps.hTileInfo, 0, (size_t)nSub*2*subS*sizeof(int));
	std::fill(pendTileHas.begin(), pendTileHas.end(), TileSummary{});
	std::fill(pendMaxSpan.begin(), pendMaxSpan.end(), 0);
	bool anyFrozen = false, anyZeroPrev = false;
	for (int s : pendList) {
		const PendingBlock &pb = pend[s];
		HopDesc &hd = ps.hHops[s];
		pendingHop(s, hd);
		EmitDesc &ed = ps.hEmit[s];
		ed.firstHopPos = hd.outPos;
		ed.hopCount = 1;
		const int sub = s/subS, sl = s%subS;
		int *info = ps.hTileInfo + (size_t)sub*2*subS;
		info[sl] = 1;
		info[subS + sl] = (pb.flags & HOP_NEW_SPECTRUM) ? 0 : -1;
		TileSummary &th = pendTileHas[sub];
		th.anyHop = true;
		if (pb.flags & HOP_MAPPED) th.mapped = true;
		if (pb.flags & HOP_FORMANTS) th.formants = th.estimatesBase = true; // (a block in flight may carry latched parameters: the three-kernel form decides per stream)
		if (pb.flags & HOP_RANDOM_TF) th.randomTimeFactor = true;
		if (pb.startBin > 0) th.startBin = true;
		th.preAnalysed = true;
		anyFrozen = anyFrozen || pb.frozenPeaks || pb.frozenForm0 || pb.frozenForm2;
		anyZeroPrev = anyZeroPrev || pb.zeroPrevAfter;
		noteLastHop(s, sub & 1, 0, pb.flags);
	}
	SMST_HIP(hipMemcpyAsync(ps.hops, ps.hHops, S*sizeof(HopDesc), hipMemcpyHostToDevice, st));
	SMST_HIP(hipMemcpyAsync(ps.emit, ps.hEmit, S*sizeof(EmitDesc), hipMemcpyHostToDevice, st));
	SMST_HIP(hipMemcpyAsync(ps.tileInfo, ps.hTileInfo, (size_t)nSub*2*subS*sizeof(int), hipMemcpyHostToDevice, st));
	if (anyFrozen) { // some step of some block ran before a setter: that step keeps the values it saw
		for (int s = 0; s < S; ++s) ps.hPrm[0][s] = ps.hPrm[1][s] = ps.hPrm[2][s] = params[s];
		for (int s : pendList) {
			const PendingBlock &pb = pend[s];
			if (pb.frozenPeaks) ps.hPrm[0][s] = pb.peaks;
			if (pb.frozenForm0) ps.hPrm[1][s] = pb.form0;
			if (pb.frozenForm2) ps.hPrm[2][s] = pb.form2;
		}
		for (int j = 0; j < 3; ++j) SMST_HIP(hipMemcpyAsync(ps.prm[j], ps.hPrm[j], S*sizeof(StreamParams), hipMemcpyHostToDevice, st));
		d.paramsPeaks = ps.prm[0]; d.paramsForm0 = ps.prm[1]; d.paramsForm2 = ps.prm[2];
	}
	if (synthChannels) {
		for (int s = 0; s < S; ++s) ps.hSynthChannels[s] = -1;
		for (int s : pendList) ps.hSynthChannels[s] = synthChannels[s];
		SMST_HIP(hipMemcpyAsync(ps.synthChannels, ps.hSynthChannels, S*sizeof(int), hipMemcpyHostToDevice, st));
	}
	d.hops = ps.hops;
	d.emit = ps.emit;
	d.hopStride = 1;
	d.emitStride = 1;
	const IoArgs io{nullptr, nullptr, 0, 0, 0, 0, dZeroCounts, dZeroCounts};
	runTiles(TileRun{&io, 1, 1, pendTileHas.data(), pendMaxSpan.data(), ps.tileInfo, true, synthChannels ? ps.synthChannels : nullptr, false});
	d.paramsPeaks = d.paramsForm0 = d.paramsForm2 = dParams;
	if (anyZeroPrev) {
		for (int s = 0; s < S; ++s) ps.hBits[s] = 0;
		for (int s : pendList) if (pend[s].zeroPrevAfter) ps.hBits[s] = RESET_PREV;
		SMST_HIP(hipMemcpyAsync(ps.bits, ps.hBits, S*sizeof(int), hipMemcpyHostToDevice, st));
		launchResetStreams(d, ps.bits, 0, dSeedWp, st);
	}
	pendSets.end(st);
	for (int s : pendList) {
		if (pend[s].flags & HOP_RANDOM_TF) sched[s].seed = advanceOneHop(sched[s].seed); // its draws happen now
		pend[s] = PendingBlock();
	}
	pendList.clear();
}

// The tiles of a call (or of a run of blocks in flight): analysis, feed-forward passes, recurrence, synthesis and emission, pipelined
// over three HIP streams and two workspaces.
void Batch::runTiles(const TileRun &run) {
	const IoArgs &io = *run.io;
	const int nTiles = run.nTiles;
	if (run.carriedOnly) { // no stream fires a hop: the front of the carry is the output, and what is left stays where it is
		timed(timings.emitMs, [&] { launchEmitCarried(d, io, st); if (profiling) ++timings.emitLaunches; });
		checkLaunch("emission of the carried sums");
		return;
	}
	std::fill(carryBase.begin(), carryBase.end(), 0); // every tile writes every stream's carry from the front of its rows
	const int carryFirst = d.carryCur;
	// Runs of two or more tiles that the continuous wavefront can take (kVocoderCont) go to it, the tiles around them -- the first tile
	// after a reset, whose first hop draws random time factors; a tile with a pitch map -- tile by tile; the segments follow each other on `st`.
	int t = 0;
	while (t < nTiles) {
		int e = t;
		while (e < nTiles && continuousApplies(run, e)) ++e;
		if (e - t >= 2) { runTilesContinuous(run, t, e, carryFirst); t = e; continue; }
		e = std::max(e, t + 1);
		for (;;) { // extend the tile-by-tile segment up to the next run of two
			int r = e;
			while (r < nTiles && continuousApplies(run, r)) ++r;
			if (e >= nTiles || r - e >= 2) break;
			e = std::max(r, e + 1);
		}
		runTilesRange(run, t, e, carryFirst);
		t = e;
	}
	d.carryCur = (carryFirst + nTiles) & 1;
}

// A segment of tiles begins: its three streams (all `st` when the run is serial), forked from what is already queued on `st`
Batch::TileStreams Batch::forkTileStreams(const TileRun &run) {
	const bool serial = profiling || !overlap || run.pendingRun;
	const TileStreams ts{serial, st, serial ? st : stChain, serial ? st : stSynth};
	if (!serial) {
		SMST_HIP(hipEventRecord(evStart, st));
		SMST_HIP(hipStreamWaitEvent(ts.sC, evStart, 0));
		SMST_HIP(hipStreamWaitEvent(ts.sS, evStart, 0));
	}
	return ts;
}
// ... and ends: everything the caller can observe is ordered on `st` again -- `passes` tile passes over a ring of `depth` workspaces, from slot first % depth on
void Batch::joinTileStreams(const TileStreams &ts, int first, int passes, int depth) {
	if (ts.serial) return;
	for (int i = 0; i < depth && i < passes; ++i) { // join the slots the segment used: (first + i) % depth, not i
		SMST_HIP(hipStreamWaitEvent(st, evChain[(first + i)%depth], 0));
		SMST_HIP(hipStreamWaitEvent(st, evSynth[(first + i)%depth], 0));
	}
}
// The recurrence launch of a tile, timed as its class -- and in place, between two events on its own stream, where live timing is on
template <typename F> void Batch::timedRecurrence(const TileStreams &ts, F &&launch) {
	const bool live = liveTiming && !ts.serial;
	if (live) {
		if (liveEvents.size() == livePool.size()) growLivePool(livePool.size() + 64); // only if a run outgrows what enableProfiling() made
		SMST_HIP(hipEventRecord(livePool[liveEvents.size()].first, ts.sC));
	}
	timed(timings.chainMs, [&] { launch(); if (profiling) ++timings.chainLaunches; });
	if (live) {
		SMST_HIP(hipEventRecord(livePool[liveEvents.size()].second, ts.sC));
		liveEvents.push_back(livePool[liveEvents.size()]);
	}
}
// The batch as the kernels of one tile see it: the tile's workspace, the half of the carry it writes, its rows of the tile-info table
DevBatch Batch::tileView(const TileBuffers &w, int carryCur, const int *tileInfo) const {
	DevBatch dd = d;
	dd.Xcur = w.Xcur; dd.Xprev = w.Xprev; dd.PE = w.PE; dd.OUT = w.OUT; dd.REC = w.REC; dd.dump = w.dump;
	dd.map = w.map; dd.ratio = w.ratio; dd.envelope = w.envelope; dd.energyT = w.energyT; dd.smoothT = w.smoothT; dd.peaksT = w.peaksT; dd.est = w.est; dd.freqEst = w.freqEst; dd.frames = w.frames; dd.fftScratch = w.fftScratch;
	dd.carryCur = carryCur;
	dd.nHops = tileInfo; dd.lastNewHop = tileInfo + subS;
	return dd;
}

void Batch::runTilesRange(const TileRun &run, int tile0, int tile1, int carryFirst) {
	const IoArgs &io = *run.io;
	const int T = d.T, nTiles = run.nTiles, maxHops = run.maxHops;
	const int nSub = (S + subS - 1)/subS;
	// Three HIP streams: `st` runs the feed-forward kernels of tile q, `stChain` the recurrence of tile q (a few
	// hundred waves, instruction-issue bound), `stSynth` synthesis + emission.  Two workspaces alternate, so the bulk
	// kernels of the next tile fill the machine while the recurrence of the current one is in flight.
	const TileStreams ts = forkTileStreams(run);
	int q = tile0; // (the workspace of tile t of a single sub-batch is slots[t & 1] whatever segment it runs in: debugGetMap relies on it)
	for (int sub = 0; sub < nSub; ++sub) {
		const int sBase = sub*subS;
		const int ns = std::min(subS, S - sBase);
		for (int t = tile0; t < tile1; ++t, ++q) {
			const TileSummary &th = run.tileHas[(size_t)sub*nTiles + t];
			const int hopBase = t*T;
			const int tileHops = std::min(T, std::max(1, maxHops - hopBase));
			const int slot = q & 1;
			const bool plain = th.plain();
			// which recurrence the tile takes: decided once, here (smst_recurrence_form.h).  fused: the records stay in LDS; twisted (DESIGN.md
			// section 4): the rows of Xprev hold the finished previous-hop twists, formed once per bin by the analysis pass, instead of Band.prevInput
			const RecurrenceForm form = recurrenceForm(d, th, tileHops, ns, run.pendingRun, formSwitches);
			const bool fused = form.fused();
			const DevBatch dd = tileView(slots[slot], (carryFirst + t) & 1, run.dTileInfo + ((size_t)(sub*nTiles + t)*2)*subS);
			if (!ts.serial && q - tile0 >= 2) { // this workspace was last used by tile q-2
				SMST_HIP(hipStreamWaitEvent(ts.sF, evChain[slot], 0));
				SMST_HIP(hipStreamWaitEvent(ts.sF, evSynth[slot], 0));
			}
			if (!ts.serial && fused && !plain && q - tile0 >= 1) SMST_HIP(hipStreamWaitEvent(ts.sF, evChain[slot ^ 1], 0)); // pass A reads the carried state
			if (th.anyHop) {
				if (th.preAnalysed) timed(timings.otherMs, [&] { launchPendingToTile(dd, sBase, ns, dPendIn, dPendPrev, ts.sF); }); // blocks that began in an earlier call: their spectra are waiting
				if (th.newSpectrum) timed(timings.analyseMs, [&] { launchAnalyse(dd, io, sBase, ns, hopBase, tileHops, th.windowInCall, th.windowInHistory, ts.sF, form.twisted, th.lateHops); if (profiling) ++timings.analyseLaunches; });
				bool passADone = false;
				if (!plain) timed(timings.feedMs, [&] { passADone = launchFeed(dd, sBase, ns, hopBase, tileHops, th.formants, th.estimatesBase, ts.sF); });
				timed(timings.predictMs, [&] { launchPredict(dd, fused, sBase, ns, hopBase, tileHops, plain, passADone, ts.sF); if (profiling) ++timings.predictLaunches; });
				// the carried feed-forward state (Band.input/.prevInput, Prediction.energy) may only move on once every
				// reader of the OLD state has run: in the fused path the producers inside kVocoder still read it
				if (!fused) timed(timings.otherMs, [&] { launchCarryFeed(dd, sBase, ns, hopBase, th.formants, ts.sF); });
			}
			checkLaunch("analysis / feed-forward kernels");
			if (!ts.serial) {
				SMST_HIP(hipEventRecord(evFeed[slot], ts.sF));
				SMST_HIP(hipStreamWaitEvent(ts.sC, evFeed[slot], 0));
			}
			// synthesis + overlap-add + emission in one kernel where the geometry and the batch allow it
			const bool emitted = th.anyHop && !th.preAnalysed && synthEmitApplies(dd, ns, tileHops); // (preAnalysed: a hop that began before the call's first sample -- kSynthTeams + kEmit place its frame)
			const bool earlySynth = emitted || tileHops == 1;
			if (th.anyHop) {
				timedRecurrence(ts, [&] { launchRecurrence(dd, form, sBase, ns, hopBase, plain, ts.sC); });
				// synthesis needs the recurrence's rows only: the hand-over of the tile's last rows to the carried state (two copies at HBM rate --
				// 250 us of a 4096-stream hop quantum) runs beside it, behind the event synthesis waits for.  Where synthesis is a grid of
				// per-frame workgroups and more recurrence launches follow (config 5) the hand-over goes first, as before: it is what the NEXT
				// recurrence waits for, and behind a machine full of synthesis workgroups it would start late (config 5: 99.6 -> 101 ms)
				timed(timings.otherMs, [&] {
					if (run.dSynthChannels || !earlySynth) { // (the carried output state takes the rows as the recurrence left them)
						launchCarryOut(dd, sBase, ns, ts.sC);
						if (run.dSynthChannels) launchMaskOutRows(dd, sBase, ns, run.dSynthChannels, ts.sC);
					}
					if (!earlySynth && fused) launchCarryFeed(dd, sBase, ns, hopBase, th.formants, ts.sC);
					if (!ts.serial) SMST_HIP(hipEventRecord(evOut[slot], ts.sC));
					if (earlySynth && fused) launchCarryFeed(dd, sBase, ns, hopBase, th.formants, ts.sC);
					if (earlySynth && !run.dSynthChannels) launchCarryOut(dd, sBase, ns, ts.sC);
				});
			}
			checkLaunch("bin recurrence");
			// kSynthEmitTeams' window products depend on nothing the recurrence writes: queued in front of the wait for it
			if (emitted) timed(timings.otherMs, [&] { launchEmitProducts(dd, sBase, ns, t, ts.sS); });
			if (!ts.serial) {
				SMST_HIP(hipEventRecord(evChain[slot], ts.sC));
				SMST_HIP(hipStreamWaitEvent(ts.sS, th.anyHop ? evOut[slot] : evChain[slot], 0));
			}
			if (th.anyHop) timed(timings.synthMs, [&] {
				if (emitted) launchSynthEmit(dd, io, sBase, ns, t, ts.sS);
				else launchSynth(dd, sBase, ns, hopBase, tileHops, ts.sS);
				if (profiling) ++timings.synthLaunches;
			});
			if (!emitted) timed(timings.emitMs, [&] { launchEmit(dd, io, sBase, ns, t, run.maxSpan[(size_t)sub*nTiles + t], ts.sS); if (profiling) ++timings.emitLaunches; });
			checkLaunch("synthesis / emission");
			if (!ts.serial) SMST_HIP(hipEventRecord(evSynth[slot], ts.sS));
		}
	}
	joinTileStreams(ts, tile0, q - tile0, 2); // (passes, not tiles: q runs on through the sub-batches; tile0 may be odd)
}

// Whether a tile can be part of a continuous wavefront (kVocoderCont; runs of two or more such tiles are): the third workspace exists (the
// geometry and SMST_CONTINUOUS: allocateWorkspace), one sub-batch, what the tile's hops need (TileSummary::continuousCapable) -- and tile by
// tile it would be an ALIGNED one.  Asked for a FULL tile: rows of a wavefront that does not drain are never a one-hop tile's, so a run's
// last tile rides the wavefront even where it has one hop (tile by tile it would go to the single-hop kernels).
bool Batch::continuousApplies(const TileRun &run, int t) const {
	if (!slots[2].Xcur || run.pendingRun || run.carriedOnly || subS != S) return false;
	const TileSummary &th = run.tileHas[t];
	return th.continuousCapable() && recurrenceForm(d, th, d.T, S, false, formSwitches).kernel == RecurrenceKernel::ALIGNED;
}

// The same pipeline as runTiles -- analysis of tile t+1, recurrence, synthesis + emission over three HIP streams -- with the recurrence as
// launch t of the continuous wavefront: it begins tile t and finishes tile t-1, so synthesis runs one tile later and the workspaces rotate
// over three slots (launch t reads the spectra of tiles t-1 and t while tile t+1 is analysed).  The carried state is read by launch 0 only
// (the call's first hop); it is written once per stream, from its last tile, behind the launch that finishes that tile.
void Batch::runTilesContinuous(const TileRun &run, int tile0, int tile1, int carryFirst) {
	const IoArgs &io = *run.io;
	const int T = d.T, maxHops = run.maxHops;
	const TileStreams ts = forkTileStreams(run); // (a run of blocks in flight never comes here: continuousApplies)
	const int P = continuousPeriod(d);
	auto view = [&](int t) {
		DevBatch dd = tileView(slots[t%3], (carryFirst + t) & 1, run.dTileInfo + ((size_t)t*2)*subS);
		dd.PE = nullptr; dd.REC = nullptr; dd.map = nullptr; dd.ratio = nullptr; // (plain tiles: never touched -- nor are the slot's dump / envelope / serial-feed scratch / est / freqEst that tileView hands over: no kernel of this path reads them)
		return dd;
	};
	auto tileHops = [&](int t) { return std::min(T, std::max(1, maxHops - t*T)); };
	auto lastOfSomeStream = [&](int t) {
		if (t == tile1 - 1) return true; // (the tiles behind the segment, if any, start from the carried state)
		for (int s = 0; s < S; ++s) if (hopCount[s] > 0 && (hopCount[s] - 1)/T == t) return true;
		return false;
	};
	// tile t is complete (its last rows ran in the launch just enqueued on ts.sC): hand-over to the carried state, synthesis + emission
	auto finishTile = [&](int t, int launch) {
		const DevBatch dd = view(t);
		const bool emitted = synthEmitApplies(dd, S, tileHops(t));
		if (lastOfSomeStream(t)) // (only a stream's last tile goes to the carried state)
		 timed(timings.otherMs, [&] {
			launchCarryFeed(dd, 0, S, t*T, false, ts.sC);
			launchCarryOut(dd, 0, S, ts.sC);
		});
		if (!ts.serial) SMST_HIP(hipEventRecord(evChain[t%3], ts.sC)); // (everything that reads tile t's workspace on ts.sC is in front of this)
		if (emitted) timed(timings.otherMs, [&] { launchEmitProducts(dd, 0, S, t, ts.sS); });
		if (!ts.serial) SMST_HIP(hipStreamWaitEvent(ts.sS, evOut[launch%3], 0));
		timed(timings.synthMs, [&] {
			if (emitted) launchSynthEmit(dd, io, 0, S, t, ts.sS);
			else launchSynth(dd, 0, S, t*T, tileHops(t), ts.sS);
			if (profiling) ++timings.synthLaunches;
		});
		if (!emitted) timed(timings.emitMs, [&] { launchEmit(dd, io, 0, S, t, run.maxSpan[t], ts.sS); if (profiling) ++timings.emitLaunches; });
		checkLaunch("synthesis / emission");
		if (!ts.serial) SMST_HIP(hipEventRecord(evSynth[t%3], ts.sS));
	};
	for (int t = tile0; t < tile1; ++t) {
		const TileSummary &th = run.tileHas[t];
		const DevBatch dd = view(t);
		if (!ts.serial && t >= tile0 + 3) { // this workspace held tile t-3: its spectra were last read by launch t-2, its results by the synthesis of tile t-3
			SMST_HIP(hipStreamWaitEvent(ts.sF, evChain[t%3], 0));
			SMST_HIP(hipStreamWaitEvent(ts.sF, evSynth[t%3], 0));
		}
		timed(timings.analyseMs, [&] { launchAnalyse(dd, io, 0, S, t*T, tileHops(t), th.windowInCall, th.windowInHistory, ts.sF); if (profiling) ++timings.analyseLaunches; });
		checkLaunch("analysis");
		if (!ts.serial) {
			SMST_HIP(hipEventRecord(evFeed[t%3], ts.sF));
			SMST_HIP(hipStreamWaitEvent(ts.sC, evFeed[t%3], 0));
		}
		ContArgs a{};
		const TileBuffers &w0 = slots[(t + 2)%3], &w1 = slots[t%3]; // tile t-1, tile t
		a.Xcur[0] = w0.Xcur; a.Xprev[0] = w0.Xprev; a.OUT[0] = w0.OUT;
		a.Xcur[1] = w1.Xcur; a.Xprev[1] = w1.Xprev; a.OUT[1] = w1.OUT;
		a.tileInfo = run.dTileInfo + ((size_t)tile0*2)*subS; // the kernel counts tiles, hops and blocks from the segment's first tile
		a.tileStride = 2*subS;
		a.nTiles = tile1 - tile0;
		a.tile = t - tile0;
		a.hopBase = tile0*T;
		a.period = P;
		a.n0 = P*a.tile;
		a.n1 = (t == tile1 - 1) ? P*(a.tile + 1) + 62 : P*(a.tile + 1); // the last launch runs until row 63 of the last tile is through
		a.save = dContSave;
		a.writerWave = contWriterWave;
		timedRecurrence(ts, [&] { launchVocoderContinuous(d, a, 0, S, ts.sC); });
		checkLaunch("bin recurrence (continuous)");
		if (!ts.serial) SMST_HIP(hipEventRecord(evOut[t%3], ts.sC));
		if (t > tile0) finishTile(t - 1, t);
	}
	finishTile(tile1 - 1, tile1 - 1);
	joinTileStreams(ts, tile0, tile1 - tile0, 3);
}

// K0, pass 1: silence gate (signalsmith-stretch.h:231-278) and the number of hops each stream fires in this call.  Host only.
void Batch::gateAndCount(CallPlan &c) {
	const CallSet &cs = *c.cs;
	const int *nIn = cs.hInSamples, *nOut = cs.hOutSamples;
	int *passFlags = cs.hFlags;
	int *clearBits = cs.hResetBits; // per CALL (pinned + its own device copy): a shared buffer could be overwritten by the next call's upload before this call's kResetStreams has run
	pendList.clear();
	for (int s = 0; s < S; ++s) {
		passFlags[s] = 0;
		hopFirst[s] = 0;
		hopCount[s] = 0;
		leavesPendingV[s] = 0;
		ridesV[s] = 0;
		clearBits[s] = 0;
		if (c.active && !c.active[s]) continue;
		lastHop[s].slot = -1; // smst_batch_debug_get_map reports the newest hop of THIS call only
		StreamSched &sc = sched[s];
		float e = 0;
		for (int p = 0; p < kEnergyParts; ++p) e += cs.hEnergy[(size_t)s*kEnergyParts + p];
		if (e < kNoiseFloor) { // :240-278
			if (sc.silenceCounter >= size_t(2*B)) {
				if (sc.silenceFirst) {
					sc.silenceFirst = false;
					sc.seed = seedAfterDroppedBlock(s); // ... which drops the block in flight, with the draws it has made
					sc.samplesSinceLast = SIZE_MAX; // blockProcess = {}
					pend[s] = PendingBlock();
					clearBits[s] = RESET_INPUT | RESET_PREV | RESET_OUTPUT; // Band.input / .prevInput / .output := 0
					c.anyClear = true;
				}
				passFlags[s] = 1;
				c.anyPass = true;
				continue; // the input history is still updated, at the end of process() (copyInput, :270)
			} else {
				sc.silenceCounter += size_t(nIn[s]);
			}
		} else {
			sc.silenceCounter = 0;
			sc.silenceFirst = true;
		}
		const int first = (sc.samplesSinceLast >= size_t(I)) ? 0 : int(size_t(I) - sc.samplesSinceLast);
		hopFirst[s] = first;
		const int starts = (nOut[s] > first) ? (nOut[s] - first + I - 1)/I : 0; // blocks that begin in this call (:281)
		lastStarts[s] = starts;
		if (split) {
			// split computation: a block is finished when its interval is (:321-325).  The block in flight from earlier calls runs now if
			// this call reaches the end of its interval; the last block that begins here stays in flight unless its interval ends here too
			// (a plain one becomes the stream's first hop of this call; one that a flush() interrupted or whose steps saw different parameters runs by itself first)
			if (pend[s].valid && nOut[s] >= first) {
				const PendingBlock &pb = pend[s];
				if (pb.startBin > 0 || pb.zeroPrevAfter || pb.frozenPeaks || pb.frozenForm0 || pb.frozenForm2) pendList.push_back(s);
				else ridesV[s] = 1;
			}
			const int complete = (nOut[s] > first) ? (nOut[s] - first)/I : 0;
			leavesPendingV[s] = starts > complete;
			hopCount[s] = complete + ridesV[s];
		} else {
			hopCount[s] = starts;
		}
		c.maxHops = std::max(c.maxHops, hopCount[s]);
	}
}

// One of a call set's tables has to hold `need` elements: a table that is outgrown is replaced, device copy and pinned staging.  The old pair
// of the set in use is free at once (its last call has finished); the other set's may still be read by the previous call's kernels
template <typename T> void Batch::growCallTable(CallSet &t, bool mine, T *&dev, T *&host, size_t &cap, size_t need) {
	if (need <= cap) return;
	if (mine) { devFree(dev); pinnedFree(host); }
	else { if (dev) t.retiredDevice.push_back(dev); if (host) t.retiredPinned.push_back(host); }
	cap = need + need/4;
	dev = devAlloc<T>(cap);
	host = pinnedAlloc<T>(cap);
}
// per-call tables: pinned staging and device copies grow only when a call needs more hops than any earlier call -- and
// then BOTH sets grow, so that the call after this one (which uses the other set) does not allocate either.  The other
// set's old tables may still be read by the previous call's kernels: they are retired and freed when that set is next used.
void Batch::growCallTables(const CallPlan &c) {
	CallSet &cs = *c.cs;
	for (void *q : cs.retiredDevice) devFree(q);
	for (void *q : cs.retiredPinned) pinnedFree(q);
	cs.retiredDevice.clear();
	cs.retiredPinned.clear();
	for (int which = 0; which < 2; ++which) {
		CallSet &t = which ? callSets.other() : cs;
		growCallTable(t, which == 0, t.hops, t.hHops, t.hopsCap, c.needHops);
		growCallTable(t, which == 0, t.emit, t.hEmit, t.emitCap, c.needEmit);
		growCallTable(t, which == 0, t.tileInfo, t.hTileInfo, t.tileInfoCap, c.needInfo);
	}
}

// K0, pass 2: the block scheduler of stream s, exactly as signalsmith-stretch.h:280-319 does it, straight into the stream's row of the hop
// table; the last block that begins in the call may stay in flight (PendingBlock).  Host only.
void Batch::scheduleStream(CallPlan &c, int s) {
	CallSet &cs = *c.cs;
	const int *nIn = cs.hInSamples, *nOut = cs.hOutSamples;
	const int T = d.T;
	const bool on = !(c.active && !c.active[s]) && !cs.hFlags[s]; // (neither masked out nor passed through by the silence gate)
	HopDesc *list = cs.hHops + (size_t)s*c.hopStride;
	const int nh = hopCount[s];
	const int rides = ridesV[s]; // split computation: the block in flight from an earlier call is this call's hop 0 ...
	const int nStart = nh + (leavesPendingV[s] ? 1 : 0); // ... and the last block that begins here may stay in flight
	if (split) cs.hPendHops[s] = HopDesc{};
	int lastNew = -1;
	if (rides) {
		pendingHop(s, list[0]);
		if (pend[s].flags & HOP_NEW_SPECTRUM) lastNew = 0;
		if (pend[s].flags & HOP_RANDOM_TF) sched[s].seed = advanceOneHop(sched[s].seed); // its draws happen now
		pend[s] = PendingBlock();
	}
	if (nStart > rides) {
		StreamSched &sc = sched[s];
		const StreamParams &prm = params[s];
		const bool mapped = prm.hasCustomMap || prm.freqMultiplier != 1; // :300
		const bool formants = prm.formantMultiplier != 1 || (prm.formantCompensation && mapped); // :310
		int o = hopFirst[s];
		for (int j = rides; j < nStart; ++j, o += I) {
			HopDesc inFlight{};
			HopDesc &hd = (j < nh) ? list[j] : inFlight;
			int inputOffset = int(std::round(o*float(nIn[s])/nOut[s])); // :288 (fp32 on purpose)
			int inputInterval = inputOffset - sc.prevInputOffset;
			sc.prevInputOffset = inputOffset;
			hd.inputOffset = inputOffset;
			hd.outPos = o;
			unsigned flags = HOP_ACTIVE;
			const bool newSpectrum = sc.didSeek || inputInterval > 0; // :299
			bool reanalyse = false;
			if (newSpectrum) {
				flags |= HOP_NEW_SPECTRUM;
				reanalyse = sc.didSeek || std::abs(inputInterval - I) > 1; // :303
				if (reanalyse) flags |= HOP_REANALYSE_PREV;
			}
			if (mapped) flags |= HOP_MAPPED;
			if (formants) flags |= HOP_FORMANTS;
			float tf = sc.didSeek ? sc.seekTimeFactor : float(I)/std::max<float>(1, float(inputInterval)); // :312
			sc.didSeek = false;
			tf = std::max<float>(tf, 1/kMaxCleanStretch); // :638
			if (tf > kMaxCleanStretch) flags |= HOP_RANDOM_TF; // :639
			hd.timeFactor = tf;
			hd.flags = flags;
			lastSteps[s] = stepLayout(flags).steps;
			hd.seed = sc.seed; // the engine's state before this hop's draws
			if ((flags & HOP_RANDOM_TF) && j < nh) sc.seed = advanceOneHop(sc.seed); // 2M - 2 draws later (a block left in flight draws when it runs: seedAfterDroppedBlock)
			if (j == nh) {
				// in flight at the end of the call: analysed now, from the input as it stands (:293 stashes it), into the pending buffers;
				// everything else when its interval is complete -- or when a flush() needs to know how far it has come
				PendingBlock &pb = pend[s];
				pb = PendingBlock();
				pb.valid = true;
				pb.flags = flags;
				pb.timeFactor = tf;
				pb.seed = hd.seed;
				HopDesc &ph = cs.hPendHops[s];
				ph.inputOffset = inputOffset;
				ph.flags = flags & (HOP_ACTIVE | HOP_NEW_SPECTRUM | HOP_REANALYSE_PREV);
				if (newSpectrum) {
					c.anyPendAnalysis = true;
					for (int which = 0; which < (reanalyse ? 2 : 1); ++which) (analysisWindowInCall(d.B, d.M, d.I, inputOffset, which, nIn[s]) ? c.pendInCall : c.pendLate) = true;
				}
				continue;
			}
			const int tile = j/T;
			const bool lastInTile = lastNew >= 0 && lastNew/T == tile;
			hd.inSrc = newSpectrum ? j%T : (lastInTile ? lastNew%T : SRC_STATE);
			if (newSpectrum && reanalyse) hd.prevSrc = SRC_REANALYSED;
			else hd.prevSrc = lastInTile ? lastNew%T : SRC_STATE;
			if (newSpectrum) lastNew = j;
		}
		sc.samplesSinceLast = size_t(nOut[s] - (o - I));
	} else if (on && sched[s].samplesSinceLast != SIZE_MAX) {
		sched[s].samplesSinceLast += size_t(nOut[s]);
	}
	if (on) sched[s].prevInputOffset -= nIn[s]; // :419
}

// What the hops that scheduleStream() gave stream s mean for each tile: the stream's emission windows, its rows of the tile-info table
// (layout [sub][tile][2][subS]: nHops, lastNewHop), its share of the tiles' summaries and spans.  Host only.
void Batch::summariseStreamTiles(const CallPlan &c, int s) {
	const CallSet &cs = *c.cs;
	const int T = d.T, nTiles = c.nTiles, sub = s/subS, sl = s%subS;
	const int nIn = cs.hInSamples[s], nh = hopCount[s];
	const HopDesc *list = cs.hHops + (size_t)s*c.hopStride;
	for (int t = 0; t < nTiles; ++t) {
		const int h0 = t*T, h1 = std::min(nh, h0 + T);
		const int cnt = std::max(0, h1 - h0);
		EmitDesc ed{};
		const int total = cs.hFlags[s] ? 0 : cs.hOutSamples[s];
		if (t == 0) ed.nLo = 0; else ed.nLo = (h0 < nh) ? list[h0].outPos : total;
		ed.nHi = (h1 < nh && cnt > 0) ? list[h1].outPos : total;
		if (cnt == 0 && t > 0) ed.nLo = ed.nHi = total;
		ed.firstHopPos = cnt > 0 ? list[h0].outPos : 0;
		ed.hopCount = cnt;
		cs.hEmit[(size_t)s*nTiles + t] = ed;
		int *info = cs.hTileInfo + ((size_t)(sub*nTiles + t)*2)*subS;
		info[sl] = cnt;
		int lastNewLocal = -1;
		TileSummary &th = tileHasV[(size_t)sub*nTiles + t];
		th.maxHops = std::max(th.maxHops, cnt);
		for (int h = h0; h < h1; ++h) {
			const unsigned f = list[h].flags;
			if (f & HOP_PREANALYSED) th.preAnalysed = true;
			if ((f & HOP_NEW_SPECTRUM) && (f & HOP_PREANALYSED)) lastNewLocal = h - h0;
			if ((f & HOP_NEW_SPECTRUM) && !(f & HOP_PREANALYSED)) {
				lastNewLocal = h - h0; th.newSpectrum = true;
				// analysis frames whose window lies in this call's input (taken by kAnalyseTeams) / reaches into the history
				for (int which = 0; which < ((f & HOP_REANALYSE_PREV) ? 2 : 1); ++which) {
					const bool inCall = analysisWindowInCall(d.B, d.M, d.I, list[h].inputOffset, which, nIn);
					(inCall ? th.windowInCall : th.windowInHistory) = true;
					if (!inCall) th.lateHops = std::max(th.lateHops, h - h0 + 1);
				}
			}
			if (!(f & HOP_REANALYSE_PREV) || list[h].prevSrc != SRC_REANALYSED) th.plainPrev = true;
			th.anyHop = true;
			if (!(f & HOP_NEW_SPECTRUM)) th.reusedSpectrum = true; // (a hop that re-uses the spectrum before it: the continuous wavefront asks for a new one per hop)
			if (f & HOP_MAPPED) th.mapped = true;
			if (f & HOP_FORMANTS) { th.formants = true; if ((f & HOP_PREANALYSED) || params[s].formantBaseFreq <= 0) th.estimatesBase = true; } // (a stream that estimates its base frequency, :929-966)
			if (f & HOP_RANDOM_TF) th.randomTimeFactor = true;
		}
		info[subS + sl] = lastNewLocal;
		if (cnt > 0) noteLastHop(s, (sub*nTiles + t) & 1, cnt - 1, list[h1 - 1].flags);
		int &span = maxSpanV[(size_t)sub*nTiles + t];
		span = std::max(span, ed.nHi - ed.nLo);
	}
}

void Batch::process(const float *in, long long inSS, long long inCS, const int *inSamples,
                    float *out, long long outSS, long long outCS, const int *outSamples, const unsigned char *active) {
	SMST_HIP(hipSetDevice(dev));
	const auto hostT0 = std::chrono::steady_clock::now();
	auto msSince = [](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count(); };
	uploadParams();
	// This call's tables go into the set that the call before the previous one used (its kernels must have finished);
	// everything up to the first tile launch runs on `stGate`, so the host-side scheduling of this call overlaps the
	// kernels of the previous call that are still queued on `st`.  All staging is pinned and owned by the set, so the
	// uploads are asynchronous and the ONLY host synchronisation of a call is the silence-gate readback.
	CallSet &cs = callSets.begin(&hostTimes.waitTablesMs);
	dInSamples = cs.inSamples; dOutSamples = cs.outSamples; dFlags = cs.flags;
	const int T = d.T;
	int *nIn = cs.hInSamples, *nOut = cs.hOutSamples;
	int maxOut = 0, maxIn = 0;
	for (int s = 0; s < S; ++s) {
		bool on = !active || active[s];
		nIn[s] = on ? inSamples[s] : 0;
		nOut[s] = on ? outSamples[s] : 0;
		if (nIn[s] < 0 || nOut[s] < 0) throw Error("negative sample count");
		maxOut = std::max(maxOut, nOut[s]);
		maxIn = std::max(maxIn, nIn[s]);
	}
	SMST_HIP(hipMemcpyAsync(dInSamples, nIn, S*sizeof(int), hipMemcpyHostToDevice, stGate));
	SMST_HIP(hipMemcpyAsync(dOutSamples, nOut, S*sizeof(int), hipMemcpyHostToDevice, stGate));
	IoArgs io{in, out, inSS, inCS, outSS, outCS, dInSamples, dOutSamples};

	// K5: silence gate needs the input energy on the host (one 64-byte-per-stream readback per call)
	launchEnergy(d, io, 0, S, maxIn, dEnergy, stGate);
	SMST_HIP(hipMemcpyAsync(cs.hEnergy, dEnergy, (size_t)S*kEnergyParts*sizeof(float), hipMemcpyDeviceToHost, stGate));
	{ const auto t = std::chrono::steady_clock::now(); SMST_HIP(hipStreamSynchronize(stGate)); hostTimes.waitGateMs += msSince(t); }

	CallPlan c{&cs, active}; // (everything else zero)
	gateAndCount(c);
	if (c.anyClear) { // asynchronous: the masks travel on `st`, ahead of the launch that reads them
		SMST_HIP(hipMemcpyAsync(cs.resetBits, cs.hResetBits, S*sizeof(int), hipMemcpyHostToDevice, st));
		launchResetStreams(d, cs.resetBits, 0, dSeedWp, st);
	}
	if (!pendList.empty()) runPendingBlocks(nullptr);
	const int maxHops = c.maxHops, nTiles = std::max(1, (maxHops + T - 1)/T);
	// One row of T hop descriptors per stream and tile -- except in the real-time calling pattern, where no stream fires more than one hop per
	// call: the single-hop kernels index hop 0 only, so a row is ONE descriptor (4096 streams: 131 KB to clear and upload per 128-frame
	// quantum instead of 8.4 MB -- a third of the quantum's cost).  (The wavefront kernels load a row of 64 blindly: they keep the full rows.)
	const bool compactHops = maxHops <= 1 && formReachable(d, formSwitches, RecurrenceKernel::ONE);
	c.nTiles = nTiles;
	c.hopStride = compactHops ? 1 : nTiles*T;
	const int nSub = (S + subS - 1)/subS;
	c.needHops = (size_t)S*c.hopStride; c.needEmit = (size_t)S*nTiles; c.needInfo = (size_t)nSub*nTiles*2*subS;
	growCallTables(c);
	dHops = cs.hops; dEmit = cs.emit; dTileInfo = cs.tileInfo;
	std::memset(cs.hHops, 0, c.needHops*sizeof(HopDesc));
	std::memset(cs.hTileInfo, 0, c.needInfo*sizeof(int));
	ensureSize(maxSpanV, (size_t)nSub*nTiles, allocEvents);
	ensureSize(tileHasV, (size_t)nSub*nTiles, allocEvents);
	std::fill(maxSpanV.begin(), maxSpanV.end(), 0);
	std::fill(tileHasV.begin(), tileHasV.end(), TileSummary{});
	for (int s = 0; s < S; ++s) {
		scheduleStream(c, s);
		summariseStreamTiles(c, s);
	}
	SMST_HIP(hipMemcpyAsync(dHops, cs.hHops, c.needHops*sizeof(HopDesc), hipMemcpyHostToDevice, stGate));
	SMST_HIP(hipMemcpyAsync(dEmit, cs.hEmit, c.needEmit*sizeof(EmitDesc), hipMemcpyHostToDevice, stGate));
	SMST_HIP(hipMemcpyAsync(dTileInfo, cs.hTileInfo, c.needInfo*sizeof(int), hipMemcpyHostToDevice, stGate));
	if (c.anyPass) SMST_HIP(hipMemcpyAsync(dFlags, cs.hFlags, S*sizeof(int), hipMemcpyHostToDevice, stGate));
	if (c.anyPendAnalysis) SMST_HIP(hipMemcpyAsync(cs.pendHops, cs.hPendHops, S*sizeof(HopDesc), hipMemcpyHostToDevice, stGate));
	// the kernels below are ordered after the uploads by an event, not by the host
	SMST_HIP(hipEventRecord(cs.tables, stGate));
	SMST_HIP(hipStreamWaitEvent(st, cs.tables, 0));

	d.hops = dHops;
	d.emit = dEmit;
	d.hopStride = c.hopStride;
	d.emitStride = nTiles;

	// no stream fires a hop (most quanta of a real-time host): the output is the front of the carried sums, and -- while the rows have room --
	// what is left of them stays in place (kEmitCarried)
	bool carriedOnly = maxHops == 0 && carriedEmit;
	for (int s = 0; s < S && carriedOnly; ++s) carriedOnly = carryBase[s] + (cs.hFlags[s] ? 0 : nOut[s]) + d.carryLen <= d.carryPitch;
	if (carriedOnly) for (int s = 0; s < S; ++s) carryBase[s] += cs.hFlags[s] ? 0 : nOut[s];
	runTiles(TileRun{&io, nTiles, maxHops, tileHasV.data(), maxSpanV.data(), dTileInfo, false, nullptr, carriedOnly});
	if (c.anyPendAnalysis) timed(timings.analyseMs, [&] {
		// the blocks left in flight: their spectra (Band.input and, where :303 asks for it, the re-analysed Band.prevInput) into the pending
		// buffers, laid out as a one-hop tile over ALL streams
		DevBatch dp = d;
		dp.hops = cs.pendHops;
		dp.hopStride = 1;
		dp.T = 1;
		dp.Xcur = dPendIn;
		dp.Xprev = dPendPrev;
		launchAnalyse(dp, io, 0, S, 0, 1, c.pendInCall, c.pendLate, st);
		if (profiling) ++timings.analyseLaunches;
	});
	timed(timings.otherMs, [&] {
		if (c.anyPass) launchPassThrough(d, io, dFlags, maxOut, st);
		// the input history slides (kHistory): the host follows each stream's window to size the launch
		int span = 0;
		for (int s = 0; s < S; ++s) {
			const int n = nIn[s];
			if (histBase[s] + d.histLen + n <= d.histPitch) { histBase[s] += n; span = std::max(span, n); }
			else { histBase[s] = 0; span = std::max(span, d.histLen); }
		}
		launchHistory(d, io, span, st);
	});
	d.histCur ^= 1;
	callSets.end(st);
	SMST_HIP(hipGetLastError());
	hostTimes.callMs += msSince(hostT0);
	++hostTimes.calls;
}

// ---- seek -------------------------------------------------------------------------------------------------
void Batch::seek(const float *in, long long inSS, long long inCS, const int *inSamples, const double *rates, const unsigned char *active) {
	SMST_HIP(hipSetDevice(dev));
	// a stage set ([S] sample counts, [S] flags, [S] history lengths; the energy partials come back into it): one host synchronisation of its
	// own (the energy readback that decides about the silence counter, :159-162)
	SMST_HIP(hipStreamSynchronize(st)); // (no staging needs it any more -- the set's event guards that; kept: EXPERIMENTS.md, "One per-call table set")
	StageSet &t = stageSets.begin();
	int *nIn = t.host, *flags = t.host + S, *histN = t.host + 2*S;
	for (int s = 0; s < S; ++s) {
		const bool on = !active || active[s];
		flags[s] = on ? 1 : 0;
		nIn[s] = on ? inSamples[s] : 0;
		histN[s] = d.histLen;
		if (nIn[s] < 0) throw Error("negative sample count");
	}
	uploadStage(t, 3);
	IoArgs io{in, nullptr, inSS, inCS, 0, 0, t.dev, dOutSamples};
	launchSeekHistory(d, io, t.dev + S, st);
	d.histCur ^= 1;
	// energy of the copied part only (:144-154) = energy over the new history (the zero padding adds nothing)
	for (int s = 0; s < S; ++s) if (flags[s]) histBase[s] = 0;
	IoArgs ioE{d.hist, nullptr, (long long)C*d.histPitch, (long long)d.histPitch, 0, 0, t.dev + 2*S, dOutSamples}; // (the streams that seek: their windows are at the front of the rows now)
	launchEnergy(d, ioE, 0, S, d.histLen, dEnergy, st);
	SMST_HIP(hipMemcpyAsync(t.hEnergy, dEnergy, (size_t)S*kEnergyParts*sizeof(float), hipMemcpyDeviceToHost, st));
	stageSets.end(st);
	SMST_HIP(hipStreamSynchronize(st));
	for (int s = 0; s < S; ++s) {
		if (!flags[s]) continue;
		float e = 0;
		for (int p = 0; p < kEnergyParts; ++p) e += t.hEnergy[(size_t)s*kEnergyParts + p];
		StreamSched &sc = sched[s];
		if (e >= kNoiseFloor) { // :159-162
			sc.silenceCounter = 0;
			sc.silenceFirst = true;
		}
		sc.didSeek = true; // :163
		const double rate = rates ? rates[s] : 1.0;
		sc.seekTimeFactor = (rate*I > 1) ? float(1/rate) : float(I); // :164
	}
}

// ---- flush ------------------------------------------------------------------------------------------------
// How far the REAL output ring, which the reference's flush() / outputSeek() touch, is ahead of the stashed one that process() emits from (split computation: what is left of the interval)
int Batch::aheadOffset(int s) const {
	const size_t since = sched[s].samplesSinceLast;
	return (split && since != SIZE_MAX && since < size_t(I)) ? int(size_t(I) - since) : 0;
}
void Batch::flush(float *out, long long outSS, long long outCS, const int *outSamples, const float *rates, const unsigned char *active) {
	SMST_HIP(hipSetDevice(dev));
	std::vector<int> &blockOut = flushV.blockOut, &blockIn = flushV.blockIn, &synthChannels = flushV.synthChannels; // (every entry is written below)
	std::vector<unsigned char> &runBlock = flushV.runBlock, &on = flushV.on;
	bool anyBlock = false;
	int maxIn = 0;
	for (int s = 0; s < S; ++s) {
		on[s] = !(active && !active[s]);
		if (on[s] && outSamples[s] < 0) throw Error("negative sample count");
		const int outputBlock = on[s] ? std::max(0, outSamples[s] - I) : 0; // :439
		runBlock[s] = outputBlock > 0;
		anyBlock = anyBlock || runBlock[s];
		blockOut[s] = outputBlock;
		blockIn[s] = (runBlock[s] && rates) ? int(outputBlock*rates[s]) : 0; // :440
		maxIn = std::max(maxIn, blockIn[s]);
		synthChannels[s] = -1;
	}
	if (anyBlock) {
		if (growScratch(dZeros, zerosCapacity, (size_t)maxIn + 1, 4096, false)) {
			// process() reads this on another stream (the silence gate runs on stGate): complete the fill before going on
			SMST_HIP(hipMemsetAsync(dZeros, 0, zerosCapacity*sizeof(float), st));
			SMST_HIP(hipStreamSynchronize(st));
		}
		process(dZeros, 0, 0, blockIn.data(), out, outSS, outCS, blockOut.data(), runBlock.data());
	}
	// Split computation, between two interval boundaries: how far has the block in flight come?  (:321-325 spread its steps over the
	// interval; flush() reads the REAL ring, one interval ahead of the stashed one that process() emits from, then stft.reset(0.1) and
	// prevInput = output = 0, :442-463 -- and the block's remaining steps run afterwards, on what the flush left.  Pinned step by step by
	// tests/golden/split_events.)
	pendList.clear();
	for (int s = 0; s < S; ++s) {
		if (!on[s] || !split || !pend[s].valid) continue;
		PendingBlock &pb = pend[s];
		const StepLayout l = stepLayout(pb.flags);
		const size_t e = stepsExecuted(size_t(l.steps), sched[s].samplesSinceLast);
		if (e > size_t(l.synth0)) {
			// the spectrum is complete and e - synth0 channels have been synthesised into the ring (all of them: the block is finished): run
			// the block now; the other channels' frames never come -- stft.reset() clears the spectrum they would be made from
			synthChannels[s] =(e >= size_t(l.steps)) ? -1 : int(e) - l.synth0;
			pendList.push_back(s);
		} else if (e >= size_t(l.spectrum)) {
			// output (and, after `.input -> .prevInput`, prevInput) were complete and are zeroed; what remains is a silent frame: its window product
			pb.startBin = M;
			pb.zeroPrevAfter = true;
		} else if (e > size_t(l.main0)) {
			// e - main0 chunks of the main prediction ran: those bins are zero now, the later chunks start from zeros (:725-726)
			pb.startBin = std::max(pb.startBin, int(size_t(M)*(e - size_t(l.main0))/8));
		} else if (l.copyIn >= 0 && e > size_t(l.analyse0) && e <= size_t(l.copyIn)) {
			// e - analyse0 channels were analysed, not yet copied into Band.input: stft.reset() cleared their spectra (:356-373)
			const int n = std::min(C, int(e) - l.analyse0);
			SMST_HIP(hipMemsetAsync(dPendIn + (size_t)s*C*d.Mp, 0, (size_t)n*d.Mp*sizeof(float2), st));
		}
	}
	if (!pendList.empty()) runPendingBlocks(synthChannels.data());
	// the stage's own set, now that process() and runPendingBlocks() are through with theirs: the tail's length (-1: the stream takes no
	// part), where the real ring's read position is in the stashed one, where the tail goes in the stream's output
	StageSet &t = stageSets.begin();
	int *tail = t.host, *tailOff = t.host + S, *outOff = t.host + 2*S;
	for (int s = 0; s < S; ++s) {
		tail[s] = on[s] ? outSamples[s] - blockOut[s] : -1;
		tailOff[s] = on[s] ? aheadOffset(s) : 0;
		outOff[s] = blockOut[s];
	}
	uploadStage(t, 3);
	SMST_HIP(hipStreamSynchronize(st)); // (the upload no longer needs it -- pinned, and the set's event guards it; kept: EXPERIMENTS.md, "One per-call table set")
	IoArgs io{nullptr, out, 0, 0, outSS, outCS, dInSamples, t.dev};
	settleCarry();
	launchFlushTail(d, io, t.dev + S, t.dev + 2*S, st);
	stageSets.end(st);
	// stft.reset(0.1) + zero prevInput/output (:456-463).  Split computation: the samples up to the end of the interval still come from
	// the stashed ring (:407-415), which the reset does not touch -- the fresh ring begins behind them
	for (int s = 0; s < S; ++s) if (on[s]) lastHop[s] = LastHop();
	resetStreams([&on](int s) { return on[s] != 0; }, RESET_STFT | RESET_PREV | RESET_OUTPUT, split);
	SMST_HIP(hipGetLastError());
}

// ---- outputSeek -------------------------------------------------------------------------------------------
void Batch::outputSeek(const float *in, long long inSS, long long inCS, const int *inputLengths, const unsigned char *active) {
	// signalsmith-stretch.h:173-204
	if (active) resetStreamsMasked(active);
	else reset();
	const int outLat = outputLatency(), inLat = inputLatency();
	std::vector<int> &seekSamples = outputSeekV.seekSamples, &surplus = outputSeekV.surplus, &preOut = outputSeekV.preOut, &done = outputSeekV.done; // (every entry is written below)
	std::vector<double> &rates = outputSeekV.rates;
	std::vector<unsigned char> &mask = outputSeekV.mask;
	for (int s = 0; s < S; ++s) {
		const bool on = !(active && !active[s]);
		surplus[s] = on ? std::max(inputLengths[s] - inLat, 0) : 0;
		float playbackRate = surplus[s]/float(outLat);
		seekSamples[s] = on ? inputLengths[s] - surplus[s] : 0;
		rates[s] = on ? playbackRate : 1.0;
		preOut[s] = outLat;
		done[s] = !on; // (... of the pre-roll, below)
	}
	seek(in, inSS, inCS, seekSamples.data(), rates.data(), active);
	growScratch(dScratchOut, scratchOutCapacity, (size_t)S*C*outLat, 0, false); // pre-roll output into scratch [S][C][outLat]
	// offset input per stream: seekSamples differ per stream, so pass per-stream start through a shifted base when uniform,
	// otherwise run stream groups with equal offsets
	for (int s0 = 0; s0 < S; ++s0) {
		if (done[s0]) continue;
		std::fill(mask.begin(), mask.end(), 0);
		for (int s = s0; s < S; ++s) if (!done[s] && seekSamples[s] == seekSamples[s0]) { mask[s] = 1; done[s] = 1; }
		process(in + seekSamples[s0], inSS, inCS, surplus.data(), dScratchOut, (long long)C*outLat, outLat, preOut.data(), mask.data());
	}
	// "put the thing down, flip it and reverse it" (:198-203): negate, reverse, add into the output ring (a stream that is masked out
	// gets an offset behind its ring: nothing is added)
	StageSet &t = stageSets.begin();
	for (int s = 0; s < S; ++s) t.host[s] = (active && !active[s]) ? d.carryLen : aheadOffset(s);
	uploadStage(t, 1);
	SMST_HIP(hipStreamSynchronize(st)); // (the upload no longer needs it -- pinned, and the set's event guards it; kept: EXPERIMENTS.md, "One per-call table set")
	settleCarry();
	launchAddPreRoll(d, dScratchOut, outLat, t.dev, st);
	stageSets.end(st);
	SMST_HIP(hipGetLastError());
}

// ---- exact ------------------------------------------------------------------------------------------------
bool Batch::growScratch(float *&scratch, size_t &capacity, size_t need, size_t room, bool workspace) {
	if (need <= capacity) return false;
	if (scratch) { SMST_HIP(hipStreamSynchronize(st)); devFree(scratch); if (workspace) wsBytes -= capacity*sizeof(float); }
	scratch = nullptr;
	capacity = 0;
	scratch = devAlloc<float>(need + room);
	capacity = need + room;
	if (workspace) wsBytes += capacity*sizeof(float);
	return true;
}

void Batch::exact(const ClipIo &io, const int *inSamples, const int *outSamples, unsigned char *tooShort) {
	// signalsmith-stretch.h:468-491, every participating stream at once.  A stream cuts its clip where its own rate says (exactLengths), the
	// engine's kernels take one offset for all streams: so the stages run on planar images in which every stream's stage begins at one
	// column -- input [0, seekLength_s) at column 0 and [seekLength_s, in_s) at column P; output [0, outputIndex_s) from column 0 and the
	// flush [outputIndex_s, out_s) from column Q -- and kClipIn / kClipOut (smst_clip.h) move the segments.  A caller's buffer that is planar
	// fp32 itself serves the two stages whose offset is 0 for every stream directly: outputSeek reads it, the main process writes it; only the
	// input behind seekLength_s and the flush go through the images.
	SMST_HIP(hipSetDevice(dev));
	const bool direct = io.format == 0;
	for (ClipSet &t : clipSets.sets) { // (both sets with the first call: the second call allocates nothing)
		if (t.host) continue;
		t.host = pinnedAlloc<ClipSeg>((size_t)4*S);
		t.dev = devAlloc<ClipSeg>((size_t)4*S);
		wsBytes += (size_t)4*S*sizeof(ClipSeg);
	}
	clipSets.create();
	ClipSet &cs = clipSets.begin(); // (the call before the previous one: its clip kernels must have read the tables)
	std::vector<int> &seekLen = exactV.seekLen, &rest = exactV.rest, &procOut = exactV.procOut, &flushN = exactV.flushN, &frames = exactV.frames, &render = exactV.render;
	std::vector<float> &rates = exactV.rates;
	std::vector<unsigned char> &run = exactV.run;
	int maxSeek = 0, maxRest = 0, maxProc = 0, maxFlush = 0, maxZeros = 0;
	int maxRaw = 0, maxResampled = 0, maxPlainSeek = 0, maxPlainRest = 0; // the resampled streams that run: their longest clip, before and behind; the others' longest segments
	int maxDelivered = 0; // the out-resampled streams that run: their longest delivered clip
	bool anyRun = false;
	for (int s = 0; s < S; ++s) {
		seekLen[s] = rest[s] = procOut[s] = flushN[s] = run[s] = 0;
		rates[s] = 0.0f;
		frames[s] = render[s] = 0;
		if (outSamples[s] < 0) continue;
		// (a resampled stream behaves exactly as if the caller had handed over its Nr frames; the caller has checked that Nr fits an int)
		frames[s] = io.resample && resampled(s) ? int(resampledLengthOf(s, inSamples[s])) : inSamples[s];
		// (an out-resampled stream behaves towards the engine exactly as if the caller had asked for its E frames; the caller has checked that E fits an int)
		const bool outRes = io.outResample && outResampled(s);
		render[s] = outRes ? int(outRenderLengthOf(s, outSamples[s])) : outSamples[s];
		ExactLengths l = exactLengths(frames[s], render[s]);
		if (l.tooShort) { maxZeros = std::max(maxZeros, outSamples[s]); continue; }
		l.outputIndex = std::min(std::max(l.outputIndex, 0), render[s]); // (seekLength/rate <= render[s] but for its rounding: the two output parts stay inside the stream's count)
		run[s] = 1;
		anyRun = true;
		rates[s] = l.rate;
		seekLen[s] = l.seekLength; rest[s] = frames[s] - l.seekLength;
		if (io.resample && resampled(s)) { maxRaw = std::max(maxRaw, inSamples[s]); maxResampled = std::max(maxResampled, frames[s]); }
		else { maxPlainSeek = std::max(maxPlainSeek, seekLen[s]); maxPlainRest = std::max(maxPlainRest, rest[s]); }
		procOut[s] = l.outputIndex; flushN[s] = render[s] - l.outputIndex;
		if (outRes) maxDelivered = std::max(maxDelivered, outSamples[s]);
		maxSeek = std::max(maxSeek, seekLen[s]); maxRest = std::max(maxRest, rest[s]);
		maxProc = std::max(maxProc, procOut[s]); maxFlush = std::max(maxFlush, flushN[s]);
	}
	// columns and row pitches: multiples of 4 floats, so that every row and both columns of an image begin on 16-byte boundaries
	auto up4 = [](int n) { return (n + 3)/4*4; };
	const int P = direct ? 0 : up4(maxSeek), Q = direct ? 0 : up4(maxProc);
	// (a call with an out-resampled stream: a third column R of the output image, where kClipResampleOut puts those streams' delivered frames)
	const int R = up4(Q + maxFlush);
	const int pitchIn = std::max(up4(P + maxRest), 4), pitchOut = std::max(maxDelivered > 0 ? up4(R + maxDelivered) : R, 4);
	const size_t needIn = (size_t)S*C*pitchIn, needOut = (size_t)S*C*pitchOut;
	growScratch(dClipIn, clipInCapacity, needIn, needIn/8 + 1024, true);
	growScratch(dClipOut, clipOutCapacity, needOut, needOut/8 + 1024, true);
	ClipSeg *segIn = cs.host, *segOut = cs.host + (size_t)2*S;
	for (int s = 0; s < S; ++s) {
		const ClipSeg none{0, 0, 0, 0};
		segIn[2*s] = segIn[2*s + 1] = segOut[2*s] = segOut[2*s + 1] = none;
		if (run[s]) {
			if (!direct) segIn[2*s] = ClipSeg{0, 0, seekLen[s], 0};
			segIn[2*s + 1] = ClipSeg{seekLen[s], P, rest[s], 0};
			if (!direct) segOut[2*s] = ClipSeg{0, 0, procOut[s], 0};
			segOut[2*s + 1] = ClipSeg{Q, procOut[s], flushN[s], 0};
			if (io.outResample && outResampled(s)) { // what the level stages and kClipOut read: the delivered frames, one segment from column R
				segOut[2*s] = ClipSeg{R, 0, outSamples[s], 0};
				segOut[2*s + 1] = none;
			}
		} else if (outSamples[s] > 0) {
			segOut[2*s] = ClipSeg{0, 0, outSamples[s], 1}; // too short: zeros, and the stream's state stays as it is
		}
	}
	const long long inImgSS = (long long)C*pitchIn, outImgSS = (long long)C*pitchOut;
	int maxOutSpanPitch = 4;
	const ResampleOutTableLayout outAt(S);
	if (maxDelivered > 0) {
		// The out-resampled streams: where their rendered frames lie (the two segments every other stream hands to kClipOut), where their
		// delivered frames go, and their entries, in a table of its own
		if (direct) throw Error("exact: an out-resampled stream in a planar call");
		for (ClipSet &t : clipSets.sets) { // (both sets with the first such call)
			if (t.outHost) continue;
			t.outHost = pinnedAlloc<unsigned char>(outAt.bytes());
			t.outDev = devAlloc<unsigned char>(outAt.bytes());
			wsBytes += outAt.bytes();
		}
		for (int s = 0; s < S; ++s) {
			const ClipSeg none{0, 0, 0, 0};
			ResampleOutEntry e{nullptr, 0, 0, 0, 0, 0, 0, 0, 0};
			outAt.srcSegs(cs.outHost)[2*s] = outAt.srcSegs(cs.outHost)[2*s + 1] = outAt.dstSegs(cs.outHost)[2*s] = outAt.dstSegs(cs.outHost)[2*s + 1] = none;
			if (run[s] && outResampled(s)) {
				const ResampleSlot &slot = resampleSlots[outResampleSlot[s]];
				const ResampleShape &g = slot.shape;
				e = ResampleOutEntry{slot.taps, render[s], outSamples[s], g.L, g.M, g.H, g.T, g.pitch, 0};
				maxOutSpanPitch = std::max(maxOutSpanPitch, resampleSpanPitch(g.L, g.M, g.T));
				outAt.srcSegs(cs.outHost)[2*s] = ClipSeg{0, 0, procOut[s], 0};
				outAt.srcSegs(cs.outHost)[2*s + 1] = ClipSeg{Q, procOut[s], flushN[s], 0};
				outAt.dstSegs(cs.outHost)[2*s] = ClipSeg{0, R, outSamples[s], 0};
			}
			outAt.entries(cs.outHost)[s] = e;
		}
		SMST_HIP(hipMemcpyAsync(cs.outDev, cs.outHost, outAt.bytes(), hipMemcpyHostToDevice, st));
	}
	if (maxResampled > 0) {
		// The resampled streams: kClipIn moves their whole clips into the raw image -- a second segment table, one whole-clip segment per
		// stream -- and leaves them out of the input image, which kClipResample fills where the call's two input segments put their frames
		if (direct) throw Error("exact: a resampled stream in a planar call");
		const ResampleTableLayout at(S);
		for (ClipSet &t : clipSets.sets) { // (both sets with the first such call)
			if (t.resHost) continue;
			t.resHost = pinnedAlloc<unsigned char>(at.bytes());
			t.resDev = devAlloc<unsigned char>(at.bytes());
			wsBytes += at.bytes();
		}
		const int pitchRaw = up4(maxRaw);
		const size_t needRaw = (size_t)S*C*pitchRaw;
		growScratch(dClipRaw, clipRawCapacity, needRaw, needRaw/8 + 1024, true);
		int maxSpanPitch = 4;
		for (int s = 0; s < S; ++s) {
			const ClipSeg none{0, 0, 0, 0};
			ResampleEntry e{nullptr, 0, 0, 0, 0, 0, 0, 0, 0};
			at.rawSegs(cs.resHost)[2*s] = at.rawSegs(cs.resHost)[2*s + 1] = at.dstSegs(cs.resHost)[2*s] = at.dstSegs(cs.resHost)[2*s + 1] = none;
			if (run[s] && resampled(s)) {
				const ResampleSlot &slot = resampleSlots[resampleSlot[s]];
				const ResampleShape &g = slot.shape;
				e = ResampleEntry{slot.taps, inSamples[s], frames[s], g.L, g.M, g.H, g.T, g.pitch, 0};
				maxSpanPitch = std::max(maxSpanPitch, resampleSpanPitch(g.L, g.M, g.T));
				at.rawSegs(cs.resHost)[2*s] = ClipSeg{0, 0, inSamples[s], 0};
				at.dstSegs(cs.resHost)[2*s] = segIn[2*s];
				at.dstSegs(cs.resHost)[2*s + 1] = segIn[2*s + 1];
				segIn[2*s] = segIn[2*s + 1] = none;
			}
			at.entries(cs.resHost)[s] = e;
		}
		SMST_HIP(hipMemcpyAsync(cs.dev, cs.host, (size_t)4*S*sizeof(ClipSeg), hipMemcpyHostToDevice, st));
		SMST_HIP(hipMemcpyAsync(cs.resDev, cs.resHost, at.bytes(), hipMemcpyHostToDevice, st));
		const long long rawSS = (long long)C*pitchRaw;
		launchClipIn(io.format, io.in, io.inStreamStride, io.inInnerStride, dClipRaw, rawSS, pitchRaw, at.rawSegs(cs.resDev), S, C, maxRaw, st);
		launchClipIn(io.format, io.in, io.inStreamStride, io.inInnerStride, dClipIn, inImgSS, pitchIn, cs.dev, S, C, std::max(maxPlainSeek, maxPlainRest), st);
		launchClipResample(dClipRaw, rawSS, pitchRaw, dClipIn, inImgSS, pitchIn, at.dstSegs(cs.resDev), at.entries(cs.resDev), S, C, maxResampled, maxSpanPitch, st);
	} else {
		SMST_HIP(hipMemcpyAsync(cs.dev, cs.host, (size_t)4*S*sizeof(ClipSeg), hipMemcpyHostToDevice, st));
		launchClipIn(io.format, io.in, io.inStreamStride, io.inInnerStride, dClipIn, inImgSS, pitchIn, cs.dev, S, C, std::max(direct ? 0 : maxSeek, maxRest), st);
	}
	// the engine reads its input on more than one stream (the silence gate on its own): the edge a caller's producer stream gets
	waitForStream(st);
	if (anyRun) {
		if (direct) {
			outputSeek(static_cast<const float *>(io.in), io.inStreamStride, io.inInnerStride, seekLen.data(), run.data());
			process(dClipIn, inImgSS, pitchIn, rest.data(), static_cast<float *>(io.out), io.outStreamStride, io.outInnerStride, procOut.data(), run.data());
		} else {
			outputSeek(dClipIn, inImgSS, pitchIn, seekLen.data(), run.data());
			process(dClipIn + P, inImgSS, pitchIn, rest.data(), dClipOut, outImgSS, pitchOut, procOut.data(), run.data());
		}
		flush(dClipOut + Q, outImgSS, pitchOut, flushN.data(), rates.data(), run.data());
		// the delivered frames of the out-resampled streams, from the finished two-piece image into its third column: in front of every level stage
		if (maxDelivered > 0)
			launchClipResampleOut(dClipOut, outImgSS, pitchOut, dClipOut, outImgSS, pitchOut, outAt.srcSegs(cs.outDev), outAt.dstSegs(cs.outDev), outAt.entries(cs.outDev), S, C,
			                      maxDelivered, maxOutSpanPitch, st);
	}
	// behind the call's last emitting kernel (everything of a call is joined into `st`), in front of whatever synchronize() / signalStream() wait for
	bool wholeClip = false;
	if (io.pcm.level.table && io.wholeClip) for (int s = 0; s < S; ++s) wholeClip = wholeClip || (run[s] && io.wholeClip[s]);
	if (wholeClip) { // the clips' peaks, from the finished image: what kClipOut forms those streams' gains from
		SMST_HIP(hipMemsetAsync(io.pcm.level.clipPeak, 0, (size_t)S*sizeof(int), st));
		launchClipPeak(dClipOut, outImgSS, pitchOut, cs.dev + (size_t)2*S, S, C, std::max(std::max(maxProc, maxFlush), maxDelivered), io.pcm.level.clipPeak, st);
	}
	PcmLevelIo level = io.pcm.level;
	int loudMost = 0, loudSub = 0;
	if (io.pcm.level.table && io.loudHop) for (int s = 0; s < S; ++s) if (run[s] && io.loudHop[s] > 0) { // (a stream in the loudness mode, or a metered one of any mode)
		loudMost = std::max(loudMost, outSamples[s]);
		loudSub = std::max(loudSub, outSamples[s]/io.loudHop[s] + 1);
	}
	if (loudMost > 0) { // the clips' loudness, from the same image: the meters hold what kClipOut forms those streams' gains from
		const int maxChunks = (loudMost + kLoudChunk - 1)/kLoudChunk;
		const size_t doubles = loudScratchDoubles(S, C, maxChunks, loudSub);
		growScratch(dLoud, loudCapacity, 2*doubles, doubles/4 + 1024, true);
		const LoudScratch w = loudScratchAt(reinterpret_cast<double *>(dLoud), S, C, maxChunks, loudSub);
		launchClipLoudness(dClipOut, outImgSS, pitchOut, cs.dev + (size_t)2*S, S, C, io.pcm.loud, io.pcm.loudWeights, w, st);
		level.loudGain = w.gain;
		bool metered = false;
		if (io.loudMeter) for (int s = 0; s < S; ++s) metered = metered || (run[s] && io.loudMeter[s] && io.loudHop[s] > 0);
		if (metered) { // the range and the two maxima, from what the passes left; a capped stream's gain is lowered where kLoudGate wrote it
			const size_t more = loudRangeDoubles(S, loudSub);
			growScratch(dLoudRange, loudRangeCapacity, 2*more, more/4 + 1024, true);
			launchClipLoudnessRange(cs.dev + (size_t)2*S, S, C, io.pcm.loud, io.pcm.loudWeights, w, loudRangeAt(reinterpret_cast<double *>(dLoudRange), S, loudSub), st);
		}
	}
	int truePeakMost = 0;
	if (io.pcm.level.table && io.truePeak) for (int s = 0; s < S; ++s) if (run[s] && io.truePeak[s]) truePeakMost = std::max(truePeakMost, outSamples[s]);
	if (truePeakMost > 0) { // the flagged clips' true peaks, from the same image: what kClipOut forms those streams' whole-clip gains from
		growScratch(dTruePeak, truePeakCapacity, (size_t)S, 0, true);
		int *words = reinterpret_cast<int *>(dTruePeak);
		SMST_HIP(hipMemsetAsync(words, 0, (size_t)S*sizeof(int), st));
		launchClipTruePeak(dClipOut, outImgSS, pitchOut, cs.dev + (size_t)2*S, S, C, truePeakMost, io.pcm.level.table, words, st);
		level.truePeak = words;
	}
	int limitMost = 0;
	if (io.pcm.level.table && io.limiter && !direct) for (int s = 0; s < S; ++s) if (run[s] && io.limiter[s]) limitMost = std::max(limitMost, outSamples[s]);
	if (limitMost > 0) { // the limited clips' gain curves, from the same image: what kClipOut multiplies those streams' frames by
		if (!dLimitWin) throw Error("exact: a limited stream, but the limiter's window has not been prepared");
		const size_t head = (size_t)(2*S + 3)/4*4; // (the meters; need and r begin on 16-byte boundaries)
		const long long pitch = up4(limitMost);
		const size_t rows = (size_t)S*(size_t)pitch;
		growScratch(dLimit, limitCapacity, head + 2*rows, rows/4 + 1024, true);
		int *meters = reinterpret_cast<int *>(dLimit);
		float *need = dLimit + head, *r = need + rows;
		SMST_HIP(hipMemsetAsync(meters, 0, (size_t)2*S*sizeof(int), st));
		launchClipLimit(dClipOut, outImgSS, pitchOut, cs.dev + (size_t)2*S, S, C, limitMost, level, limitH, dLimitWin, need, r, pitch, meters, st);
		level.limit = r;
		level.limitPitch = pitch;
	}
	launchClipOut(io.format, dClipOut, outImgSS, pitchOut, io.out, io.outStreamStride, io.outInnerStride, cs.dev + (size_t)2*S, S, C,
	              std::max(std::max(std::max(direct ? 0 : maxProc, maxFlush), maxZeros), maxDelivered), io.pcm.overs, st, io.pcm.dither, level);
	clipSets.end(st);
	SMST_HIP(hipGetLastError());
	if (tooShort) for (int s = 0; s < S; ++s) if (outSamples[s] >= 0) tooShort[s] = run[s] ? 0 : 1; // (only once every stage has been issued)
}

bool Batch::readLoudness(double *Z, int *counts) {
	if (!dLoud) return false;
	SMST_HIP(hipSetDevice(dev));
	SMST_HIP(hipStreamSynchronize(st));
	const LoudScratch w = loudScratchAt(reinterpret_cast<double *>(dLoud), S, C, 0, 0); // (the meters lie in front, whatever the call's shapes)
	SMST_HIP(hipMemcpy(Z, w.Z, (size_t)S*sizeof(double), hipMemcpyDeviceToHost));
	SMST_HIP(hipMemcpy(counts, w.counts, (size_t)2*S*sizeof(int), hipMemcpyDeviceToHost));
	return true;
}

bool Batch::readLoudnessRange(double *meters, int *counts) {
	if (!dLoudRange) return false;
	SMST_HIP(hipSetDevice(dev));
	SMST_HIP(hipStreamSynchronize(st));
	const LoudRangeScratch r = loudRangeAt(reinterpret_cast<double *>(dLoudRange), S, 0); // (the meters lie in front, whatever the call's shapes)
	SMST_HIP(hipMemcpy(meters, r.meters, (size_t)4*S*sizeof(double), hipMemcpyDeviceToHost));
	SMST_HIP(hipMemcpy(counts, r.counts, (size_t)2*S*sizeof(int), hipMemcpyDeviceToHost));
	return true;
}

bool Batch::readTruePeaks(float *truePeaks) {
	if (!dTruePeak) return false;
	SMST_HIP(hipSetDevice(dev));
	SMST_HIP(hipStreamSynchronize(st));
	SMST_HIP(hipMemcpy(truePeaks, dTruePeak, (size_t)S*sizeof(float), hipMemcpyDeviceToHost));
	return true;
}

void Batch::setLimiterLookahead(int frames) {
	if (frames < 1 || frames > kLimitMaxLookahead) throw Error("limiter: the lookahead is outside 1 ... " + std::to_string(kLimitMaxLookahead) + " frames");
	limitH = frames;
	if (dLimitWin) prepareLimiter();
}

void Batch::prepareLimiter() {
	SMST_HIP(hipSetDevice(dev));
	if (!dLimitWin) {
		dLimitWin = devAlloc<float>((size_t)2*kLimitMaxLookahead + 1);
		wsBytes += ((size_t)2*kLimitMaxLookahead + 1)*sizeof(float);
	}
	std::vector<float> win((size_t)2*limitH + 1);
	limitWindow(limitH, win.data());
	SMST_HIP(hipStreamSynchronize(st)); // (a call in flight reads the window it was issued with)
	SMST_HIP(hipMemcpy(dLimitWin, win.data(), win.size()*sizeof(float), hipMemcpyHostToDevice));
}

// the reduced ratio, checked against the limits of include/smst.h, "Resample" (also smst_resample_ratio's check)
void resampleReduce(int &up, int &down) {
	const std::string limit = std::to_string(kResampleMaxTerm);
	if (up < 1 || down < 1) throw Error("resample: the ratio " + std::to_string(up) + "/" + std::to_string(down) + " has a term below 1 (both are 1 ... " + limit + ")");
	int a = up, b = down;
	while (b) { const int r = a%b; a = b; b = r; }
	up /= a; down /= a;
	if (up > kResampleMaxTerm || down > kResampleMaxTerm)
		throw Error("resample: the reduced ratio " + std::to_string(up) + "/" + std::to_string(down) + " has a term above " + limit + " (SMST_RESAMPLE_MAX_TERM)");
	if (2LL*down > 9LL*up)
		throw Error("resample: the ratio " + std::to_string(up) + "/" + std::to_string(down) + " downsamples by more than 4.5 (2*down <= 9*up)");
	if (2LL*up > 9LL*down)
		throw Error("resample: the ratio " + std::to_string(up) + "/" + std::to_string(down) + " upsamples by more than 4.5 (2*up <= 9*down)");
}

void Batch::setResample(int stream, int up, int down, int setting) {
	if (stream < -1 || stream >= S) throw Error("stream index out of range");
	resampleReduce(up, down);
	std::vector<int> &mine = setting == kResampleStream ? streamResampleSlot : setting == kResampleOut ? outResampleSlot : setting == kResampleStreamOut ? streamOutResampleSlot : resampleSlot; // (a slot's users are the streams of ALL four settings)
	SMST_HIP(hipSetDevice(dev));
	const bool none = up == 1 && down == 1;
	const int first = stream < 0 ? 0 : stream, last = stream < 0 ? S : stream + 1;
	// the slot the ratio has or takes, once the streams named have dropped theirs: refused, before anything changes, where there would be a ninth
	int target = -1;
	if (!none) {
		int users[kResampleMaxRatios];
		for (int k = 0; k < kResampleMaxRatios; ++k) users[k] = resampleSlots[k].users;
		for (int s = first; s < last; ++s) if (mine[s] >= 0) --users[mine[s]];
		for (int k = 0; k < kResampleMaxRatios && target < 0; ++k) if (resampleSlots[k].taps && resampleSlots[k].shape.L == up && resampleSlots[k].shape.M == down) target = k;
		for (int k = 0; k < kResampleMaxRatios && target < 0; ++k) if (users[k] == 0) target = k;
		if (target < 0) throw Error("resample: " + std::to_string(up) + "/" + std::to_string(down) + " would be distinct ratio number " + std::to_string(kResampleMaxRatios + 1) +
		                            " of the batch, at most " + std::to_string(kResampleMaxRatios) + " are live at a time (SMST_RESAMPLE_MAX_RATIOS)");
	}
	for (int s = first; s < last; ++s) if (mine[s] >= 0) { --resampleSlots[mine[s]].users; mine[s] = -1; }
	bool synced = false;
	for (int k = 0; k < kResampleMaxRatios; ++k) { // a ratio that no stream has any more frees its slot (but the one that is about to be taken again)
		ResampleSlot &slot = resampleSlots[k];
		if (!slot.taps || slot.users > 0 || (k == target && slot.shape.L == up && slot.shape.M == down)) continue;
		if (!synced) SMST_HIP(hipStreamSynchronize(st)); // (a call in flight reads the table it was issued with)
		synced = true;
		wsBytes -= (size_t)slot.shape.L*slot.shape.pitch*sizeof(float);
		devFree(slot.taps);
		slot = ResampleSlot();
	}
	if (none) return;
	ResampleSlot &slot = resampleSlots[target];
	if (!slot.taps) { // the first stream with this ratio: the table, built in double and put into device memory here, not in a call
		const ResampleShape g = resampleShapeOf(up, down);
		std::vector<float> taps((size_t)g.L*g.pitch);
		resampleTaps(g, taps.data());
		slot.taps = devAlloc<float>(taps.size());
		slot.shape = g;
		wsBytes += taps.size()*sizeof(float);
		SMST_HIP(hipMemcpy(slot.taps, taps.data(), taps.size()*sizeof(float), hipMemcpyHostToDevice));
	}
	for (int s = first; s < last; ++s) { mine[s] = target; ++slot.users; }
}

void Batch::resampleOf(int stream, int &up, int &down) const {
	if (stream < 0 || stream >= S) throw Error("stream index out of range");
	up = down = 1;
	if (resampleSlot[stream] >= 0) { up = resampleSlots[resampleSlot[stream]].shape.L; down = resampleSlots[resampleSlot[stream]].shape.M; }
}

void Batch::streamResampleOf(int stream, int &up, int &down) const {
	if (stream < 0 || stream >= S) throw Error("stream index out of range");
	up = down = 1;
	if (streamResampleSlot[stream] >= 0) { up = resampleSlots[streamResampleSlot[stream]].shape.L; down = resampleSlots[streamResampleSlot[stream]].shape.M; }
}

void Batch::streamOutResampleOf(int stream, int &up, int &down) const {
	if (stream < 0 || stream >= S) throw Error("stream index out of range");
	up = down = 1;
	if (streamOutResampleSlot[stream] >= 0) { up = resampleSlots[streamOutResampleSlot[stream]].shape.L; down = resampleSlots[streamOutResampleSlot[stream]].shape.M; }
}

void Batch::outResampleOf(int stream, int &up, int &down) const {
	if (stream < 0 || stream >= S) throw Error("stream index out of range");
	up = down = 1;
	if (outResampleSlot[stream] >= 0) { up = resampleSlots[outResampleSlot[stream]].shape.L; down = resampleSlots[outResampleSlot[stream]].shape.M; }
}

long long Batch::outRenderLengthOf(int stream, long long outSamples) const {
	if (stream < 0 || stream >= S) throw Error("stream index out of range");
	if (outResampleSlot[stream] < 0 || outSamples < 0) return outSamples;
	const ResampleShape &g = resampleSlots[outResampleSlot[stream]].shape;
	return resampleRenderLength(outSamples, g.L, g.M);
}

long long Batch::resampledLengthOf(int stream, long long inSamples) const {
	if (stream < 0 || stream >= S) throw Error("stream index out of range");
	if (resampleSlot[stream] < 0 || inSamples < 0) return inSamples;
	const ResampleShape &g = resampleSlots[resampleSlot[stream]].shape;
	return resampledLength(inSamples, g.L, g.M);
}

bool Batch::readLimiter(float *minGain, long long *limitedFrames) {
	if (!dLimit) return false;
	SMST_HIP(hipSetDevice(dev));
	SMST_HIP(hipStreamSynchronize(st));
	std::vector<int> words((size_t)2*S);
	SMST_HIP(hipMemcpy(words.data(), dLimit, words.size()*sizeof(int), hipMemcpyDeviceToHost));
	for (int s = 0; s < S; ++s) {
		const int bits = 0x3f800000 - words[s];
		std::memcpy(minGain + s, &bits, sizeof(float));
		limitedFrames[s] = words[(size_t)S + s];
	}
	return true;
}

// ---- copy -------------------------------------------------------------------------------------------------
void Batch::copyStateFrom(Batch &o) { // every stream of a batch of the same shape (the move checks the rest of the geometry and the device)
	if (o.S != S) throw Error("copyStateFrom: the two batches differ in geometry");
	std::vector<int> all(S);
	for (int s = 0; s < S; ++s) all[s] = s;
	moveStreamsFrom(o, all.data(), all.data(), S);
}

void Batch::moveStreamsFrom(Batch &o, const int *from, const int *to, int n) {
	if (&o == this) throw Error("moveStreamsFrom: source and destination are the same batch");
	if (o.C != C || o.B != B || o.I != I || o.split != split || o.halfState != halfState || o.dev != dev) throw Error("moveStreamsFrom: the two batches differ in geometry or device");
	if (n < 1) return;
	for (int p = 0; p < n; ++p) {
		if (from[p] < 0 || from[p] >= o.S || to[p] < 0 || to[p] >= S) throw Error("moveStreamsFrom: stream index out of range");
		for (int q = 0; q < p; ++q) if (to[q] == to[p]) throw Error("moveStreamsFrom: a destination stream is named twice");
	}
	SMST_HIP(hipSetDevice(dev));
	SMST_HIP(hipStreamSynchronize(o.st));
	SMST_HIP(hipStreamSynchronize(st));
	MoveArgs a{};
	const auto theirs = o.carriedArrays(), mine = carriedArrays();
	for (int i = 0; i < kCarriedArrays; ++i) {
		if (mine[i].splitOnly && !split) continue;
		for (int h = 0; h < mine[i].halves(); ++h) { // the source's current half into both halves
			MoveSeg &g = a.seg[a.nSeg++];
			g.src = theirs[i].current(); g.dst = static_cast<char *>(*mine[i].ptr[h]);
			g.rowBytes = g.srcPitch = g.dstPitch = mine[i].rowBytes;
		}
	}
	std::vector<int> pairs((size_t)2*n);
	for (int p = 0; p < n; ++p) { pairs[2*p] = from[p]; pairs[2*p + 1] = to[p]; }
	int *dPairs = devAlloc<int>(pairs.size());
	SMST_HIP(hipMemcpy(dPairs, pairs.data(), pairs.size()*sizeof(int), hipMemcpyHostToDevice));
	const int kChunk = 32768; // (a grid's z extent)
	for (int p0 = 0; p0 < n; p0 += kChunk) {
		a.pairs = dPairs + 2*(size_t)p0;
		a.nPairs = std::min(kChunk, n - p0);
		launchMoveStreams(a, st);
	}
	SMST_HIP(hipGetLastError());
	SMST_HIP(hipStreamSynchronize(st));
	devFree(dPairs);
	for (int p = 0; p < n; ++p) takeHostRow(o, from[p], to[p]);
	// the streams' own frequency-map tables, knot for knot: every row of the source's pitch fits the (possibly grown) pitch here
	if (o.d.mapTableLen > 0) {
		if (o.d.mapTableLen > d.mapTableLen) growMapTable(o.d.mapTableLen);
		const size_t op = (size_t)o.d.mapTableLen, pitch = (size_t)d.mapTableLen;
		for (int p = 0; p < n; ++p)
			for (int slot = 0; slot < kMapSlots; ++slot) {
				float *dstRow = hostMapTable.data() + ((size_t)to[p]*kMapSlots + slot)*pitch;
				const float *srcRow = o.hostMapTable.data() + ((size_t)from[p]*kMapSlots + slot)*op;
				std::copy(srcRow, srcRow + op, dstRow);
				std::fill(dstRow + op, dstRow + pitch, 0.0f);
			}
		uploadMapTable();
	}
}

void Batch::inheritAcrossConfigure(Batch &o) {
	if (o.S != S) throw Error("inheritAcrossConfigure: stream counts differ");
	SMST_HIP(hipSetDevice(o.dev));
	SMST_HIP(hipStreamSynchronize(o.st));
	const CarriedArray theirs = o.carriedArrays()[kStFreq], mine = carriedArrays()[kStFreq];
	std::vector<char> freq((size_t)S*mine.rowBytes);
	SMST_HIP(hipMemcpy(freq.data(), theirs.current(), freq.size(), hipMemcpyDeviceToHost));
	SMST_HIP(hipSetDevice(dev));
	SMST_HIP(hipStreamSynchronize(st));
	SMST_HIP(hipMemcpy(mine.current(), freq.data(), freq.size(), hipMemcpyHostToDevice));
	for (int s = 0; s < S; ++s) {
		const StreamSched &from = o.sched[s];
		StreamSched &to = sched[s];
		to.seed = o.seedAfterDroppedBlock(s); // (configure() drops a block in flight: blockProcess = {}, :89)
		to.prevInputOffset = from.prevInputOffset;
		to.didSeek = from.didSeek;
		to.seekTimeFactor = from.seekTimeFactor;
		to.silenceCounter = from.silenceCounter;
		to.silenceFirst = from.silenceFirst;
	}
}

// ---- test hooks -------------------------------------------------------------------------------------------
void Batch::debugGetState(int stream, int which, float *dst) {
	SMST_HIP(hipSetDevice(dev));
	SMST_HIP(hipStreamSynchronize(st));
	const StatePlane p = statePlane(stream, which);
	debugCopy(false, p.row, dst, 1, p.values, p.values, p.narrowed, p.root);
}
void Batch::debugSetState(int stream, int which, const float *src) {
	const StatePlane p = statePlane(stream, which);
	SMST_HIP(hipSetDevice(dev));
	SMST_HIP(hipStreamSynchronize(st));
	debugCopy(true, p.row, const_cast<float *>(src), 1, p.values, p.values, p.narrowed, p.root);
}
Batch::StatePlane Batch::statePlane(int stream, int which) { // 0 input, 1 prevInput, 2 output: 2*C*M floats; 3 energy: C*M, kept as its square root in fp16
	static_assert(kStInput == 0 && kStPrev == 1 && kStOut == 2 && kStEnergy == 3, "the debug selectors are the list's first entries");
	if (stream < 0 || stream >= S || which < 0 || which > 3) throw Error("debug state: bad stream / selector");
	const CarriedArray a = carriedArrays()[which];
	return StatePlane{a.current() + (size_t)stream*a.rowBytes, (size_t)C*M*(which == kStEnergy ? 1 : 2), a.narrowed, which == kStEnergy};
}
// fp16 storage widens / narrows on the host
void Batch::debugCopy(bool set, void *device, float *host, size_t rows, size_t len, size_t devPitch, bool narrowed, bool root) {
	const size_t width = narrowed ? sizeof(half_t) : sizeof(float);
	std::vector<half_t> tmp(narrowed ? rows*len : 0);
	if (narrowed && set) for (size_t i = 0; i < tmp.size(); ++i) tmp[i] = half_t(root ? std::sqrt(std::max(host[i], 0.0f)) : host[i]);
	void *packed = narrowed ? static_cast<void *>(tmp.data()) : host;
	if (rows == 1) SMST_HIP(hipMemcpy(set ? device : packed, set ? packed : device, len*width, set ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost));
	else if (set) SMST_HIP(hipMemcpy2D(device, devPitch*width, packed, len*width, len*width, rows, hipMemcpyHostToDevice));
	else SMST_HIP(hipMemcpy2D(packed, len*width, device, devPitch*width, len*width, rows, hipMemcpyDeviceToHost));
	if (narrowed && !set) for (size_t i = 0; i < tmp.size(); ++i) { const float v = float(tmp[i]); host[i] = root ? v*v : v; }
}
// [C] rows of B+I sums, carryPitch apart on the device, and one of products
void Batch::debugSetCarry(int stream, const float *sums, const float *products) { debugCarry(true, stream, const_cast<float *>(sums), const_cast<float *>(products)); }
void Batch::debugGetCarry(int stream, float *sums, float *products) { debugCarry(false, stream, sums, products); }
void Batch::debugCarry(bool set, int stream, float *sums, float *products) {
	if (stream < 0 || stream >= S) throw Error("debug carry: bad stream");
	SMST_HIP(hipSetDevice(dev));
	SMST_HIP(hipStreamSynchronize(st));
	settleCarry();
	SMST_HIP(hipStreamSynchronize(st));
	const auto list = carriedArrays();
	const CarriedArray &sum = list[kCarrySum], &wp = list[kCarryWp];
	debugCopy(set, sum.current() + (size_t)stream*sum.rowBytes, sums, C, d.carryLen, d.carryPitch, sum.narrowed, false);
	debugCopy(set, wp.current() + (size_t)stream*wp.rowBytes, products, 1, d.carryLen, d.carryPitch, false, false);
}
bool Batch::debugGetMap(int stream, float *dst) {
	if (stream < 0 || stream >= S) throw Error("debugGetMap: bad stream");
	const LastHop &lh = lastHop[stream];
	if (lh.slot < 0 || !lh.mapped) return false;
	SMST_HIP(hipSetDevice(dev));
	SMST_HIP(hipStreamSynchronize(st));
	SMST_HIP(hipMemcpy(dst, slots[lh.slot].map + ((size_t)lh.subLocal*d.T + lh.local)*M, (size_t)M*sizeof(float2), hipMemcpyDeviceToHost));
	return true;
}
bool Batch::debugGetFormants(int stream, float *ratio, float *envelope, float *freqEstimate) {
	if (stream < 0 || stream >= S) throw Error("debugGetFormants: bad stream");
	const LastHop &lh = lastHop[stream];
	if (lh.slot < 0 || !lh.formants || !slots[lh.slot].envelope) return false;
	SMST_HIP(hipSetDevice(dev));
	SMST_HIP(hipStreamSynchronize(st));
	const size_t row = (size_t)lh.subLocal*d.T + lh.local;
	SMST_HIP(hipMemcpy(ratio, slots[lh.slot].ratio + row*M, (size_t)M*sizeof(float), hipMemcpyDeviceToHost));
	SMST_HIP(hipMemcpy(envelope, slots[lh.slot].envelope + row*M, (size_t)M*sizeof(float), hipMemcpyDeviceToHost));
	SMST_HIP(hipMemcpy(freqEstimate, slots[lh.slot].freqEst + row, sizeof(float), hipMemcpyDeviceToHost));
	return true;
}
} // namespace smst
