// TEST INFRASTRUCTURE ONLY -- see tests/emu/hip/hip_runtime.h.
// Runs each workgroup's threads as ucontext fibers, round-robin between barriers.
#include <hip/hip_runtime.h>
#include <ucontext.h>
#include <cstdint>
#include <cstdio>
#include <deque>
#include <map>
#include <random>
#include <string>
#include <vector>
#include <stdexcept>

EmuIdx threadIdx, blockIdx, blockDim, gridDim;
// (behind the CU's 160 KB: room for the guard that emuLaunch lays behind every request)
constexpr size_t kLdsBytes = 160*1024, kLdsGuardBytes = 4096;
namespace smst { alignas(16) unsigned char smemRaw[kLdsBytes + kLdsGuardBytes]; }

// Context switches: a workgroup of 1024 fibers yields at every barrier, poll and s_sleep -- tens of millions of switches per test run.  glibc's
// swapcontext() makes a signal-mask system call per switch (the CPU suite spent 4 min 54 s of 8 min 23 s in the kernel); the switch below saves
// and restores the callee-saved registers and the stack pointer, nothing else (x86-64 System V).  The sanitizer build keeps swapcontext(), which
// AddressSanitizer intercepts and understands.
#if defined(__x86_64__) && !defined(__SANITIZE_ADDRESS__)
#define EMU_FAST_SWITCH 1
extern "C" void emuSwitch(void **saveSp, void *newSp);
asm(R"(
.text
.globl emuSwitch
.type emuSwitch,@function
emuSwitch:
	pushq %rbp
	pushq %rbx
	pushq %r12
	pushq %r13
	pushq %r14
	pushq %r15
	movq %rsp, (%rdi)
	movq %rsi, %rsp
	popq %r15
	popq %r14
	popq %r13
	popq %r12
	popq %rbx
	popq %rbp
	ret
.size emuSwitch, .-emuSwitch
)");
#endif

namespace {
struct Fiber {
#ifdef EMU_FAST_SWITCH
	void *sp = nullptr;
#else
	ucontext_t ctx;
#endif
	std::vector<unsigned char> stack;
	bool done = false;
	EmuIdx tid;
};
#ifdef EMU_FAST_SWITCH
void *schedulerSp = nullptr;
#else
ucontext_t schedulerCtx;
#endif
Fiber *current = nullptr;
const std::function<void()> *currentBody = nullptr;

void toScheduler() {
#ifdef EMU_FAST_SWITCH
	emuSwitch(&current->sp, schedulerSp);
#else
	swapcontext(&current->ctx, &schedulerCtx);
#endif
}
void fiberEntry() {
	(*currentBody)();
	current->done = true;
	toScheduler();
}
#ifdef EMU_FAST_SWITCH
extern "C" void emuFiberStart() { fiberEntry(); __builtin_trap(); } // (a finished fiber is never resumed)
void prepare(Fiber &f) {
	// the first switch into the fiber pops six registers and returns into emuFiberStart with the stack aligned as after a call
	uintptr_t top = (reinterpret_cast<uintptr_t>(f.stack.data()) + f.stack.size()) & ~uintptr_t(15);
	void **sp = reinterpret_cast<void **>(top - 8);
	*--sp = reinterpret_cast<void *>(&emuFiberStart);
	for (int i = 0; i < 6; ++i) *--sp = nullptr;
	f.sp = sp;
}
void resume(Fiber &f) { emuSwitch(&schedulerSp, f.sp); }
#else
void prepare(Fiber &f) {
	getcontext(&f.ctx);
	f.ctx.uc_stack.ss_sp = f.stack.data();
	f.ctx.uc_stack.ss_size = f.stack.size();
	f.ctx.uc_link = &schedulerCtx;
	makecontext(&f.ctx, fiberEntry, 0);
}
void resume(Fiber &f) { swapcontext(&schedulerCtx, &f.ctx); }
#endif
}

void emuSyncThreads() {
	toScheduler();
}

// A workgroup whose threads keep yielding without finishing (a poll that nothing in its own workgroup will ever satisfy) ends the
// process with the kernel's name instead of hanging the suite.  The largest legitimate count in the CPU suite is far below this.
static long maxRounds() {
	static const long v = [] { const char *e = std::getenv("SMST_EMU_MAX_ROUNDS"); return e ? std::atol(e) : (1l << 22); }();
	return v;
}

void emuLaunch(dim3 grid, dim3 block, size_t ldsBytes, const std::function<void()> &body, const char *name) {
	if (ldsBytes > kLdsBytes) throw std::runtime_error("emu: LDS request too large");
	// On the device an LDS write past what the launcher asked for is dropped silently.  Here the bytes behind the request carry a pattern
	// that must still stand after the launch: "the kernel writes nothing past what its launcher asked for", for every kernel of the library.
	auto guardByte = [](size_t i) { return (unsigned char)(0xA5u ^ (i*37u)); };
	for (size_t i = 0; i < kLdsGuardBytes; ++i) smst::smemRaw[ldsBytes + i] = guardByte(i);
	const unsigned nThreads = block.x*block.y*block.z;
	static std::vector<Fiber> fibers;
	if (fibers.size() < nThreads) fibers.resize(nThreads);
	for (unsigned i = 0; i < nThreads; ++i) if (fibers[i].stack.empty()) fibers[i].stack.resize(256*1024);
	currentBody = &body;
	gridDim = {grid.x, grid.y, grid.z};
	blockDim = {block.x, block.y, block.z};
	for (unsigned bz = 0; bz < grid.z; ++bz) for (unsigned by = 0; by < grid.y; ++by) for (unsigned bx = 0; bx < grid.x; ++bx) {
		for (unsigned i = 0; i < nThreads; ++i) {
			Fiber &f = fibers[i];
			f.done = false;
			f.tid = {i%block.x, (i/block.x)%block.y, i/(block.x*block.y)};
			prepare(f);
		}
		bool anyAlive = true;
		for (long rounds = 0; anyAlive; ++rounds) {
			if (rounds > maxRounds()) {
				std::fprintf(stderr, "emu: kernel %s, workgroup (%u, %u, %u): still polling after %ld rounds -- it waits for something only "
				             "another kernel could provide\n", name, bx, by, bz, rounds);
				std::abort();
			}
			anyAlive = false;
			for (unsigned i = 0; i < nThreads; ++i) {
				Fiber &f = fibers[i];
				if (f.done) continue;
				current = &f;
				threadIdx = f.tid;
				blockIdx = {bx, by, bz};
				resume(f);
				if (!f.done) anyAlive = true;
			}
		}
	}
	for (size_t i = 0; i < kLdsGuardBytes; ++i) {
		if (smst::smemRaw[ldsBytes + i] != guardByte(i))
			throw std::runtime_error(std::string("emu: kernel ") + name + " wrote LDS byte " + std::to_string(ldsBytes + i) + ", its launcher asked for " + std::to_string(ldsBytes));
	}
}

// ---- wave-level collectives (votes span the block and are only used by single-wave kernels): every lane deposits its value, yields once so that
// all lanes of the block have deposited, then reads.  Two alternating banks keep back-to-back collectives apart.
namespace {
float shflBankF[2][1024];
int shflBankI[2][1024];
bool anyBank[2][1024];
int collectiveSeq[1024];
}
static int laneIndex() { return (int)(threadIdx.x + blockDim.x*(threadIdx.y + blockDim.y*threadIdx.z)); }
bool emuAny(bool v) {
	const int me = laneIndex(), bank = collectiveSeq[me]++ & 1;
	anyBank[bank][me] = v;
	emuSyncThreads();
	bool r = false; // a wave-level vote: the 64 lanes of the caller's own wave (other waves may not be voting at all)
	const int n = (int)(blockDim.x*blockDim.y*blockDim.z), w0 = me & ~63;
	for (int i = w0; i < w0 + 64 && i < n; ++i) r = r || anyBank[bank][i];
	emuSyncThreads();
	return r;
}
float emuShflF(float v, int lane) {
	const int me = laneIndex(), bank = collectiveSeq[me]++ & 1;
	shflBankF[bank][me] = v;
	emuSyncThreads();
	float r = shflBankF[bank][(me & ~63) + (lane & 63)]; // source lane within the caller's own wave
	emuSyncThreads();
	return r;
}
int emuShflI(int v, int lane) {
	const int me = laneIndex(), bank = collectiveSeq[me]++ & 1;
	shflBankI[bank][me] = v;
	emuSyncThreads();
	int r = shflBankI[bank][(me & ~63) + (lane & 63)];
	emuSyncThreads();
	return r;
}

// DPP wave_shr:1 (the only control the product uses): lane i of a 64-lane wave receives lane i-1's value, lane 0 keeps
// `old`.  Lanes of a wave run consecutively in index order between yields, so lane i-1 has always executed the same
// call instance already: a per-lane ring indexed by the call counter needs no yield (at most 512 calls per lane happen
// between two yields of the recurrence wave).
namespace { int dppRing[1024][1024]; unsigned dppSeq[1024]; }
int emuDppShr1(int old, int v) {
	const int me = laneIndex();
	const unsigned seq = dppSeq[me]++ & 1023u;
	dppRing[me][seq] = v;
	return (me & 63) ? dppRing[me - 1][seq] : old;
}

// ---- streams and events: the documented HIP ordering contract, with three schedules (see tests/emu/hip/hip_runtime.h) ----------------
struct EmuEvent;
namespace {
enum Schedule { EAGER, LAZY, RANDOM };
struct Op {
	std::function<void()> fn;        // a kernel, copy or memset (empty: a wait)
	struct EmuStream *waitStream = nullptr;
	uint64_t waitSeq = 0;
	EmuEvent *waitEvent = nullptr;   // only where waits bind late (the rule switched off by a self-test)
};
}
struct EmuStream {
	std::deque<Op> q;
	uint64_t enqueued = 0, done = 0; // operations ever enqueued / run: an event record is the value of `enqueued` at the record
	Schedule mode = EAGER;
	bool live = true;
	uint64_t id = 0;                 // creation order: a seed gives the same order in every run, wherever the streams live
};
struct EmuEvent {
	EmuStream *stream = nullptr;     // null: never recorded
	uint64_t seq = 0;
};
namespace {
// Rules of the contract that the model's self-test switches off one at a time, to show that each one is what a test relies on.
struct Rules {
	bool waits = true;             // hipStreamWaitEvent orders the waiting stream
	bool bindAtWait = true;        // ... after the event's record as of the wait CALL (off: as of when the wait executes)
	bool pinnedAtExecution = true; // an async copy reads / writes hipHostMalloc memory when it runs (off: staged at enqueue)
} rules;
std::vector<EmuStream *> streams;  // live streams
std::mt19937_64 rng(0);
bool haveOverride = false;
Schedule overrideMode = EAGER;
std::string envSeen;
Schedule envMode = EAGER;
std::map<uintptr_t, size_t> deviceRanges, pinnedRanges;
long long pageableAsyncCopies = 0; // hipMemcpyAsync calls on a stream whose source is neither device nor hipHostMalloc memory, under every schedule

bool parseSchedule(const char *spec, Schedule &mode, uint64_t &seed, bool &seeded) {
	const std::string v = spec ? spec : "";
	seeded = false;
	if (v.empty() || v == "eager") { mode = EAGER; return true; }
	if (v == "lazy") { mode = LAZY; return true; }
	if (v.rfind("random", 0) == 0) {
		mode = RANDOM;
		seed = 0;
		if (v.size() > 6) {
			if (v[6] != ':' || v.size() == 7) return false;
			char *end = nullptr;
			seed = std::strtoull(v.c_str() + 7, &end, 10);
			if (*end) return false;
		}
		seeded = true;
		return true;
	}
	return false;
}
Schedule scheduleForNewStream() {
	if (haveOverride) return overrideMode;
	const char *e = std::getenv("SMST_EMU_SCHEDULE");
	const std::string v = e ? e : "";
	if (v != envSeen || streams.empty()) {
		// (re)read: a random schedule starts its generator from its seed whenever the variable changes
		uint64_t seed = 0;
		bool seeded = false;
		if (!parseSchedule(e, envMode, seed, seeded)) {
			std::fprintf(stderr, "emu: SMST_EMU_SCHEDULE=%s: expected eager, lazy or random:<seed>\n", e);
			std::abort();
		}
		if (seeded && v != envSeen) rng.seed(seed);
		envSeen = v;
	}
	return envMode;
}
bool inRange(const std::map<uintptr_t, size_t> &m, const void *p) {
	const uintptr_t a = reinterpret_cast<uintptr_t>(p);
	auto it = m.upper_bound(a);
	if (it == m.begin()) return false;
	--it;
	return a < it->first + it->second;
}

bool ready(const Op &op) {
	if (op.fn) return true;
	if (op.waitEvent) return !op.waitEvent->stream || op.waitEvent->stream->done >= op.waitEvent->seq;
	return op.waitStream->done >= op.waitSeq;
}
void runHead(EmuStream *s) {
	Op op = std::move(s->q.front());
	s->q.pop_front();
	if (op.fn) op.fn();
	++s->done;
}
// lazy: run exactly what `s` up to `seq` depends on -- its own earlier work, and through its waits the work of other streams
void drainTo(EmuStream *s, uint64_t seq) {
	while (s->done < seq) {
		Op &op = s->q.front();
		if (!op.fn) {
			EmuStream *ws = op.waitEvent ? op.waitEvent->stream : op.waitStream;
			const uint64_t wseq = op.waitEvent ? op.waitEvent->seq : op.waitSeq;
			if (ws && ws != s) drainTo(ws, wseq);
		}
		runHead(s);
	}
}
// random: the work that the host-blocking call needs (`need`: per stream, how many of its operations must have run), closed over the
// event edges, in a seeded random order that keeps each stream's order and the edges.  What the call does not need stays queued, as
// under lazy, and may run in any order later: a join that is missing leaves its work behind in every seed
void drainRandom(std::map<EmuStream *, uint64_t> need) {
	for (bool grew = true; grew;) { // close over the waits in front of what is needed
		grew = false;
		for (auto &kv : std::map<EmuStream *, uint64_t>(need)) {
			EmuStream *s = kv.first;
			for (uint64_t i = s->done; i < kv.second; ++i) {
				const Op &op = s->q[i - s->done];
				if (op.fn) continue;
				EmuStream *ws = op.waitEvent ? op.waitEvent->stream : op.waitStream;
				const uint64_t wseq = op.waitEvent ? op.waitEvent->seq : op.waitSeq;
				if (ws && ws != s && need[ws] < wseq) { need[ws] = wseq; grew = true; }
			}
		}
	}
	std::vector<EmuStream *> candidates;
	for (;;) {
		candidates.clear();
		bool any = false;
		for (auto &kv : need) {
			if (kv.first->done >= kv.second) continue;
			any = true;
			if (ready(kv.first->q.front())) candidates.push_back(kv.first);
		}
		if (!any) return;
		if (candidates.empty()) { std::fprintf(stderr, "emu: queued work waits on itself\n"); std::abort(); }
		std::sort(candidates.begin(), candidates.end(), [](const EmuStream *a, const EmuStream *b) { return a->id < b->id; });
		runHead(candidates[rng() % candidates.size()]);
	}
}
void hostWaitsFor(EmuStream *s, uint64_t seq) {
	if (s->mode == RANDOM) drainRandom({{s, seq}});
	else drainTo(s, seq);
}
void enqueue(EmuStream *s, Op op) {
	s->q.push_back(std::move(op));
	++s->enqueued;
	if (s->mode == EAGER) drainTo(s, s->enqueued);
}
void deviceSynchronize() {
	std::map<EmuStream *, uint64_t> all;
	for (EmuStream *s : streams) if (s->mode == RANDOM) all[s] = s->enqueued;
	if (!all.empty()) drainRandom(all);
	for (EmuStream *s : streams) drainTo(s, s->enqueued);
}
} // namespace

void emuEnqueue(hipStream_t stream, const char *, std::function<void()> fn) {
	if (!stream) { fn(); return; } // the null stream: only the synchronous copies and the complex self-test use it, each followed by a blocking copy
	Op op;
	op.fn = std::move(fn);
	enqueue(stream, std::move(op));
}

hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) {
	static uint64_t created = 0;
	EmuStream *n = new EmuStream;
	n->mode = scheduleForNewStream();
	n->id = created++;
	streams.push_back(n);
	*s = n;
	return 0;
}
hipError_t hipStreamCreateWithPriority(hipStream_t *s, unsigned flags, int) { return hipStreamCreateWithFlags(s, flags); }
hipError_t hipStreamDestroy(hipStream_t s) {
	if (!s || !s->live) return 0;
	hostWaitsFor(s, s->enqueued); // (queued work still completes)
	s->live = false;
	streams.erase(std::find(streams.begin(), streams.end(), s));
	// the object stays: a wait of another stream may still name it (it is complete, so such a wait is satisfied)
	return 0;
}
hipError_t hipStreamSynchronize(hipStream_t s) {
	if (!s) return hipDeviceSynchronize();
	hostWaitsFor(s, s->enqueued);
	return 0;
}
hipError_t hipDeviceSynchronize() { deviceSynchronize(); return 0; }

hipError_t hipMalloc(void **p, size_t n) {
	*p = std::calloc(n ? n : 1, 1);
	if (!*p) return 2;
	deviceRanges[reinterpret_cast<uintptr_t>(*p)] = n ? n : 1;
	return 0;
}
hipError_t hipFree(void *p) {
	if (!p) return 0;
	deviceSynchronize(); // as HIP's hipFree does
	deviceRanges.erase(reinterpret_cast<uintptr_t>(p));
	std::free(p);
	return 0;
}
hipError_t hipHostMalloc(void **p, size_t n, unsigned) {
	*p = std::calloc(n ? n : 1, 1);
	if (!*p) return 2;
	pinnedRanges[reinterpret_cast<uintptr_t>(*p)] = n ? n : 1;
	return 0;
}
hipError_t hipHostFree(void *p) {
	if (!p) return 0;
	deviceSynchronize();
	pinnedRanges.erase(reinterpret_cast<uintptr_t>(p));
	std::free(p);
	return 0;
}
hipError_t hipMemcpyAsync(void *d, const void *s, size_t n, hipMemcpyKind, hipStream_t stream) {
	if (!stream || n == 0) { if (n) std::memcpy(d, s, n); return 0; }
	// Device and pinned memory are read and written when the copy runs.  A pageable source is staged at enqueue (HIP may copy it
	// through a staging buffer at once); a pageable destination is written when the copy runs, so the host must still wait for it.
	const bool late = inRange(deviceRanges, s) || (rules.pinnedAtExecution && inRange(pinnedRanges, s));
	if (!inRange(deviceRanges, s) && !inRange(pinnedRanges, s)) ++pageableAsyncCopies; // (the model cannot see a too-early rewrite of such a source)
	if (late || stream->mode == EAGER) emuEnqueue(stream, "copy", [d, s, n]() { std::memcpy(d, s, n); });
	else {
		std::vector<unsigned char> staged(static_cast<const unsigned char *>(s), static_cast<const unsigned char *>(s) + n);
		emuEnqueue(stream, "copy", [d, staged]() { std::memcpy(d, staged.data(), staged.size()); });
	}
	return 0;
}
hipError_t hipMemsetAsync(void *d, int v, size_t n, hipStream_t stream) {
	emuEnqueue(stream, "memset", [d, v, n]() { std::memset(d, v, n); });
	return 0;
}

hipError_t hipEventCreate(hipEvent_t *e) { *e = new EmuEvent; return 0; }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { return hipEventCreate(e); }
hipError_t hipEventDestroy(hipEvent_t e) {
	if (e && rules.bindAtWait) delete e; // (a late-binding wait keeps a pointer to its event)
	return 0;
}
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) {
	if (!s) { deviceSynchronize(); e->stream = nullptr; return 0; } // (the null stream: everything before is complete)
	e->stream = s;
	e->seq = s->enqueued;
	return 0;
}
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned) {
	if (!rules.waits || !s) return 0;
	Op op;
	if (rules.bindAtWait) {
		if (!e->stream || e->stream == s) return 0; // never recorded: no wait at all (and a stream is ordered after itself)
		op.waitStream = e->stream;
		op.waitSeq = e->seq;
	} else {
		op.waitEvent = e;
	}
	enqueue(s, std::move(op));
	return 0;
}
hipError_t hipEventSynchronize(hipEvent_t e) {
	if (e->stream) hostWaitsFor(e->stream, e->seq);
	return 0;
}

// ---- test hooks (C ABI, for ctypes): schedules, the model's rules, and a caller's own streams --------------------------------------
extern "C" {
// spec: "eager", "lazy", "random:<seed>", or null / "" to go back to SMST_EMU_SCHEDULE.  Applies to streams created from now on; a
// random schedule restarts its generator from the seed.  Returns 0, or -1 for a spec it does not know.
int smst_emu_set_schedule(const char *spec) {
	if (!spec || !*spec) { haveOverride = false; return 0; }
	Schedule m;
	uint64_t seed;
	bool seeded;
	if (!parseSchedule(spec, m, seed, seeded)) return -1;
	haveOverride = true;
	overrideMode = m;
	if (seeded) rng.seed(seed);
	return 0;
}
// name: "waits", "bind_at_wait", "pinned_at_execution"; returns the previous value, or -1 for an unknown name
int smst_emu_set_rule(const char *name, int on) {
	const std::string n = name ? name : "";
	bool *r = n == "waits" ? &rules.waits : n == "bind_at_wait" ? &rules.bindAtWait : n == "pinned_at_execution" ? &rules.pinnedAtExecution : nullptr;
	if (!r) return -1;
	const int old = *r;
	*r = on != 0;
	return old;
}
void *smst_emu_stream_create() { hipStream_t s; hipStreamCreateWithFlags(&s, hipStreamNonBlocking); return s; }
void smst_emu_stream_destroy(void *s) { hipStreamDestroy(static_cast<hipStream_t>(s)); }
int smst_emu_stream_synchronize(void *s) { return hipStreamSynchronize(static_cast<hipStream_t>(s)); }
int smst_emu_device_synchronize() { return hipDeviceSynchronize(); }
void *smst_emu_event_create() { hipEvent_t e; hipEventCreate(&e); return e; }
void smst_emu_event_destroy(void *e) { hipEventDestroy(static_cast<hipEvent_t>(e)); }
int smst_emu_event_record(void *e, void *s) { return hipEventRecord(static_cast<hipEvent_t>(e), static_cast<hipStream_t>(s)); }
int smst_emu_stream_wait_event(void *s, void *e) { return hipStreamWaitEvent(static_cast<hipStream_t>(s), static_cast<hipEvent_t>(e), 0); }
int smst_emu_event_synchronize(void *e) { return hipEventSynchronize(static_cast<hipEvent_t>(e)); }
int smst_emu_memcpy_async(void *dst, const void *src, size_t n, void *s) { return hipMemcpyAsync(dst, src, n, hipMemcpyDefault, static_cast<hipStream_t>(s)); }
void *smst_emu_host_malloc(size_t n) { void *p = nullptr; hipHostMalloc(&p, n, 0); return p; }
void smst_emu_host_free(void *p) { hipHostFree(p); }
// a caller's buffer that stands for device memory (SMST_MEM_DEVICE): async copies read it when they run
void smst_emu_register_device(void *p, size_t n) { deviceRanges[reinterpret_cast<uintptr_t>(p)] = n; }
void smst_emu_unregister_device(void *p) { deviceRanges.erase(reinterpret_cast<uintptr_t>(p)); }
// an operation on `s` that writes the running count of such operations to *slot when it runs: the order in which work ran
void smst_emu_enqueue_tick(void *s, int *slot) {
	static int ticks = 0;
	emuEnqueue(static_cast<hipStream_t>(s), "tick", [slot]() { *slot = ++ticks; });
}
// async copies from pageable memory since the library was loaded: the engine's calling paths make none (csrc/smst_staging.h)
long long smst_emu_pageable_async_copies() { return pageableAsyncCopies; }
// operations queued on all live streams and not run yet
long long smst_emu_queued() {
	long long n = 0;
	for (EmuStream *s : streams) n += (long long)s->q.size();
	return n;
}
}
