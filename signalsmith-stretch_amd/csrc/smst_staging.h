// A table set that exists twice: what a call hands to the device in tables -- pinned host staging with a device twin -- may still be read by
// the kernels of the call before when the next call fills its own.  So every such set exists twice, and a call takes the one that the call
// BEFORE THE PREVIOUS one used, once the event recorded behind that call's last reader has passed.  The one rotate / wait / record protocol
// of the engine and the C ABI:
//   Set &t = sets.begin();    // the other set; waits until its last user's kernels have run
//   ... fill t's pinned staging, upload it with hipMemcpyAsync on the stream, launch what reads the device twin ...
//   sets.end(stream);         // behind the last reader
// begin() / end() pairs of one TwoSets never nest.  Nothing pageable is handed to an async copy, so a buffer that the host rewrites is always
// one that the device has finished with -- and tests/emu's stream model can see it if it is not (rule pinned_at_execution).
#pragma once
#include <chrono>
#include <hip/hip_runtime.h>

namespace smst {

[[noreturn]] void throwDeviceError(const char *call, hipError_t e); // smst::Error of a failed HIP runtime call (smst_engine.cpp)

template <typename Tables> class TwoSets {
public:
	struct Set : Tables { hipEvent_t done = nullptr; bool used = false; };
	Set sets[2]{};
	TwoSets() {}
	TwoSets(const TwoSets &) = delete;
	TwoSets &operator=(const TwoSets &) = delete;
	~TwoSets() { for (Set &s : sets) if (s.done) hipEventDestroy(s.done); } // (the owner has selected the device)
	void create() { // the events; what the tables point to is the owner's to allocate
		for (Set &s : sets) if (!s.done) check("hipEventCreateWithFlags", hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
	}
	// waitMs (may be null): the time spent waiting for the device is added to it
	Set &begin(double *waitMs = nullptr) {
		cur ^= 1;
		Set &s = sets[cur];
		if (s.used) {
			const auto t0 = std::chrono::steady_clock::now();
			check("hipEventSynchronize", hipEventSynchronize(s.done));
			if (waitMs) *waitMs += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
		}
		s.used = false;
		return s;
	}
	void end(hipStream_t stream) {
		check("hipEventRecord", hipEventRecord(sets[cur].done, stream));
		sets[cur].used = true;
	}
	Set &other() { return sets[cur ^ 1]; } // the set of the previous call (its kernels may still be running)
private:
	int cur = 0;
	static void check(const char *call, hipError_t e) { if (e != hipSuccess) throwDeviceError(call, e); }
};

} // namespace smst
