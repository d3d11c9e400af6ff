"""Experiment: the register-blocked FFT kernels at THREE waves per SIMD (<= 168 VGPRs, three 26-KB workgroups per CU) instead of four."""
import sys
p = sys.argv[1] + '/smst_kernels.hip'
s = open(p).read()
old = "__global__ __launch_bounds__(fastBlockThreads(R3)) __attribute__((amdgpu_waves_per_eu(4, 4))) void kAnalyseFast("
assert s.count(old) == 1
s = s.replace(old, "__global__ __launch_bounds__(fastBlockThreads(R3)) __attribute__((amdgpu_waves_per_eu(3, 3))) void kAnalyseFast(")
old = "__global__ __launch_bounds__(fastBlockThreads(R3)) void kSynthFast("
assert s.count(old) == 1
s = s.replace(old, "__global__ __launch_bounds__(fastBlockThreads(R3)) __attribute__((amdgpu_waves_per_eu(3, 3))) void kSynthFast(")
open(p, 'w').write(s)
