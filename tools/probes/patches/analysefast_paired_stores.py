"""Timing experiment (results wrong by construction): kAnalyseFast stores 64 lanes x 8 bytes CONTIGUOUSLY (dst[j]) instead of
interleaving even and odd bins at a 16-byte stride."""
import sys
p = sys.argv[1] + '/smst_kernels.hip'
s = open(p).read()
i = s.index('void kAnalyseFast(')
old = "	auto store = [&](int j, float2 u, int, int) { storeHalfBin(dst, j, u, H, N); };\n"
assert s.count(old, i) == 1
new = "	auto store = [&](int j, float2 u, int, int) { dst[j] = u; };\n"
open(p, 'w').write(s[:i] + s[i:].replace(old, new))
