"""Timing experiment (results wrong by construction): kAnalyseFast computes its spectra and stores almost none of them."""
import sys
p = sys.argv[1] + '/smst_kernels.hip'
s = open(p).read()
i = s.index('void kAnalyseFast(')
old = "	auto store = [&](int j, float2 u, int, int) { storeHalfBin(dst, j, u, H, N); };\n"
assert s.count(old, i) == 1
new = "	auto store = [&](int j, float2 u, int, int) { if (u.x == 1234.5f) storeHalfBin(dst, j, u, H, N); };\n"
open(p, 'w').write(s[:i] + s[i:].replace(old, new))
