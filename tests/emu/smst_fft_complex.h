// TEST INFRASTRUCTURE ONLY: the CPU stand-in's version of signalsmith-stretch_amd/csrc/smst_fft_complex.h (the product header is gfx950
// inline assembly on packed register pairs).  Same operations on the same operands in the same order, as the C++ expressions the FFT
// kernels were written in before that header.  The stand-in's compiler contracts nothing (plain x86-64: no fused multiply-add), so where
// the device fuses the first product of `p*q -+ r*s` into the sum, every product here is rounded on its own -- as it always was on
// the stand-in: its results are those of the commit before the header, bit for bit (tests/golden/fft_core_parent_emu.json).
// tests/fft_core_cases.py holds both forms of the expectation.
#pragma once
#include <hip/hip_runtime.h>

namespace smst {

typedef float2 fc;

static inline fc fmake(float re, float im) { return make_float2(re, im); }
static inline fc fpack(float2 a) { return a; }
static inline float2 funpack(fc a) { return a; }
static inline fc fadd(fc a, fc b) { return make_float2(a.x + b.x, a.y + b.y); }
static inline fc fsub(fc a, fc b) { return make_float2(a.x - b.x, a.y - b.y); }
static inline fc fmulExpr(fc a, fc b) { return make_float2(a.x*b.x - a.y*b.y, a.x*b.y + a.y*b.x); }
template <bool CONJ>
static inline fc fmul(fc a, fc b) { // a*b, or a*conj(b)
	if (CONJ) b.y = -b.y;
	return fmulExpr(a, b);
}
static inline fc fmulc(fc a, fc b) { return make_float2(b.x*a.x + b.y*a.y, b.x*a.y - b.y*a.x); } // a*conj(b), b's terms first
static inline fc faddI(fc a, fc b) { return make_float2(a.x - b.y, a.y + b.x); } // a + i b
static inline fc fsubI(fc a, fc b) { return make_float2(a.x + b.y, a.y - b.x); } // a - i b
static inline fc fconjIf(fc a, bool c) { return make_float2(a.x, c ? -a.y : a.y); }
static inline fc fconjLoad(const float2 *p, bool c) { return fconjIf(*p, c); }
static inline void fconjStore(float2 *p, fc a, bool c) { *p = fconjIf(a, c); }

} // namespace smst
