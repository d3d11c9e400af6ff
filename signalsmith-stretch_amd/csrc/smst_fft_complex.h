// The complex primitives of the FFT kernels (smst_fft.hip) on gfx950 packed-f32 VALU instructions (VOP3P: v_pk_mul_f32, v_pk_fma_f32, v_pk_add_f32).
//
// A value is one 64-bit register pair (fc = pk2f: .x real, .y imaginary) from the load to the store.  What a butterfly does TO an operand --
// conjugate it, multiply it by +-i, negate it -- is no instruction of its own: op_sel / op_sel_hi pick, per result lane, which half of each
// source is read, neg_lo / neg_hi negate a source for one lane.  Written as C++ on float2 (cmulPlain, mulI, mulNegI, `w.y = -w.y` in front of a
// product) the compiler formed the packed instruction for one lane pattern only and built every other operand first: a v_xor + v_mov
// pair for (-w.y, w.x), two packed additions and a v_mov for a +- i b, and v_mov clusters that re-formed pairs from halves of other pairs
// at the end of a stage's region -- 150 to 260 of the 550 to 920 vector instructions of a frame (EXPERIMENTS.md, profiles/fft_core_isa_table.txt).
//
// Rounding.  These are the roundings of the C++ expressions the kernels used before, as -ffp-contract=on compiled them (in `p*q - r*s` and
// `p*q + r*s` the FIRST product is fused, the second rounded), NOT those of smst_complex.h (which rounds the a.x terms and fuses the a.y terms):
//   fmul<false>(a, b)   re = fma(a.x,  b.x, -rnd(a.y*b.y))    im = fma(a.x,  b.y,  rnd(a.y*b.x))      a * b            (was cmulPlain(a, b))
//   fmul<true>(a, b)    re = fma(a.x,  b.x,  rnd(a.y*b.y))    im = fma(a.x, -b.y,  rnd(a.y*b.x))      a * conj(b)      (was cmulPlain(a, (b.x, -b.y)))
//   fmulc(a, b)         re = fma(b.x,  a.x,  rnd(b.y*a.y))    im = fma(b.x,  a.y, -rnd(b.y*a.x))      a * conj(b)      (was cmulcPlain(a, b))
//   faddI(a, b) = (a.x - b.y, a.y + b.x)   a + i b     fsubI(a, b) = (a.x + b.y, a.y - b.x)   a - i b     (was cadd / csub(a, mulI(b)); -i: the other one)
//   fadd, fsub: component-wise; fconjIf(a, c): a.y negated where c (the conjugating load and store of a half-bin row: fconjLoad, fconjStore)
// Negation is exact and fma(p, -q, -r) = -fma(p, q, r), so folding a sign into an operand changes no bit; conj(a)*conj(b) = conj(a*b) bit
// for bit likewise, but for the sign of a zero that two non-zero terms cancel to exactly (the lean first-stage twiddles are multiplied
// unconjugated and conjugated in the product that uses them: products of two table entries, none of which cancels so).
// fmulExpr is fmul<false> as a C++ expression, for an operand that is a compile-time constant (the compiler folds it into the instruction;
// an assembly operand would first be moved into registers): the same formula, so the same bits.
// Products with the constants of a butterfly (mulConst) and the radix-3 / radix-5 butterflies keep their expressions on .x / .y.
//
// The assembly statements are not volatile and touch no memory: the compiler schedules them like its own instructions.
// smst_debug_fft_complex_selftest (kFftComplexSelfTest, smst_state.hip) evaluates every helper on the device against these formulas.
// tests/emu/smst_fft_complex.h is the CPU stand-in's version of this header.
#pragma once
#include <hip/hip_runtime.h>
#include <smst_complex.h> // pk2f

namespace smst {

typedef pk2f fc;

__device__ __forceinline__ fc fmake(float re, float im) { const fc r = {re, im}; return r; }
__device__ __forceinline__ fc fpack(float2 a) { return fmake(a.x, a.y); }
__device__ __forceinline__ float2 funpack(fc a) { return make_float2(a.x, a.y); }
__device__ __forceinline__ fc fadd(fc a, fc b) { return a + b; }
__device__ __forceinline__ fc fsub(fc a, fc b) { return a - b; }

template <bool CONJ>
__device__ __forceinline__ fc fmul(fc a, fc b) { // a*b, or a*conj(b)
	fc t, r;
	asm("v_pk_mul_f32 %0, %1, %2 op_sel:[1,1] op_sel_hi:[1,0]" : "=v"(t) : "v"(a), "v"(b)); // (a.y*b.y, a.y*b.x)
	if constexpr (CONJ) asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[0,1,1] neg_hi:[0,1,0]" : "=v"(r) : "v"(a), "v"(b), "v"(t));
	else asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[0,1,1] neg_lo:[0,0,1]" : "=v"(r) : "v"(a), "v"(b), "v"(t));
	return r;
}
__device__ __forceinline__ fc fmulExpr(fc a, fc b) { return fmake(a.x*b.x - a.y*b.y, a.x*b.y + a.y*b.x); }
__device__ __forceinline__ fc fmulc(fc a, fc b) { // a*conj(b), b's terms first
	fc t, r;
	asm("v_pk_mul_f32 %0, %1, %2 op_sel:[1,1] op_sel_hi:[1,0]" : "=v"(t) : "v"(b), "v"(a)); // (b.y*a.y, b.y*a.x)
	asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[0,1,1] neg_hi:[0,0,1]" : "=v"(r) : "v"(b), "v"(a), "v"(t));
	return r;
}
__device__ __forceinline__ fc faddI(fc a, fc b) { // a + i b
	fc r;
	asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[0,1]" : "=v"(r) : "v"(a), "v"(b));
	return r;
}
__device__ __forceinline__ fc fsubI(fc a, fc b) { // a - i b
	fc r;
	asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_hi:[0,1]" : "=v"(r) : "v"(a), "v"(b));
	return r;
}
__device__ __forceinline__ fc fconjIf(fc a, bool c) { return fmake(a.x, c ? -a.y : a.y); }
__device__ __forceinline__ fc fconjLoad(const float2 *p, bool c) { return fconjIf(*reinterpret_cast<const fc *>(p), c); }
__device__ __forceinline__ void fconjStore(float2 *p, fc a, bool c) { *reinterpret_cast<fc *>(p) = fconjIf(a, c); }

} // namespace smst
