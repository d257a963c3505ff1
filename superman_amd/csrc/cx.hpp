// cx.hpp — complex fp64 arithmetic shared by the gfx950 complex walk
// (walk_cplx.hip) and its host twin (cplx.cpp), so both run the same
// operations in the same order and agree bit for bit.
//
// The reference refuses complex input ("SUPerman does not support complex
// type", revised_perman/main.cpp:1557).  A value is a pair of fp64 registers
// (re, im).  Built with -ffp-contract=off (host and device): the only fmas
// are the explicit ones below.
//
// Operation order (device and host round alike because both run exactly this):
//   cx_add_d2(x, cre, cim)  re' = x.re + cre;  im' = x.im + cim          2 adds
//   cx_mul(a, b)            t   = a.im * b.im                            1 mul
//                           re' = fma(a.re, b.re, -t)                    1 fma
//                           u   = a.im * b.re                            1 mul
//                           im' = fma(a.re, b.im, u)                     1 fma
//   cx_add / cx_sub         componentwise, re then im                    2 adds
//   cx_neg                  sign flips (exact)
// cx_mul is not commutative in its rounding (a's parts are the fma
// multiplicands, the plain products take a.im): callers keep the operand
// order, (p0 p1)(p2 p3) with the lower-indexed factor first.
#pragma once

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define SUP_CX_FN __host__ __device__ __forceinline__
#else
#define SUP_CX_FN inline
#endif

namespace sup {

struct cx {
  double re, im;
};

// x + (cre + i cim): the walk's column add, the column's two planes as doubles.
SUP_CX_FN cx cx_add_d2(cx x, double cre, double cim) { return cx{x.re + cre, x.im + cim}; }

SUP_CX_FN cx cx_mul(cx a, cx b) {
  const double t = a.im * b.im;
  const double re = __builtin_fma(a.re, b.re, -t);
  const double u = a.im * b.re;
  const double im = __builtin_fma(a.re, b.im, u);
  return cx{re, im};
}

SUP_CX_FN cx cx_add(cx a, cx b) { return cx{a.re + b.re, a.im + b.im}; }
SUP_CX_FN cx cx_sub(cx a, cx b) { return cx{a.re - b.re, a.im - b.im}; }
SUP_CX_FN cx cx_neg(cx a) { return cx{-a.re, -a.im}; }

}  // namespace sup
