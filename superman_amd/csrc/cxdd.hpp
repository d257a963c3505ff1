// cxdd.hpp — complex double-double arithmetic shared by the gfx950 complex
// double-double walk (walk_cplxdd.hip) and its host twin (cplx_quad.cpp), so
// both run the same operations in the same order and agree bit for bit.
//
// A value is two double-doubles (re, im): four fp64 registers, ~106 bits per
// part.  Everything here is composed from dd.hpp operations in a fixed order
// (dd.hpp holds the only fmas; built with -ffp-contract=off on host and
// device), so the twin needs nothing of its own.
//
// Operation order and fp64 VALU ops:
//   cxdd_add_d2(x, cre, cim)  re' = dd_add_d(x.re, cre)                    9
//                             im' = dd_add_d(x.im, cim)                    9   = 18
//   cxdd_mul(a, b)            re' = dd_add(dd_mul(a.re, b.re),
//                                          dd_neg(dd_mul(a.im, b.im)))     7 + 7 + 20
//                             im' = dd_add(dd_mul(a.re, b.im),
//                                          dd_mul(a.im, b.re))             7 + 7 + 20   = 68
//   cxdd_add                  componentwise dd_add, re then im             20 + 20      = 40
//   cxdd_neg                  sign flips (exact)
// cxdd_mul is not commutative in its rounding (dd_mul adds its cross terms in
// operand order): callers keep the operand order, (p0 p1)(p2 p3) with the
// lower-indexed factor first, as cx_mul's callers do.
// A walk of order n costs 18n + 68(n - 1) + 40 = 86n - 28 ops per Gray step
// and lane (sup_stats.est_ops_per_step of sup_perman_complex_quad); a change
// to the arithmetic here changes that formula with it.  The counts are
// dd.hpp's nominal ones, as sup_perman_quad's 16n + 13; dd_add_d compiles to
// 10 instructions (two_sum is 6), so the kernel's loop holds 88n - 28.
#pragma once

#include "dd.hpp"

namespace sup {

struct cxdd {
  dd re, im;
};

// x + (cre + i cim): the walk's column add, the column's two planes as doubles.
SUP_DD_FN cxdd cxdd_add_d2(cxdd x, double cre, double cim) {
  return cxdd{dd_add_d(x.re, cre), dd_add_d(x.im, cim)};
}

SUP_DD_FN cxdd cxdd_mul(cxdd a, cxdd b) {
  const dd re = dd_add(dd_mul(a.re, b.re), dd_neg(dd_mul(a.im, b.im)));
  const dd im = dd_add(dd_mul(a.re, b.im), dd_mul(a.im, b.re));
  return cxdd{re, im};
}

SUP_DD_FN cxdd cxdd_add(cxdd a, cxdd b) { return cxdd{dd_add(a.re, b.re), dd_add(a.im, b.im)}; }
SUP_DD_FN cxdd cxdd_neg(cxdd a) { return cxdd{dd_neg(a.re), dd_neg(a.im)}; }

}  // namespace sup
