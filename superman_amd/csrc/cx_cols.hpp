// cx_cols.hpp — the complex walks' column add: a column's Re and Im planes
// added to x as SGPR operands (walk_cplx.hip, walk_cplxexact.hip).
#pragma once
#include "cx.hpp"
#include "walk_common.hpp"

namespace sup {

// Rows [LO, HI) of one plane: HI - LO <= 32 doubles = 64 SGPRs of column data.
// SEL (the chunk start's lane bits): a lane whose bit is clear adds 0.0.  The
// column value is pinned in SGPRs before the select, so the load stays one
// unconditional scalar load (left to itself LLVM guards each row's load with a
// divergent branch on `on`: 2n branches per lane bit and spilled selects).
template <int N, int LO, int HI, bool SEL>
__device__ __forceinline__ void cx_add_re(cx (&x)[N], cdbl* cre, bool on) {
#pragma unroll
  for (int j = LO; j < HI; ++j) {
    double c = cre[j];
    if constexpr (SEL) {
      asm volatile("" : "+s"(c));
      c = on ? c : 0.0;
    }
    x[j].re = x[j].re + c;
  }
}
template <int N, int LO, int HI, bool SEL>
__device__ __forceinline__ void cx_add_im(cx (&x)[N], cdbl* cim, bool on) {
#pragma unroll
  for (int j = LO; j < HI; ++j) {
    double c = cim[j];
    if constexpr (SEL) {
      asm volatile("" : "+s"(c));
      c = on ? c : 0.0;
    }
    x[j].im = x[j].im + c;
  }
}

// Full-column update (cx_add_d2 on every row).  A plane goes through add_col's
// SGPR-operand path in pieces of at most 32 rows with a scheduling fence
// between pieces, so at most 64 SGPRs of column data are live: up to 16 rows
// both planes in one piece, up to 32 rows a piece per plane, above that two
// passes of two pieces (a complex column of 32 rows taken at once would be
// 128 SGPRs; the wave has 102).
template <int N, bool SEL = false>
__device__ __forceinline__ void cx_add_col(cx (&x)[N], cdbl* cre, cdbl* cim, bool on = true) {
  if constexpr (N <= 16) {
    cx_add_re<N, 0, N, SEL>(x, cre, on);
    cx_add_im<N, 0, N, SEL>(x, cim, on);
  } else if constexpr (N <= 32) {
    cx_add_re<N, 0, N, SEL>(x, cre, on);
    __builtin_amdgcn_sched_barrier(0);
    cx_add_im<N, 0, N, SEL>(x, cim, on);
  } else {
    cx_add_re<N, 0, 32, SEL>(x, cre, on);
    __builtin_amdgcn_sched_barrier(0);
    cx_add_im<N, 0, 32, SEL>(x, cim, on);
    __builtin_amdgcn_sched_barrier(0);
    cx_add_re<N, 32, N, SEL>(x, cre, on);
    __builtin_amdgcn_sched_barrier(0);
    cx_add_im<N, 32, N, SEL>(x, cim, on);
  }
}

}  // namespace sup
