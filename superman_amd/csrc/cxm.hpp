// cxm.hpp — one Gray state of the one-walk permanent minors, shared by the
// gfx950 kernel (walk_cplxm.hip) and its host twin (cplx_minors.cpp), so both
// run the same cx.hpp operations in the same order and agree bit for bit.
//
// B is N x (N-1) complex; minor j is B without row j.  The Nijenhuis-Wilf row
// sums x_0..x_{N-1} of a Gray state serve every minor: the term of minor j is
// the product of all x_i but x_j, formed from a prefix and a suffix product.
//
// Operation order of cxm_accumulate<N, SUB>(x, acc), N >= 2 (built with
// -ffp-contract=off; the only fmas are cx_mul's):
//   pre_1 = x_0;  pre_{i+1} = cx_mul(pre_i, x_i)        i = 1 .. N-2, ascending
//   acc_{N-1} -+= pre_{N-1}                              (term_{N-1})
//   suf = x_{N-1}                                        (suf_{N-1})
//   for j = N-2 down to 1:
//     acc_j -+= cx_mul(pre_j, suf)                       (term_j = pre_j suf_{j+1})
//     suf     = cx_mul(x_j, suf)                         (suf_j  = x_j suf_{j+1})
//   acc_0 -+= suf                                        (term_0 = suf_1)
// with the lower-indexed factor first in every cx_mul and -+ = cx_sub (SUB) or
// cx_add.  3 (N-2) cx_mul and N accumulates: 12 N - 24 + 2 N fp64 operations;
// with the walk's column add (2 N) a Gray step costs 16 N - 24.
#pragma once
#include "cx.hpp"

namespace sup {

template <int N, bool SUB>
SUP_CX_FN void cxm_accumulate(const cx (&x)[N], cx (&acc)[N]) {
  static_assert(N >= 2, "a minor needs at least two rows to choose from");
  cx pre[N];  // pre[i] = x_0 .. x_{i-1}; pre[0] is not used
  pre[1] = x[0];
#pragma unroll
  for (int i = 1; i + 1 < N; ++i) pre[i + 1] = cx_mul(pre[i], x[i]);
  acc[N - 1] = SUB ? cx_sub(acc[N - 1], pre[N - 1]) : cx_add(acc[N - 1], pre[N - 1]);
  cx suf = x[N - 1];
#pragma unroll
  for (int j = N - 2; j >= 1; --j) {
    const cx term = cx_mul(pre[j], suf);
    acc[j] = SUB ? cx_sub(acc[j], term) : cx_add(acc[j], term);
    suf = cx_mul(x[j], suf);
  }
  acc[0] = SUB ? cx_sub(acc[0], suf) : cx_add(acc[0], suf);
}

}  // namespace sup
