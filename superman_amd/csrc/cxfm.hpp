// cxfm.hpp — one walked state of the collision-aware one-walk minors, shared by
// the gfx950 kernel (walk_cplxfm.hip) and its host twin (cplx_fock_minors.cpp),
// so both run the same cx.hpp operations in the same order and agree bit for
// bit.
//
// B is N x (N-1) complex, minor j is B without row j, and the column side is
// collapsed as §8c collapses it: a walked state has the row sums x_0..x_{N-1}
// and the real signed weight w = (-1)^(sum v) prod C(t'_k, v_k) of its walk
// digits.  The term of minor j is w times the product of all x_i but x_j, from
// cxm.hpp's prefix and suffix products; w enters once at each end of the
// chain (x_0 opens every prefix, the suffix alone is term 0), so weighting
// costs 4 multiplies and not 2N.
//
// Operation order of cxfm_accumulate<N>(x, w, acc), N >= 2 (built with
// -ffp-contract=off; the only fmas are cx_mul's):
//   pw = {w x_0.re, w x_0.im}
//   pre_1 = pw;  pre_{i+1} = cx_mul(pre_i, x_i)         i = 1 .. N-2, ascending
//   acc_{N-1} += pre_{N-1}
//   suf = x_{N-1}
//   for j = N-2 down to 1:
//     acc_j += cx_mul(pre_j, suf)
//     suf    = cx_mul(x_j, suf)
//   acc_0 += {w suf.re, w suf.im}
// with the lower-indexed factor first in every cx_mul; the sign lives in w, so
// every accumulate is cx_add.  3 (N-2) cx_mul, 4 multiplies and N accumulates:
// 12 N - 24 + 4 + 2 N fp64 operations; with the walk's column add (2 N) a
// walked step costs 16 N - 20.  The state t = 0 of a chunk has weight +1 and
// runs cxm_accumulate<N, false> (cxm.hpp) as it is.
#pragma once
#include "cxm.hpp"

namespace sup {

template <int N>
SUP_CX_FN void cxfm_accumulate(const cx (&x)[N], double w, cx (&acc)[N]) {
  static_assert(N >= 2, "a minor needs at least two rows to choose from");
  cx pre[N];  // pre[i] = w x_0 .. x_{i-1}; pre[0] is not used
  pre[1] = cx{w * x[0].re, w * x[0].im};
#pragma unroll
  for (int i = 1; i + 1 < N; ++i) pre[i + 1] = cx_mul(pre[i], x[i]);
  acc[N - 1] = cx_add(acc[N - 1], pre[N - 1]);
  cx suf = x[N - 1];
#pragma unroll
  for (int j = N - 2; j >= 1; --j) {
    acc[j] = cx_add(acc[j], cx_mul(pre[j], suf));
    suf = cx_mul(x[j], suf);
  }
  acc[0] = cx_add(acc[0], cx{w * suf.re, w * suf.im});
}

}  // namespace sup
