// haf.hpp — what the hafnian walk (walk_haf.hip), its host twin and slab
// builder (hafnian.cpp) and its device runner (engine.cpp run_hafnian) share:
// the descriptors of a slab, the table every matrix's walk reads, and the
// summand.  DESIGN.md §8h states the sum.
//
// Matrix k is the n x n symmetric gather A[idx_i][idx_j].  With the K distinct
// values of idx (multiplicities s_k, order of first appearance), B = Abar / 2
// on them, one copy of the rarest group held (s'_k; cplx_fock.cpp's rule) and
//   h_k = s_k / 2 - v_k,  Q(v) = h^T B h (= q / 2),  r(v) = mu . h
//   haf  = 2 / m!  sum_v (-1)^(sum v) prod C(s'_k, v_k)  Q^m          m = n / 2
//   lhaf = 2       sum_v (...)  sum_j Q^j / j!  r^(n-2j) / (n-2j)!
// The digits v_k are cplx_fock.cpp's: walk digits (every lane walks them in the
// same reflected mixed-radix Gray order) and high digits (h = 64 chunk + lane).
// A step that moves walk digit d by delta updates, with G = B h:
//   Q <- fma(-2 delta, G_d, Q) + B_dd;  G_e <- G_e - delta B_ed (walk digits e);
//   r <- r - delta mu_d
//
// The table of one matrix, in (re, im) pairs, W walk digits and ND high digits
// (entries of walk digits e >= W are zero):
//   [0] Q(0)  [1] r(0)  [2 + e] G_e(0), e < 10                       kHafStart pairs
//   step row 2 d + s (s = 0: delta = +1, s = 1: delta = -1), d < W:  kHafRow pairs each
//     [e] -delta B(e, d), e < 10   [10] B(d, d)   [11] -delta mu_d
//   high row j < ND (digit W + j):                                   kHafHigh + ND pairs each
//     [0] (B h(0))_j  [1] B(j, j)  [2] mu_j  [3 + e] B(j, e), e < 10  [13 + j'] B(j, j'), j' < ND
// haf_entry below gives every pair; the host twin and haf_prepare both call it.
#pragma once
#include <stdint.h>

#include "cplx_fock.hpp"
#include "cx.hpp"

namespace sup {

constexpr int kHafWalkDigits = 10;  // Tw <= 2^10, every radix >= 2
constexpr int kHafHighDigits = 30;  // H <= 64 x 2^24 = 2^30, every radix >= 2
constexpr int kHafStart = 2 + kHafWalkDigits;
constexpr int kHafRow = kHafWalkDigits + 2;
constexpr int kHafHigh = 3 + kHafWalkDigits;

struct HafStep {
  uint32_t row;  // byte offset of the step row in the matrix's table
  uint32_t dsg;  // 2 d + s
  double w;      // (-1)^(sum of walk digits) x prod C(s'_k, v_k) over the walk digits, after the step
};

struct HafDigit {
  uint32_t radix;   // s'_k + 1
  uint32_t wt_off;  // wts index of (-1)^0 C(s'_k, 0)
};

struct HafMat {
  uint64_t tab;     // tabs index (doubles) of the table
  uint32_t prog;    // prog index of entry 0
  uint32_t dig;     // dig index of the first high digit
  uint32_t Tw;      // states each lane walks
  uint32_t W;       // walk digits
  uint32_t ndig;    // high digits
  uint32_t H;       // valid values of h = 64 chunk + lane
  uint32_t chunk0;  // the matrix's first wave-chunk in the slab's queue and partials
  uint32_t chunks;  // ceil(H / 64)
  uint32_t K;       // distinct values
  uint32_t grp;     // grp index: K (value, multiplicity) pairs, then the group of each digit
  uint32_t pairs;   // pairs in the table
  uint32_t ord;     // ragged slabs (walk_lhafe.hip): the matrix's order n | its coef row's offset (doubles) << 8; else 0
};

struct HafParams {
  const double* tabs;
  const HafStep* prog;
  const HafDigit* dig;
  const double* wts;
  const HafMat* mats;
  const FockChunk* chunks;
  const double* coef;  // loop form: 1 / (j! (n - 2j)!), j <= n / 2 (ragged slabs: the pool of those rows, HafMat::ord)
  unsigned long long chunk_count;
  double* chunk_out;      // 2 doubles (re, im) per wave-chunk
  unsigned int* counter;  // queue head (zeroed before launch)
  unsigned int group;     // chunks per ticket (1..64)
  unsigned int n;         // the order of every matrix (ragged slabs: unused, HafMat::ord)
};

inline uint32_t haf_pairs(int W, int ND) {
  return (uint32_t)(kHafStart + 2 * W * kHafRow + ND * (kHafHigh + ND));
}

// B(k, l) = A[val_k][val_l] / 2; g = the (value, multiplicity) pairs.
SUP_CX_FN cx haf_b(const double* A, int M, const int32_t* g, int k, int l) {
  const double* p = A + 2 * ((uint64_t)g[2 * k] * (uint64_t)M + (uint64_t)g[2 * l]);
  return cx{0.5 * p[0], 0.5 * p[1]};
}
SUP_CX_FN cx haf_mu(const double* mu, const int32_t* g, int k) {
  return mu ? cx{mu[2 * (uint64_t)g[2 * k]], mu[2 * (uint64_t)g[2 * k] + 1]} : cx{0.0, 0.0};
}
// (B h(0))_k, h(0)_l = s_l / 2: fma per part, l ascending.
SUP_CX_FN cx haf_bh0(const double* A, int M, const int32_t* g, int K, int k) {
  cx y{0.0, 0.0};
  for (int l = 0; l < K; ++l) {
    const double h = 0.5 * (double)g[2 * l + 1];
    const cx b = haf_b(A, M, g, k, l);
    y = cx{__builtin_fma(h, b.re, y.re), __builtin_fma(h, b.im, y.im)};
  }
  return y;
}

// Pair e of the table of a matrix with groups g (K of them, then the group of
// each of its W + ND digits).  mu null: the plain hafnian (r = 0).
SUP_CX_FN cx haf_entry(const double* A, int M, const double* mu, const int32_t* g, int K, int W, int ND, uint32_t e) {
  const int32_t* col = g + 2 * K;
  if (e == 0) {  // Q(0) = sum_k h_k (B h)_k, k ascending
    cx q{0.0, 0.0};
    for (int k = 0; k < K; ++k) {
      const double h = 0.5 * (double)g[2 * k + 1];
      const cx y = haf_bh0(A, M, g, K, k);
      q = cx{__builtin_fma(h, y.re, q.re), __builtin_fma(h, y.im, q.im)};
    }
    return q;
  }
  if (e == 1) {  // r(0) = sum_k h_k mu_k, k ascending
    cx r{0.0, 0.0};
    for (int k = 0; k < K; ++k) {
      const double h = 0.5 * (double)g[2 * k + 1];
      const cx u = haf_mu(mu, g, k);
      r = cx{__builtin_fma(h, u.re, r.re), __builtin_fma(h, u.im, r.im)};
    }
    return r;
  }
  if (e < (uint32_t)kHafStart) {
    const int i = (int)e - 2;
    return i < W ? haf_bh0(A, M, g, K, col[i]) : cx{0.0, 0.0};
  }
  e -= (uint32_t)kHafStart;
  if (e < (uint32_t)(2 * W * kHafRow)) {
    const int row = (int)e / kHafRow, i = (int)e - row * kHafRow, cd = col[row >> 1];
    const bool up = (row & 1) == 0;  // delta = +1: the row holds -B, -mu
    if (i == kHafWalkDigits) return haf_b(A, M, g, cd, cd);
    if (i >= W && i < kHafWalkDigits) return cx{0.0, 0.0};
    const cx b = i < W ? haf_b(A, M, g, col[i], cd) : haf_mu(mu, g, cd);
    return up ? cx_neg(b) : b;
  }
  e -= (uint32_t)(2 * W * kHafRow);
  const int hs = kHafHigh + ND, j = (int)e / hs, i = (int)e - j * hs, cj = col[W + j];
  if (i == 0) return haf_bh0(A, M, g, K, cj);
  if (i == 1) return haf_b(A, M, g, cj, cj);
  if (i == 2) return haf_mu(mu, g, cj);
  if (i < kHafHigh) return i - 3 < W ? haf_b(A, M, g, cj, col[i - 3]) : cx{0.0, 0.0};
  return haf_b(A, M, g, cj, col[W + i - kHafHigh]);
}

// Q^m, m >= 1: left-to-right square and multiply, the running power first in
// every product.
SUP_CX_FN cx haf_pow(cx q, uint32_t m) {
  int top = 0;
  while ((m >> (top + 1)) != 0u) ++top;
  cx p = q;
  for (int b = top - 1; b >= 0; --b) {
    p = cx_mul(p, p);
    if ((m >> b) & 1u) p = cx_mul(p, q);
  }
  return p;
}

// sum_j c_j Q^j r^(n-2j), c_j = 1 / (j! (n-2j)!), m = n / 2, R = r r:
//   P = c_m;  for j = m-1 .. 0:  P = P Q + c_j R^(m-j)   (cx_mul(P, Q), then the
//   two parts of c_j x the running power of R added, then that power x R);
//   n odd: P = P r.
template <class CP>
SUP_CX_FN cx haf_loop_poly(cx q, cx r, CP c, uint32_t n) {
  const uint32_t m = n >> 1;
  const cx R = cx_mul(r, r);
  cx P{c[m], 0.0};
  cx Rp = R;
  for (uint32_t j = m; j-- > 0;) {
    P = cx_mul(P, q);
    const double cj = c[j];
    const double ar = cj * Rp.re, ai = cj * Rp.im;
    P = cx{P.re + ar, P.im + ai};
    if (j) Rp = cx_mul(Rp, R);
  }
  if (n & 1u) P = cx_mul(P, r);
  return P;
}

// fp64 operations per visited state and lane: the Q update 4,
// the G update 8 (W <= 4) or 20, the accumulate 4; the power 4 per cx_mul; the loop form
// adds r (2), R (4), per j 4 + 4 + 4 (no power step at j = 0) and 4 for odd n.
inline double haf_ops(int W, int n, bool loop) {
  const int m = n / 2;
  const double gops = W <= 4 ? 8.0 : 20.0;
  if (!loop) {
    int top = 0, pop = 0;
    for (int b = 0; b < 31; ++b)
      if ((m >> b) & 1) top = b, ++pop;
    return 8.0 + gops + 4.0 * (top + pop - 1);
  }
  return 8.0 + gops + 2.0 + 4.0 + (m ? 12.0 * m - 4.0 : 0.0) + ((n & 1) ? 4.0 : 0.0);
}

}  // namespace sup
