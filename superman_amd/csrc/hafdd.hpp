// hafdd.hpp — what the double-double hafnian walk (walk_hafdd.hip), its host
// twin and slab builder (hafnian_quad.cpp) and its device runner (engine.cpp
// run_hafnian_quad) share: the table every matrix's walk reads, the program
// entry, and every arithmetic operation of the walk, so that kernel and twin
// run the same dd.hpp / cxdd.hpp operations in the same order and agree bit for
// bit.  DESIGN.md §8q states the sum, the order and the error bound.
//
// The sum, the index set, the digits and the queue are haf.hpp's (§8h); every
// running value is a cxdd.  The inputs are doubles: B = A / 2 and mu are exact,
// so the step rows and the B entries of the high rows stay (re, im) pairs; the
// four kinds of entry that are sums are cxdd, two pairs each,
// (re.hi, re.lo) then (im.hi, im.lo).  The table of one matrix, in pairs, W
// walk digits and ND high digits (entries of walk digits e >= W are zero):
//   [0, 1] Q(0)  [2, 3] r(0)  [4 + 2e, 5 + 2e] G_e(0), e < 10        kHafddStart pairs
//   step row 2 d + s, d < W: haf.hpp's row, unchanged                kHafRow pairs each
//   high row j < ND (digit W + j):                                   kHafddHigh + ND pairs each
//     [0, 1] (B h(0))_j  [2] B(j, j)  [3] mu_j  [4 + e] B(j, e), e < 10  [14 + j'] B(j, j')
// hafdd_entry below gives every pair; the host twin and hafdd_prepare call it.
//
// Operations (h_l = s_l / 2 a half-integer, dv = -v an integer, both exact
// doubles; the parts re and im never mix outside cxdd_mul):
//   (B h(0))_k  = sum_l two_prod(h_l, B_kl)         dd_add, l ascending
//   Q(0)        = sum_k dd_mul_d((B h(0))_k, h_k)   dd_add, k ascending
//   r(0)        = sum_k two_prod(h_k, mu_k)         dd_add, k ascending
//   chunk start, per high digit j ascending (hafdd_mad, hafdd_mad_dd):
//     t  = (B h(0))_j + sum_{j' < j} two_prod(dv_j', B(j, j'))   j' ascending
//     Q  = (Q + dd_mul_d(t, 2 dv_j)) + two_prod(dv_j^2, B_jj)
//     r  = r + two_prod(dv_j, mu_j);  G_e = G_e + two_prod(dv_j, B(j, e)), e < 4 or e < 10
//     hw = dd_mul(hw, C_j)            the dd weight table's entry
//   step (hafdd_step_q, hafdd_add_d2):
//     Q  = dd_add_d(dd_add(Q, (-2 delta) G_d), B_dd)    the scaling by 2 is exact
//     G_e = dd_add_d(G_e, -delta B_ed), e < 4 or e < 10;  r = dd_add_d(r, -delta mu_d)
//   term = Q^m (hafdd_pow: cxdd_mul, the running power first) or the loop
//     polynomial (hafdd_loop_poly: haf_loop_poly's Horner form, c_j a dd)
//   acc  = cxdd_add(acc, (dd_mul(w, term.re), dd_mul(w, term.im)))   w the entry's dd weight
//   lane end: acc = (dd_mul(acc.re, hw), dd_mul(acc.im, hw))
//   64-lane xor butterfly, chunk fold (fock_fold's tree), both on cxdd_add
//   result = 2 x the sum (exact), then dd_div by m! for the plain form
#pragma once
#include <stdint.h>

#include "cxdd.hpp"
#include "haf.hpp"

namespace sup {

constexpr int kHafddStart = 2 * (2 + kHafWalkDigits);
constexpr int kHafddHigh = 4 + kHafWalkDigits;

struct HafddStep {
  uint32_t row;  // byte offset of the step row in the matrix's table
  uint32_t dsg;  // 2 d + s
  uint32_t pad_[2];
  double w_hi, w_lo;  // (-1)^(sum of walk digits) x prod C(s'_k, v_k) over the walk digits: the exact integer as a dd
};
static_assert(sizeof(HafddStep) == 32, "a program entry is two 16-byte scalar loads");

struct HafddParams {
  const double* tabs;
  const HafddStep* prog;
  const HafDigit* dig;
  const double* wts;  // (hi, lo) per entry of the weight triangle (HafDigit::wt_off)
  const HafMat* mats;  // HafMat::tab and ::pairs describe the dd table
  const FockChunk* chunks;
  const double* coef;  // loop form: 1 / (j! (n - 2j)!) as (hi, lo), j <= n / 2
  unsigned long long chunk_count;
  double* chunk_out;      // 4 doubles (re.hi, re.lo, im.hi, im.lo) per wave-chunk
  unsigned int* counter;  // queue head (zeroed before launch)
  unsigned int group;     // chunks per ticket (1..64)
  unsigned int n;         // the order of every matrix
};

inline uint32_t hafdd_pairs(int W, int ND) {
  return (uint32_t)(kHafddStart + 2 * W * kHafRow + ND * (kHafddHigh + ND));
}
inline uint32_t hafdd_row_bytes(uint32_t dsg) { return 16u * (uint32_t)(kHafddStart + (int)dsg * kHafRow); }

// Part `part` (0: re, 1: im) of (B h(0))_k.
SUP_DD_FN dd hafdd_bh0(const double* A, int M, const int32_t* g, int K, int k, int part) {
  dd y{0.0, 0.0};
  for (int l = 0; l < K; ++l) {
    const double h = 0.5 * (double)g[2 * l + 1];
    const cx b = haf_b(A, M, g, k, l);
    y = dd_add(y, dd_two_prod(h, part ? b.im : b.re));
  }
  return y;
}

// Pair e of the dd table of a matrix with groups g (haf_entry's arguments).
SUP_DD_FN cx hafdd_entry(const double* A, int M, const double* mu, const int32_t* g, int K, int W, int ND, uint32_t e) {
  const int32_t* col = g + 2 * K;
  if (e < (uint32_t)kHafddStart) {
    const int slot = (int)(e >> 1), part = (int)(e & 1u);
    dd s{0.0, 0.0};
    if (slot == 0) {
      for (int k = 0; k < K; ++k) {
        const double h = 0.5 * (double)g[2 * k + 1];
        s = dd_add(s, dd_mul_d(hafdd_bh0(A, M, g, K, k, part), h));
      }
    } else if (slot == 1) {
      for (int k = 0; k < K; ++k) {
        const double h = 0.5 * (double)g[2 * k + 1];
        const cx u = haf_mu(mu, g, k);
        s = dd_add(s, dd_two_prod(h, part ? u.im : u.re));
      }
    } else if (slot - 2 < W) {
      s = hafdd_bh0(A, M, g, K, col[slot - 2], part);
    }
    return cx{s.hi, s.lo};
  }
  e -= (uint32_t)kHafddStart;
  const uint32_t rows = (uint32_t)(2 * W * kHafRow);
  if (e < rows) return haf_entry(A, M, mu, g, K, W, ND, (uint32_t)kHafStart + e);
  e -= rows;
  const int hs = kHafddHigh + ND, j = (int)e / hs, i = (int)e - j * hs;
  if (i < 2) {
    const dd s = hafdd_bh0(A, M, g, K, col[W + j], i);
    return cx{s.hi, s.lo};
  }
  // haf.hpp's high row holds the same plain entries one pair lower
  return haf_entry(A, M, mu, g, K, W, ND, (uint32_t)kHafStart + rows + (uint32_t)(j * (kHafHigh + ND) + i - 1));
}

// x + s b: s an integer-valued double, b a plain pair.
SUP_DD_FN cxdd hafdd_mad(cxdd x, double s, double bre, double bim) {
  return cxdd{dd_add(x.re, dd_two_prod(s, bre)), dd_add(x.im, dd_two_prod(s, bim))};
}
// x + s t: t a cxdd.
SUP_DD_FN cxdd hafdd_mad_dd(cxdd x, double s, cxdd t) {
  return cxdd{dd_add(x.re, dd_mul_d(t.re, s)), dd_add(x.im, dd_mul_d(t.im, s))};
}
// (Q + m2 G_d) + B_dd, m2 = +-2.
SUP_DD_FN cxdd hafdd_step_q(cxdd Q, cxdd gd, double m2, double bre, double bim) {
  const dd sr{m2 * gd.re.hi, m2 * gd.re.lo}, si{m2 * gd.im.hi, m2 * gd.im.lo};
  return cxdd{dd_add_d(dd_add(Q.re, sr), bre), dd_add_d(dd_add(Q.im, si), bim)};
}
SUP_DD_FN cxdd hafdd_accum(cxdd acc, dd w, cxdd term) {
  return cxdd_add(acc, cxdd{dd_mul(w, term.re), dd_mul(w, term.im)});
}
SUP_DD_FN cxdd hafdd_scale(cxdd a, dd w) { return cxdd{dd_mul(a.re, w), dd_mul(a.im, w)}; }

// Q^m, m >= 1: haf_pow on cxdd_mul.
SUP_DD_FN cxdd hafdd_pow(cxdd q, uint32_t m) {
  int top = 0;
  while ((m >> (top + 1)) != 0u) ++top;
  cxdd p = q;
  for (int b = top - 1; b >= 0; --b) {
    p = cxdd_mul(p, p);
    if ((m >> b) & 1u) p = cxdd_mul(p, q);
  }
  return p;
}

// haf_loop_poly on cxdd; c holds (hi, lo) per j.
template <class CP>
SUP_DD_FN cxdd hafdd_loop_poly(cxdd q, cxdd r, CP c, uint32_t n) {
  const uint32_t m = n >> 1;
  const cxdd R = cxdd_mul(r, r);
  cxdd P{dd{c[2 * m], c[2 * m + 1]}, dd{0.0, 0.0}};
  cxdd Rp = R;
  for (uint32_t j = m; j-- > 0;) {
    P = cxdd_mul(P, q);
    const dd cj{c[2 * j], c[2 * j + 1]};
    P = cxdd{dd_add(P.re, dd_mul(cj, Rp.re)), dd_add(P.im, dd_mul(cj, Rp.im))};
    if (j) Rp = cxdd_mul(Rp, R);
  }
  if (n & 1u) P = cxdd_mul(P, r);
  return P;
}

// fock_fold's tree over `count` partials of 4 doubles, on cxdd_add.
SUP_DD_FN cxdd hafdd_fold_tree(const double* src, uint32_t count) {
  const cxdd zero{dd{0.0, 0.0}, dd{0.0, 0.0}};
  cxdd st[kFockFoldStack];
#pragma unroll
  for (int l = 0; l < kFockFoldStack; ++l) st[l] = zero;
  for (uint32_t i = 0; i < count; ++i) {
    const double* s = src + 4 * (uint64_t)i;
    cxdd c{dd{s[0], s[1]}, dd{s[2], s[3]}};
    bool placed = false;
#pragma unroll
    for (int l = 0; l < kFockFoldStack; ++l) {
      if (!placed) {
        if ((i >> l) & 1u) {
          c = cxdd_add(st[l], c);
        } else {
          st[l] = c;
          placed = true;
        }
      }
    }
  }
  cxdd r = zero;
  bool have = false;
#pragma unroll
  for (int l = 0; l < kFockFoldStack; ++l) {
    if ((count >> l) & 1u) {
      r = have ? cxdd_add(st[l], r) : st[l];
      have = true;
    }
  }
  return r;
}

// 2 x the folded sum, divided by div = m! for the plain form (loop: not divided).
SUP_DD_FN cxdd hafdd_finish(cxdd v, dd div, bool loop) {
  const cxdd t{dd{2.0 * v.re.hi, 2.0 * v.re.lo}, dd{2.0 * v.im.hi, 2.0 * v.im.lo}};
  return loop ? t : cxdd{dd_div(t.re, div), dd_div(t.im, div)};
}

// fp64 operations per visited state and lane in dd.hpp's nominal counts
// (dd_add 20, dd_add_d 9, dd_mul 7, cxdd_mul 68, cxdd_add 40): the Q update
// 4 + 40 + 18 = 62, the G update 18 per entry (4 entries at W <= 4, else 10),
// the accumulate 14 + 40 = 54, the power 68 per cxdd_mul; the loop form adds r
// (18), R (68), per j 68 + 14 + 40 + 68 (no power step at j = 0) and 68 for odd n.
inline double hafdd_ops(int W, int n, bool loop) {
  const int m = n / 2;
  const double gops = W <= 4 ? 72.0 : 180.0;
  if (!loop) {
    int top = 0, pop = 0;
    for (int b = 0; b < 31; ++b)
      if ((m >> b) & 1) top = b, ++pop;
    return 62.0 + 54.0 + gops + 68.0 * (top + pop - 1);
  }
  return 62.0 + 54.0 + gops + 18.0 + 68.0 + (m ? 190.0 * m - 68.0 : 0.0) + ((n & 1) ? 68.0 : 0.0);
}

}  // namespace sup
