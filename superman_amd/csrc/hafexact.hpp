// hafexact.hpp — what the exact hafnian walk (walk_hafexact.hip), its host twin
// (hafnian_exact.cpp) and its device runner (engine.cpp run_hafnian_exact)
// share: the integer table of a matrix, the residue power and loop polynomial,
// the per-prime constants, the op census and the launch parameters.
// DESIGN.md §8k states the sum.
//
// Notation as haf.hpp, with the integers (no halves anywhere)
//   H_k = s_k - 2 v_k,  q'(v) = H^T Abar H (= 8 Q),  r'(v) = mubar . H (= 2 r),  G' = Abar H
//   T = sum_v (-1)^(sum v) prod C(s'_k, v_k) q'^m                       haf  = 2 T / (m! 8^m)
//   L = sum_v (...) sum_{j <= m} c_j q'^j r'^(n-2j)                     lhaf = 2 L / (n! 2^(n+m))
//   c_j = n! / (j! (n-2j)!) 2^(m-j),  m = floor(n / 2)
// A step that moves walk digit d by delta:
//   q' <- q' - 4 delta G'_d + 4 Abar_dd;  G'_e <- G'_e - 2 delta Abar_ed;  r' <- r' - 2 delta mubar_d
// Parts of A and mu are integers below 2^31 and n <= 64, so |q'| < 2^43,
// |G'| < 2^38, |r'| < 2^37 and every intermediate of the step and of the chunk
// start (below 2^46) is an integer exact in fp64, in any order of the sums.
//
// The table of one matrix has haf.hpp's layout and index rule (kHafStart,
// kHafRow, kHafHigh, haf_pairs), with integers in place of B and mu:
//   [0] q'(0)  [1] r'(0)  [2 + e] G'_e(0)
//   step row 2 d + s:  [e] -delta 2 Abar(e, d)   [10] 4 Abar(d, d)   [11] -delta 2 mubar_d
//   high row j:  [0] G'_j(0)  [1] 4 Abar(j, j)  [2] 2 mubar_j  [3 + e] 2 Abar(j, e)  [13 + j'] 2 Abar(j, j')
// Chunk start, dv_j = -v_j the lane's high digits, j ascending:
//   t = G'_j(0) + sum_{j' < j} dv_j' 2 Abar(j, j');  q' += 4 dv_j t + dv_j^2 4 Abar_jj
//   r' += dv_j 2 mubar_j;  G'_e += dv_j 2 Abar(j, e)
//
// Residues (cxexact.hpp): a residue of a Gaussian integer modulo p is a pair
// of fp64 integers in (-1.5 p, 1.5 p).  The power and the polynomial multiply
// a residue by a residue: cxe_link's multiplier then has parts up to Y = 1.5 p,
// and its inequality 1.5 p Y < 2^52 reads
//     2.25 p^2 < 2^52,  which holds for every prime p < 2^25
// (2.25 2^50 < 2^52; |uc - vd| < 4.5 2^50 < 2^53, so the product and the fma's
// one rounding are exact).  The same bound covers a residue times a weight or
// coefficient in [0, p) (1.5 p^2) and the polynomial's c_j R^(m-j) + P
// (1.5 p^2 + 1.5 p < 2^52).  kHafxPrimeBits = 25 is that limit.
// Every weight is a residue: prod C(s'_k, v_k) exceeds 2^53 both over the high
// digits (C(31,15) C(32,16) at (32, 32)) and over the walk digits (C(57, 28) at
// (57, 1 x 7): the layout rule leaves H >= 64, so the walk digits hold at most
// 57 of 63 copies), so neither is kept as a double.
#pragma once
#include <stdint.h>

#include "cxexact.hpp"
#include "haf.hpp"

namespace sup {

constexpr int kHafxPrimeBits = 25;  // p < 2^25: 2.25 p^2 < 2^52 (above)

// Primes per launch of walk_hafexact (walk_hafexact.hip's header says why).
#ifndef SUP_HAFX_PRIMES
#define SUP_HAFX_PRIMES 8  // (other values: the resource scan that chose it)
#endif
constexpr int kHafxPrimes = SUP_HAFX_PRIMES;

// The constants of one prime, in doubles, `stride` apart in HafxParams::ptab:
//   [0] p  [1] 1 / p rounded  [kHafxCoef + j] c_j mod p, j <= 32
//   [kHafxBinom + t (t + 1) / 2 + v] (-1)^v C(t, v) mod p, t < 64 (HafDigit::wt_off indexes it)
//   [kHafxStepW + e] the weight of program entry e of the slab's prog pool mod p
// all in [0, p).
constexpr int kHafxCoef = 2;
constexpr int kHafxBinom = 40;
constexpr int kHafxBinoms = 64 * 65 / 2;
constexpr int kHafxStepW = kHafxBinom + kHafxBinoms;
inline uint64_t hafx_stride(uint64_t prog_entries) { return ((uint64_t)kHafxStepW + prog_entries + 7) / 8 * 8; }

struct HafxParams {
  const double* tabs;  // hafx_entry's tables
  const HafStep* prog;  // HafStep::w is not read: the weights are in ptab
  const HafDigit* dig;
  const HafMat* mats;
  const FockChunk* chunks;
  const double* ptab;  // nprimes blocks of `stride` doubles
  unsigned long long chunk_count;
  double* chunk_out;      // [chunk][kHafxPrimes][2]: the chunk's residue sums (re, im), in [0, p)
  unsigned int* counter;  // queue head (zeroed before launch)
  unsigned int group;     // chunks per ticket (1..64)
  unsigned int n;
  unsigned int nprimes;  // 1..kHafxPrimes
  unsigned int stride;   // doubles per prime in ptab
};

// Abar(k, l) and mubar_k of the groups g (haf.hpp haf_b without the half).
SUP_CX_FN cx hafx_a(const double* A, int M, const int32_t* g, int k, int l) {
  const double* p = A + 2 * ((uint64_t)g[2 * k] * (uint64_t)M + (uint64_t)g[2 * l]);
  return cx{p[0], p[1]};
}
SUP_CX_FN cx hafx_scale(double s, cx v) { return cx{s * v.re, s * v.im}; }
// G'_k(0) = sum_l s_l Abar(k, l)
SUP_CX_FN cx hafx_g0(const double* A, int M, const int32_t* g, int K, int k) {
  cx y{0.0, 0.0};
  for (int l = 0; l < K; ++l) y = cx_add(y, hafx_scale((double)g[2 * l + 1], hafx_a(A, M, g, k, l)));
  return y;
}

// Pair e of the integer table (haf.hpp haf_entry's index rule).  mu null: r' = 0.
SUP_CX_FN cx hafx_entry(const double* A, int M, const double* mu, const int32_t* g, int K, int W, int ND, uint32_t e) {
  const int32_t* col = g + 2 * K;
  if (e == 0) {
    cx q{0.0, 0.0};
    for (int k = 0; k < K; ++k) q = cx_add(q, hafx_scale((double)g[2 * k + 1], hafx_g0(A, M, g, K, k)));
    return q;
  }
  if (e == 1) {
    cx r{0.0, 0.0};
    for (int k = 0; k < K; ++k) r = cx_add(r, hafx_scale((double)g[2 * k + 1], haf_mu(mu, g, k)));
    return r;
  }
  if (e < (uint32_t)kHafStart) {
    const int i = (int)e - 2;
    return i < W ? hafx_g0(A, M, g, K, col[i]) : cx{0.0, 0.0};
  }
  e -= (uint32_t)kHafStart;
  if (e < (uint32_t)(2 * W * kHafRow)) {
    const int row = (int)e / kHafRow, i = (int)e - row * kHafRow, cd = col[row >> 1];
    const bool up = (row & 1) == 0;  // delta = +1: the row holds -2 Abar, -2 mubar
    if (i == kHafWalkDigits) return hafx_scale(4.0, hafx_a(A, M, g, cd, cd));
    if (i >= W && i < kHafWalkDigits) return cx{0.0, 0.0};
    const cx b = hafx_scale(2.0, i < W ? hafx_a(A, M, g, col[i], cd) : haf_mu(mu, g, cd));
    return up ? cx_neg(b) : b;
  }
  e -= (uint32_t)(2 * W * kHafRow);
  const int hs = kHafHigh + ND, j = (int)e / hs, i = (int)e - j * hs, cj = col[W + j];
  if (i == 0) return hafx_g0(A, M, g, K, cj);
  if (i == 1) return hafx_scale(4.0, hafx_a(A, M, g, cj, cj));
  if (i == 2) return hafx_scale(2.0, haf_mu(mu, g, cj));
  if (i < kHafHigh) return i - 3 < W ? hafx_scale(2.0, hafx_a(A, M, g, cj, col[i - 3])) : cx{0.0, 0.0};
  return hafx_scale(2.0, hafx_a(A, M, g, cj, col[W + i - kHafHigh]));
}

// q^m in (Z/p)[i] for a residue q, m >= 1: haf_pow's square and multiply with
// every cx_mul a cxe_link (residue times residue: p < 2^25).
SUP_CX_FN cx hafx_pow(cx q, uint32_t m, double p, double pinv) {
  int top = 0;
  while ((m >> (top + 1)) != 0u) ++top;
  cx r = q;
  for (int b = top - 1; b >= 0; --b) {
    r = cxe_link(r, r, p, pinv);
    if ((m >> b) & 1u) r = cxe_link(r, q, p, pinv);
  }
  return r;
}

// sum_j c_j q^j r^(n-2j) in (Z/p)[i] for residues q, r and c_j in [0, p):
// haf_loop_poly's Horner scheme, every cx_mul a cxe_link.
template <class CP>
SUP_CX_FN cx hafx_loop_poly(cx q, cx r, CP c, uint32_t n, double p, double pinv) {
  const uint32_t m = n >> 1;
  const cx R = cxe_link(r, r, p, pinv);
  cx P{c[m], 0.0};
  cx Rp = R;
  for (uint32_t j = m; j-- > 0;) {
    P = cxe_link(P, q, p, pinv);
    const double cj = c[j];
    const double ar = cj * Rp.re, ai = cj * Rp.im;
    P = cxe_red2(cx{P.re + ar, P.im + ai}, p, pinv);
    if (j) Rp = cxe_link(Rp, R, p, pinv);
  }
  if (n & 1u) P = cxe_link(P, r, p, pinv);
  return P;
}

// term x weight for a weight w in [0, p), reduced: 2 muls and 2 cxe_red.
SUP_CX_FN cx hafx_weigh(cx t, double w, double p, double pinv) {
  return cxe_red2(cx{t.re * w, t.im * w}, p, pinv);
}

// fp64 instructions per visited state and lane of walk_hafexact<LOOP> over the
// launches that `primes` primes take.  Shared by the primes of
// a launch: the q' update 4, the G' update 8 (W <= 4) or 20, r' 2 (loop).  Per
// prime: cxe_red2(q') 6; plain: 10 per link of the power; loop: cxe_red2(r') 6,
// R 10, per j 10 + 10 + 10 (no power step at j = 0), odd n 10; the weight 8 and
// the accumulate 2.  The fold every 256 states is not counted.
inline double hafx_ops_shared(int W, bool loop) { return 4.0 + (W <= 4 ? 8.0 : 20.0) + (loop ? 2.0 : 0.0); }
inline double hafx_ops_prime(int n, bool loop) {
  const int m = n / 2;
  double per = 6.0 + 8.0 + 2.0;
  if (!loop) {
    int top = 0, pop = 0;
    for (int b = 0; b < 31; ++b)
      if ((m >> b) & 1) top = b, ++pop;
    per += 10.0 * (top + pop - 1);
  } else {
    per += 6.0 + 10.0 + (m ? 30.0 * m - 10.0 : 0.0) + ((n & 1) ? 10.0 : 0.0);
  }
  return per;
}
inline double hafx_ops(int W, int n, bool loop, int primes) {
  const int launches = (primes + kHafxPrimes - 1) / kHafxPrimes;
  return (double)launches * hafx_ops_shared(W, loop) + (double)primes * hafx_ops_prime(n, loop);
}

}  // namespace sup
