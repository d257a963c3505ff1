// hafpt.hpp — what the power-trace hafnian kernel (walk_hafpt.hip), its host
// twin (hafnian_pt.cpp) and its device runner (engine.cpp run_hafnian_pt)
// share: the table of a matrix, the chunking, and the order of every
// operation.  DESIGN.md §8i states the sum.
//
// Matrix k is the n x n symmetric gather N_ij = A[idx_i][idx_j], d_i =
// mu[idx_i] (loop form).  Odd n (loop form only): one virtual index with a
// zero row and column and d = 1.  np is the padded order, m = np / 2, NP =
// 8 ceil(np / 8) the table's row stride.  C[l][c] = N[l][c ^ 1] (C = N X).
//
// For z in [1, 2^m) with k bits set, the rows are r_0 < ... < r_{2k-1} = {2b,
// 2b + 1 : bit b of z}; row index i is compact (r_i the actual row, r_{i^1} =
// r_i ^ 1), column index l is actual and runs over the rows of z ascending.
//   P_1[i][c] = C[r_i][c]                                         (copied)
//   P_a[i][c] = sum_l cx_fma(P_{a-1}[i][l], C[l][c], .)  from +0, a = 2 .. ceil(m/2)
//   t_1 = W_i C[r_i][r_i]
//   t_j = W_i ( sum_l cx_fma(P_a[i][l], P_b[i^1][l^1], .) from +0 ),  a = ceil(j/2), b = floor(j/2), j = 2 .. m
//   y(0)_i = d[r_i];  y(j)_i = sum_l cx_fma(C[r_i][l], y(j-1)_{i(l)}, .) from +0
//   x_j = W_i cx_mul(d[r_i ^ 1], y(j-1)_i)                         (loop form), j = 1 .. m
// W_i is the 64-lane xor butterfly (offsets 1, 2, .., 32; cx_add) with the
// lanes i >= 2k holding +0.
//   c_j  = t_j * inv2[j]                    (plain: one multiply per part)
//   c_j  = fma(t_j, inv2[j], 0.5 * x_j)     (loop, per part)
//   jc_j = (double)j * c_j                  (per part)
//   g_0 = 1;  g_s = invs[s] * ( sum_{j=1..s} cx_fma(jc_j, g_{s-j}, .) from +0 )   (per part)
//   f(z) = g_m
// inv2[j] = 1 / (2j) and invs[s] = 1 / s are the host's table (hafpt_coef).
// A wave-chunk is L(m) = 2^hafpt_chunk_log(m) consecutive z; its partial is the
// ascending-z sum (cx_add, from +0) of f(z) for m - k even and -f(z) for m - k
// odd; fock_fold reduces a matrix's chunk partials.
#pragma once
#include <stdint.h>

#include "cplx_fock.hpp"
#include "cx.hpp"

namespace sup {

constexpr int kPtMaxM = 32;
constexpr int kPtCoef = 2 * (kPtMaxM + 1);  // inv2[0..32], then invs[0..32]

// s + a b, per part by fma: the first operand's parts are the multiplicands.
SUP_CX_FN cx cx_fma(cx a, cx b, cx s) {
  double re = __builtin_fma(a.re, b.re, s.re);
  re = __builtin_fma(-a.im, b.im, re);
  double im = __builtin_fma(a.re, b.im, s.im);
  im = __builtin_fma(a.im, b.re, im);
  return cx{re, im};
}

// log2 of the z values of one wave-chunk: at most 2^18 chunks per matrix.
SUP_CX_FN int hafpt_chunk_log(int m) { return m > 18 ? m - 18 : 0; }
inline int hafpt_pad8(int v) { return (v + 7) / 8 * 8; }

// The kernel instantiation a subset runs in: its columns reach 2 (top bit + 1),
// padded to 8.  (The columns past a subset's last row are never read.)
SUP_CX_FN int hafpt_kpad(uint64_t z) {
  int top = 0;
  while ((z >> (top + 1)) != 0ull) ++top;
  return (2 * (top + 1) + 7) / 8 * 8;
}

// A slab: K matrices of one order, every one with the same subsets [z_begin,
// z_end) and so the same cm wave-chunks; item a of the queue is chunk `local` =
// cm - 1 - a % cm of matrix a / cm (its subsets start at (chunk_first + local)
// L), and its partial goes to chunk_out[2 (cm (a / cm) + local)].
struct PtParams {
  const double* tabs;     // tab_doubles per matrix
  const double* coef;     // kPtCoef doubles
  unsigned long long chunk_count;
  double* chunk_out;      // 2 doubles (re, im) per wave-chunk
  unsigned int* counter;  // queue head (zeroed before launch)
  unsigned int group;     // chunks per ticket (1..64)
  unsigned int np, m;
  unsigned int llog;      // hafpt_chunk_log(m)
  unsigned int cm;        // wave-chunks per matrix
  unsigned int tab_doubles;
  unsigned long long z_begin, z_end;  // z in [max(1, z_begin), z_end), z_end <= 2^m
  unsigned long long chunk_first;     // z_begin >> llog
};

// Pairs in a matrix's table: np rows of NP pairs of C, then NP pairs of d.
inline uint64_t hafpt_pairs(int np) { return (uint64_t)(np + 1) * (uint64_t)hafpt_pad8(np); }

// Pair e of the table of the matrix gathered by idx (n indices) from A (M x M)
// and mu (null: the plain form, d = 0).
SUP_CX_FN cx hafpt_entry(const double* A, int M, const double* mu, const int32_t* idx, int n, int np, uint64_t e) {
  const int NP = (np + 7) / 8 * 8;
  const int l = (int)(e / (uint64_t)NP), c = (int)(e - (uint64_t)l * (uint64_t)NP);
  if (l == np) {  // d
    if (!mu || c >= np) return cx{0.0, 0.0};
    if (c >= n) return cx{1.0, 0.0};
    return cx{mu[2 * (uint64_t)idx[c]], mu[2 * (uint64_t)idx[c] + 1]};
  }
  const int j = c ^ 1;
  if (c >= np || l >= n || j >= n) return cx{0.0, 0.0};
  const double* p = A + 2 * ((uint64_t)idx[l] * (uint64_t)M + (uint64_t)idx[j]);
  return cx{p[0], p[1]};
}

// c_j, jc_j and g_s from the traces (see the head of this file).
SUP_CX_FN cx hafpt_cj(cx t, cx x, double inv2, bool loop) {
  if (!loop) return cx{t.re * inv2, t.im * inv2};
  const double hr = 0.5 * x.re, hi = 0.5 * x.im;
  return cx{__builtin_fma(t.re, inv2, hr), __builtin_fma(t.im, inv2, hi)};
}
SUP_CX_FN cx hafpt_scale(double s, cx v) { return cx{s * v.re, s * v.im}; }

// fp64 operations of one subset with k bits set, summed over its 2k rows and
// counted on the columns of the subset: the power steps 8 per
// (row, l, column), the traces 8 per (row, l) and 2 per row for the
// butterfly, the loop part 8 per (row, l) of y and 6 + 2 per row of x, the
// recurrence 8 per product and 6 per s.
inline double hafpt_ops_k(int m, int k, bool loop) {
  const double R = 2.0 * k, A = (m + 1) / 2;
  double ops = 8.0 * R * R * R * (A - 1.0);
  ops += (m - 1.0) * (8.0 * R * R + 2.0 * R) + 2.0 * R;
  if (loop) ops += (m - 1.0) * 8.0 * R * R + m * 8.0 * R;
  ops += 4.0 * m * (m + 1.0) + 6.0 * m;
  return ops;
}
// The mean over the subsets z in [1, 2^m), binomial weights.
inline double hafpt_ops(int m, bool loop) {
  if (m < 1) return 0.0;
  double w = 1.0, sum = 0.0, tot = 0.0;  // w = C(m, k)
  for (int k = 1; k <= m; ++k) {
    w = w * (double)(m - k + 1) / (double)k;
    sum += w * hafpt_ops_k(m, k, loop);
    tot += w;
  }
  return sum / tot;
}

}  // namespace sup
