// tor.hpp — what the torontonian kernel (walk_tor.hip), its host twin
// (torontonian.cpp) and its device runner (engine.cpp run_torontonian) share:
// the gathered matrix of a list, the chunking, and the order of every
// operation.  DESIGN.md §8j states the sum.
//
// O is 2M x 2M complex Hermitian (row i: mode i, row i + M: its conjugate
// partner); only its lower triangle and the real parts of its diagonal are
// read.  A list s of n distinct modes, nn = max(n, kTorW) positions (the
// positions b >= n are padding: identity rows no z selects).  The FULL row
// order puts the positions descending: full row R = 2 (nn - 1 - b) + h is row
// s_b + h M of O.  G = I - O_s in that order (tor_entry):
//   G[R][R] = 1.0 - Re O[p][p]                       (one rounding)
//   G[R][C] = -O[p][q] (p > q), -conj(O[q][p]) (p < q), C < R   (exact)
// M_z is G on the rows of the positions z selects, in full order: the rows of
// the high bits of z lead.  Its factor, row by row, columns ascending, one
// accumulator chain per entry (c <= r):
//   acc = M_z[r][c];  for l = 0 .. c-1 ascending: acc = tor_chain(acc, L[r][l], L[c][l])
//   c < r:  L[r][c] = (acc.re rho_c, acc.im rho_c)
//   c = r:  rho_r = tor_rho(acc.re)    (acc.im is never read)
//   f(z) = (..((1.0 rho_0) rho_1) ..) rho_last,  f(0) = 1.0
// tor_chain is four fmas (below); on the diagonal its re part alone
// (tor_chain_diag, the same two fmas).  tor_rho(d) = d > 0 ? 1.0 / sqrt(d) :
// NaN with the correctly rounded sqrt and division of both machines.
//
// Three things follow and the kernel uses all of them:
//  1. row r is a function of the selected positions at and above its own: a
//     row kept from the previous subset has the bits of a recomputed one;
//  2. a chain may pause after the columns of the leading rows (the prefix)
//     and go on over the others (the tail): the kernel keeps the prefix factor
//     and the tail rows' prefix columns T in LDS, pauses the chains of the
//     tail block S[t][u] = G[t][u] - sum_l T[t][l] conj(T[u][l]) there, and
//     each lane continues them over its own tail columns;
//  3. a position z does not select may stay as an identity row (every L[r][.]
//     and L[.][r] = +0, rho_r = 1.0): its terms are fma(-0 x, acc) or
//     fma(+0 x, acc) and leave a nonzero accumulator as it is.  An
//     accumulator that is -0 can become +0.  The sign of a zero never reaches
//     a result: a zero off the diagonal only ever multiplies into such terms
//     again, and a zero on the diagonal is no pivot (rho = NaN) whatever its
//     sign.  So the twin factors the compact matrix and the kernel the masked
//     one, and f(z) has the same bits (a NaN is a NaN: its payload is not
//     compared).  TOR_TWIN_TAIL (torontonian.cpp) runs the masked form on
//     the host.
//
// The low kTorW bits of z vary over the lanes of a wave, the lanes of a
// 64-aligned group of z add their (-1)^(n - |z|) f(z) (+0 outside the range)
// by the 64-lane xor butterfly (offsets 1, 2, .., 32, v = v + other), a
// wave-chunk of 2^tor_chunk_log(n) consecutive z adds its groups ascending
// from +0, and fock_fold reduces a list's chunk partials (pairs, im = 0).
#pragma once
#include <stdint.h>

#include "cplx_fock.hpp"
#include "cx.hpp"

namespace sup {

constexpr int kTorMaxN = 32;
#ifndef SUP_TOR_W
#define SUP_TOR_W 5  // 241 VGPRs and no scratch; 4 (169 VGPRs) was measured too and is slower
#endif
constexpr int kTorW = SUP_TOR_W;  // tail positions: the bits of z below it are a lane's own

// acc - a conj(b), per part by fma.
SUP_CX_FN cx tor_chain(cx acc, cx a, cx b) {
  double re = __builtin_fma(-a.re, b.re, acc.re);
  re = __builtin_fma(-a.im, b.im, re);
  double im = __builtin_fma(-a.im, b.re, acc.im);
  im = __builtin_fma(a.re, b.im, im);
  return cx{re, im};
}
// The re part of tor_chain(acc, a, a).
SUP_CX_FN double tor_chain_diag(double d, cx a) {
  d = __builtin_fma(-a.re, a.re, d);
  return __builtin_fma(-a.im, a.im, d);
}
SUP_CX_FN double tor_rho(double d) { return d > 0.0 ? 1.0 / __builtin_sqrt(d) : __builtin_nan(""); }
SUP_CX_FN cx tor_scale(cx acc, double rho) { return cx{acc.re * rho, acc.im * rho}; }

// log2 of the z values of one wave-chunk: a function of n only, at least one
// 64-aligned group, at most 2^15 chunks per list.
SUP_CX_FN int tor_chunk_log(int n) {
  int l = n < 9 ? n : 9;
  if (l < 6) l = 6;
  return n - 15 > l ? n - 15 : l;
}
SUP_CX_FN int tor_nn(int n) { return n > kTorW ? n : kTorW; }

// G[R][C] of the list s (n modes of O, 2M x 2M) in the full row order, any R, C.
SUP_CX_FN cx tor_entry(const double* O, int M, const int32_t* s, int n, int R, int C) {
  const int nn = tor_nn(n);
  const int br = nn - 1 - (R >> 1), bc = nn - 1 - (C >> 1);
  if (br >= n || bc >= n) return cx{R == C ? 1.0 : 0.0, 0.0};
  const uint64_t p = (uint64_t)s[br] + (uint64_t)(R & 1) * (uint64_t)M, q = (uint64_t)s[bc] + (uint64_t)(C & 1) * (uint64_t)M;
  const uint64_t ld = 2 * (uint64_t)M;
  if (p == q) return cx{1.0 - O[2 * (p * ld + p)], 0.0};
  // O[p][q] from O's lower triangle: the stored entry, or the conjugate of the
  // one across the diagonal
  const uint64_t a = p > q ? p : q, b = p > q ? q : p;
  const double re = -O[2 * (a * ld + b)], im = -O[2 * (a * ld + b) + 1];
  return p > q ? cx{re, im} : cx{re, -im};
}

// A slab: K lists of one order, every one with the same subsets [z_begin,
// z_end) and so the same cm wave-chunks; item a of the queue is chunk a % cm of
// list a / cm, and its partial goes to chunk_out[2 a] (im = 0).
struct TorParams {
  const double* G;        // 2 N N doubles per list, N = 2 nn, row-major
  unsigned long long chunk_count;
  double* chunk_out;
  unsigned int* counter;  // queue head (zeroed before launch)
  unsigned int group;     // chunks per ticket (1..64)
  unsigned int n, nn;
  unsigned int llog;      // tor_chunk_log(n)
  unsigned int cm;        // wave-chunks per list
  unsigned long long z_begin, z_end;  // z in [z_begin, z_end), z_end <= 2^n
  unsigned long long chunk_first;     // z_begin >> llog
};

inline uint64_t tor_g_doubles(int n) { return 8ull * (uint64_t)tor_nn(n) * (uint64_t)tor_nn(n); }

// The census: fp64 operations per subset as the kernel runs
// them, an fma counted as 2.  tail: a lane's masked 2W x 2W factor (chains 8
// per off-diagonal term and 4 per diagonal term, 2 per scaled entry, 3 per
// pivot: sqrt, division, product).  prefix: the wave-uniform work of one
// setting of the high bits, shared by its 2^W subsets: stepping z upwards
// brings in one new position (bit j of the high bits with probability
// 2^-(j+1), u of the bits above it set, binomial), so two new factor rows of
// P - 2 and P - 1 columns (P = 2 (u + 1)), two new columns of the 2W tail
// rows, and the W (2W + 1) paused chains of P terms.
inline double tor_ops_tail() {
  const int R = 2 * kTorW;
  double ops = 0.0;
  for (int r = 0; r < R; ++r) {
    for (int c = 0; c < r; ++c) ops += 8.0 * c + 2.0;
    ops += 4.0 * r + 3.0;
  }
  return ops + 1.0;  // the sign and the butterfly are not counted; the group add is
}
inline double tor_ops_prefix(int n) {
  const int H = n - kTorW;
  if (H <= 0) return 0.0;
  const int R = 2 * kTorW;
  double sum = 0.0, wsum = 0.0;
  for (int j = 0; j < H; ++j) {
    const double wj = j + 1 < H ? 1.0 / (double)(1ull << (j + 1)) : 1.0 / (double)(1ull << j);
    const int U = H - 1 - j;
    double wu = 1.0 / (double)(1ull << U);  // C(U, u) / 2^U
    for (int u = 0; u <= U; ++u) {
      const double P = 2.0 * (u + 1);
      double ops = 0.0;
      for (double i = P - 2.0; i < P; i += 1.0) ops += 8.0 * i * (i - 1.0) / 2.0 + 4.0 * i + 2.0 * i + 3.0;
      ops += R * (8.0 * (2.0 * P - 3.0) + 4.0);
      ops += kTorW * (R + 1.0) * 8.0 * P;
      sum += wj * wu * ops;
      wsum += wj * wu;
      wu = wu * (double)(U - u) / (double)(u + 1);
    }
  }
  return sum / wsum / (double)(1 << kTorW);
}
inline double tor_ops(int n) { return tor_ops_prefix(n) + tor_ops_tail(); }
// What the reuse is measured against: a fresh factor per subset, (2k)^3 / 6
// complex multiply-adds of 8 operations, binomial mean over k = |z|.
inline double tor_ops_plain(int n) {
  double w = 1.0 / (double)(1ull << n), sum = 0.0;  // C(n, k) / 2^n
  for (int k = 0; k <= n; ++k) {
    sum += w * 8.0 * (2.0 * k) * (2.0 * k) * (2.0 * k) / 6.0;
    w = w * (double)(n - k) / (double)(k + 1);
  }
  return sum;
}

}  // namespace sup
