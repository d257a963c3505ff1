// ltor.hpp — what the loop torontonian kernel (walk_ltor.hip), its host twin
// (loop_torontonian.cpp) and its device runner (engine.cpp
// run_loop_torontonian) share on top of tor.hpp: the border row, the
// exponential and the census.  DESIGN.md §8l states the sum.
//
//   ltor(O, gamma, s) = sum_z (-1)^(n - |z|) f(z),
//   f(z) = exp(1/2 gamma_z^H (I - O_z)^-1 gamma_z) / sqrt det(I - O_z),  f(0) = 1
//
// gamma is any complex vector of length 2M (entry i: mode i, entry i + M: its
// partner).  The loop term is one more row of tor.hpp's factor: border M_z =
// I - O_z with gamma_z, B = [[M_z, gamma_z], [gamma_z^H, 0]].  In tor.hpp's
// full row order the border row comes after all others; its entry in full
// column C is conj(gamma[p]) for the row p of O that tor_entry maps C to
// (ltor_border), +0 for a padding position.  Per selected column c ascending:
//   acc = conj gamma_c;  for l = 0 .. c-1 ascending: acc = tor_chain(acc, w_l, L[c][l])
//   w_c = tor_scale(acc, rho_c)
//   (a column of an unselected position keeps w_c = +0 in the masked form)
//   d = +0;  for l ascending: d = tor_chain_diag(d, w_l)
// w = conj(y) with L y = gamma_z, so -d = gamma_z^H (I - O_z)^-1 gamma_z and
//   f(z) = ((..(1.0 rho_0) ..) rho_last) ltor_exp(-0.5 d),  multiplied last.
// d is +0 or negative: the argument is -0 (exp = 1.0 exactly: gamma = 0 gives
// the torontonian's bits) or positive.  The border row depends only on the
// selected positions at and above each column, like any other row, so tor.hpp's
// three consequences (kept rows, paused chains, masked rows) hold for it too.
// The sign, the butterfly, tor_chunk_log(n), the chunk sum and fock_fold are
// the torontonian's.
#pragma once
#include <stdint.h>

#include "tor.hpp"

namespace sup {

#ifndef SUP_LTOR_W
#define SUP_LTOR_W 4  // 252 VGPRs, no spills; 5 fills all 256 and spills 8 VGPRs (into AGPRs), so it is not taken
#endif
constexpr int kLtorW = SUP_LTOR_W;  // tail positions of walk_ltor.hip (the bits do not depend on it)
static_assert(kLtorW >= 1 && kLtorW <= kTorW && kLtorW <= 6, "tor_nn pads a list to kTorW positions: the tail must fit in them");

// exp(x) from fma, multiply, round-to-nearest-integer and exponent-field
// arithmetic only, each correctly rounded on the host and on the device: the
// same bits on both.  k = rint(x log2 e), r = x - k ln 2 by two fmas
// (Cody-Waite, ln 2 = hi + lo), the degree-13 Taylor polynomial of exp(r) by
// Horner fmas (|r| <= 0.347: remainder below 0.05 ulp), then two exact powers
// of two built in the exponent field (k = k1 + k2, both normal for every k a
// finite result has; the last product rounds once, into the subnormals too).
// NaN gives NaN, x > 711 gives +inf (the products overflow to +inf on their
// own from log(DBL_MAX) on), x < -750 gives +0 (they round to +0 on their own
// below -745.14).  exp(+-0) = 1.0 exactly.  Worst error measured against
// 60-digit references: DESIGN.md §8l.
SUP_CX_FN double ltor_pow2(int e) {  // 2^e, -1022 <= e <= 1023
  const uint64_t bits = (uint64_t)(e + 1023) << 52;
  double v;
  __builtin_memcpy(&v, &bits, sizeof(v));
  return v;
}
SUP_CX_FN double ltor_exp(double x) {
  if (x != x) return x;
  if (x > 711.0) return __builtin_inf();
  if (x < -750.0) return 0.0;
  const double k = __builtin_rint(x * 0x1.71547652b82fep+0);
  double r = __builtin_fma(-k, 0x1.62e42fefa39efp-1, x);
  r = __builtin_fma(-k, 0x1.abc9e3b39803fp-56, r);
  double p = 1.0 / 6227020800.0;
  p = __builtin_fma(p, r, 1.0 / 479001600.0);
  p = __builtin_fma(p, r, 1.0 / 39916800.0);
  p = __builtin_fma(p, r, 1.0 / 3628800.0);
  p = __builtin_fma(p, r, 1.0 / 362880.0);
  p = __builtin_fma(p, r, 1.0 / 40320.0);
  p = __builtin_fma(p, r, 1.0 / 5040.0);
  p = __builtin_fma(p, r, 1.0 / 720.0);
  p = __builtin_fma(p, r, 1.0 / 120.0);
  p = __builtin_fma(p, r, 1.0 / 24.0);
  p = __builtin_fma(p, r, 1.0 / 6.0);
  p = __builtin_fma(p, r, 0.5);
  p = __builtin_fma(p, r, 1.0);
  p = __builtin_fma(p, r, 1.0);
  const int ki = (int)k, k1 = ki / 2, k2 = ki - k1;
  return (p * ltor_pow2(k1)) * ltor_pow2(k2);
}
constexpr double kLtorExpOps = 34.0;  // 1 product, 1 rint, 15 fmas, 2 scalings

// The border row's entry in full column C of the list s: conj(gamma[p]).
SUP_CX_FN cx ltor_border(const double* gamma, int M, const int32_t* s, int n, int C) {
  const int bc = tor_nn(n) - 1 - (C >> 1);
  if (bc >= n) return cx{0.0, 0.0};
  const uint64_t p = (uint64_t)s[bc] + (uint64_t)(C & 1) * (uint64_t)M;
  return cx{gamma[2 * p], -gamma[2 * p + 1]};
}

// A list's gathered data: G (tor.hpp, N = 2 nn rows of N pairs) and the border
// as row N.
inline uint64_t ltor_g_doubles(int n) { return 4ull * (uint64_t)tor_nn(n) * (2ull * (uint64_t)tor_nn(n) + 1ull); }

// The census: tor.hpp's, with kLtorW for the cut, plus the
// border.  tail: 2W chains of c terms and a scaling, the diagonal chain of 2W
// terms, the argument's product, the exponential and the last product.
// prefix: the border is one more tail row (two new columns) and brings 2W
// paused off-diagonal chains and the paused diagonal chain of P terms.
inline double ltor_ops_tail() {
  const int R = 2 * kLtorW;
  double ops = 0.0;
  for (int r = 0; r < R; ++r) {
    for (int c = 0; c < r; ++c) ops += 8.0 * c + 2.0;
    ops += 4.0 * r + 3.0;
  }
  ops += 1.0;  // the group add
  for (int c = 0; c < R; ++c) ops += 8.0 * c + 2.0;
  return ops + 4.0 * R + 1.0 + kLtorExpOps + 1.0;
}
inline double ltor_ops_prefix(int n) {
  const int H = n - kLtorW;
  if (H <= 0) return 0.0;
  const int R = 2 * kLtorW;
  double sum = 0.0, wsum = 0.0;
  for (int j = 0; j < H; ++j) {
    const double wj = j + 1 < H ? 1.0 / (double)(1ull << (j + 1)) : 1.0 / (double)(1ull << j);
    const int U = H - 1 - j;
    double wu = 1.0 / (double)(1ull << U);  // C(U, u) / 2^U
    for (int u = 0; u <= U; ++u) {
      const double P = 2.0 * (u + 1);
      double ops = 0.0;
      for (double i = P - 2.0; i < P; i += 1.0) ops += 8.0 * i * (i - 1.0) / 2.0 + 4.0 * i + 2.0 * i + 3.0;
      ops += (R + 1.0) * (8.0 * (2.0 * P - 3.0) + 4.0);
      ops += kLtorW * (R + 1.0) * 8.0 * P + R * 8.0 * P + 4.0 * P;
      sum += wj * wu * ops;
      wsum += wj * wu;
      wu = wu * (double)(U - u) / (double)(u + 1);
    }
  }
  return sum / wsum / (double)(1 << kLtorW);
}
inline double ltor_ops(int n) { return ltor_ops_prefix(n) + ltor_ops_tail(); }

}  // namespace sup
