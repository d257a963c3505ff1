// cxexact.hpp — residue arithmetic in (Z/p)[i] shared by the gfx950 exact
// complex walk (walk_cplxexact.hip) and its host twin (cplx_exact.cpp), and
// the launch parameters of that kernel.
//
// A residue of a Gaussian integer modulo a prime p < 2^42 is a pair (u, v) of
// fp64 values holding integers in (-1.5 p, 1.5 p), one per part.  Every
// operation below is exact (its true result is an integer below 2^53), so
// device and host agree residue for residue whatever the order of the sums:
//   cxe_red(t)        t - rint(t / p) p for an integer |t| < 2^53: the fma is
//                     exact, rint(t pinv) may be off by one, so the result
//                     lies in (-1.5 p, 1.5 p) — walk_exact.hip's red()
//   cxe_red2(y)       both parts of an exact Gaussian integer          6 ops
//   cxe_link(r, y)    r y for an exact Gaussian integer y = (c, d) with
//                     |c|, |d| <= Y: (red(uc - vd), red(ud + vc)).  cx_mul
//                     forms vd, then fma(u, c, -vd); |vd| < 1.5 p Y and
//                     |uc - vd| < 3 p Y, so 1.5 p Y < 2^52 keeps the product
//                     and the fma's one rounding exact.                10 ops
#pragma once
#include "cx.hpp"

namespace sup {

// Primes per launch of walk_cplxexact (its header comment says why 4).
#ifndef SUP_CXE_MAX_PRIMES
#define SUP_CXE_MAX_PRIMES 4  // (other values: the resource scans that chose it)
#endif
constexpr int kMaxCxPrimes = SUP_CXE_MAX_PRIMES;

struct CxExactParams {
  double prime[kMaxCxPrimes];
  double pinv[kMaxCxPrimes];  // 1 / p rounded
  int nprimes;
  int pad_;
  double* wave_out;  // [grid waves][kMaxCxPrimes][2]: each wave's residue sums (re, im), in [0, p)
};

SUP_CX_FN double cxe_red(double t, double p, double pinv) { return __builtin_fma(-__builtin_rint(t * pinv), p, t); }
SUP_CX_FN cx cxe_red2(cx y, double p, double pinv) { return cx{cxe_red(y.re, p, pinv), cxe_red(y.im, p, pinv)}; }
SUP_CX_FN cx cxe_link(cx r, cx y, double p, double pinv) { return cxe_red2(cx_mul(r, y), p, pinv); }

// est_ops_per_step of sup_stats (include/superman.h): fp64 VALU instructions
// per Gray step and lane of walk_cplxexact<n, G> with `primes` primes in the
// launch, K = ceil(n / G) group products:
//   2n                  the column add
//   4 floor(n / 2)      G = 2: the exact pair products (cx_mul), shared by every prime
//   primes (10 K - 2)   per prime: cxe_red2 (6), K - 1 links (10 each), the signed accumulate (2)
inline double cxe_ops_per_step(int n, int G, int primes) {
  const int K = (n + G - 1) / G;
  return 2.0 * n + (G == 2 ? 4.0 * (n / 2) : 0.0) + (double)primes * (10.0 * K - 2.0);
}

}  // namespace sup
