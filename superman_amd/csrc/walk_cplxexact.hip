// walk_cplxexact.hip — exact permanent of a matrix of Gaussian integers: the
// dense Ryser / Gray-code walk of walk_cplx.hip in residue arithmetic over
// (Z/p)[i], for gfx950.
//
// Enumeration, lane layout, chunk start order, tables and the column add
// (cx_add_col, cx_cols.hpp: SGPR operands in pieces of at most 32 rows) are
// walk_cplx.hip's, on the doubled matrix 2A, so every row value
//   X_j(S) = 2 a_j,n-1 - sum_c a_jc + 2 sum_{e in S} a_je,  |Re X_j|, |Im X_j| <= R_j,
// is a Gaussian integer held exactly in two fp64 values (R_j = sum_c |Re a_jc|
// + |Im a_jc| < 2^31).  The residue machinery is walk_exact.hip's, per prime
// and per part (cxexact.hpp): rows multiplied exactly in groups of G = 1 or 2
// (cx_mul, shared by every prime), a chain of cxe_link over the group
// products, a signed accumulate by step parity, acc folded with cxe_red every
// 256 steps, then the subset-parity flip, the lane-valid mask, an exact
// 64-lane sum, canonicalisation into [0, p) and one vector store per wave,
// prime and part.  The host joins the residues of
//   T = sum_S (-1)^|S| prod_j X_j(S),  perm = (4(n&1) - 2) T / 2^n,
// by CRT, each part on its own (cplx_exact.cpp).
// Exactness: a link multiplies a residue (|u|, |v| < 1.5 p) by a group product
// with parts <= Y; 1.5 p Y < 2^52 keeps it exact (cxexact.hpp).  G = 1:
// Y < 2^xbits, G = 2: Y <= 2 4^xbits; the host picks p < 2^pbits with pbits =
// min(42, 51 - log2 Y).  acc grows by < 1.5 p per step: < 2^51 over 256 steps.
// No chunk-end check (WalkParams::umask is not read).
//
// Walk loop: one even + one odd Gray step, blocks of 256 steps between folds,
// so the loop itself holds no fold, and no step is peeled out of it (the
// chunk start is one column back, so that step 0 is an even step like the
// others): 2 cxe_ops_per_step(N, G, kMaxCxPrimes) fp64
// VALU instructions (cxexact.hpp: per step 2N + [G = 2] 4 floor(N/2) +
// primes (10 ceil(N/G) - 2)).  The primes go in pairs, two chains side by
// side (each group product is read once for both; from N ~ 56 part of X lives
// in AGPRs and every read of it is a move); a launch with two primes branches
// round the second pair (one scalar branch per pair and step).  The host pads
// an odd count with a repeat of its last prime and drops that result.
//
// Primes per launch: kMaxCxPrimes = 4.  The state is 4N VGPRs of X, 4K of
// group products at G = 2, and 8 per prime (acc and the wave's totals, two
// parts each): beside 256 VGPRs of X at N = 64 the real kernel's 8 primes do
// not fit.  The scan that chose the constant (N = 61..64 of an earlier form of
// this loop, one chain at a time): with 8 primes N = 61 spills 67 VGPRs at
// G = 2 where 4 primes spill none; with 2 or 3 primes N = 64 still spills (4 to
// 81 VGPRs), so fewer primes buy no higher cap, and every launch repeats the
// column adds and pair products.  More primes than 4 take several launches
// (cplx_exact.cpp).
// Device cap: SUP_CPLX_EXACT_MAX_DEVICE_N = 61 (include/superman.h), the
// largest N up to which every N compiles with no scratch and no spilled VGPR
// for both G.  Compiler resource report and a scan of the generated code per
// (N, G) (profiles/complex_exact/walk_cplxexact_resources.log,
// tools/probes/cplx_resources.py exact; above the cap:
// walk_cplxexact_resources_above_the_cap.log):
//   G  N        waves/SIMD  VGPRs (+AGPRs)      spilled VGPRs  scratch  AGPR moves per pair of steps
//   1  1..12    8..5        48..95              0              0        0
//   1  13..30   4..3        99..168             0              0        0
//   1  31..51   2           172..254            0              0        0
//   1  52..60   1           255, 256 (+1..32)   0              0        0..56
//   1  61       1           256 (+204)          0              0        760
//   1  62..64   1           256 (+250..256)     42..114        0..72    1062..1104
//   2  1..8     8..5        48..94              0              0        0
//   2  9..20    4..3        98..167             0              0        0
//   2  21..35   2           171..256            0              0        0
//   2  36..61   1           255, 256 (+8..206)  0              0        0..656
//   2  62       1           256 (+214)          0              0        692
//   2  63, 64   1           256 (+256)          50, 128        76, 148  828, 836
// At every instantiated (N, G) the walk loop holds exactly
// 2 cxe_ops_per_step(N, G, 4) fp64 VALU instructions, no scratch instruction
// and no readlane; the SGPR spills (up to 253, to VGPR lanes) are in the chunk
// start only.  From N = 57 (G = 1) and N = 40 (G = 2) part of the state lives in
// AGPRs and moves every step.  G = 1 at N = 62 is the first instance that
// spills, so the cap is 61 although G = 2 compiles clean at 62.  The waves per
// SIMD are the compiler's choice at every N: no request is made.
#include "cx_cols.hpp"
#include "cxexact.hpp"
#include "kernels.hpp"
#include "walk_common.hpp"

namespace sup {

template <int N, int G>
struct CxGroups {
  static constexpr int K = (N + G - 1) / G;
};

// y_k = the exact product of the rows of group k (G = 1: the row itself).
template <int N, int G>
__device__ __forceinline__ void cxe_group_products(const cx (&x)[N], cx (&y)[CxGroups<N, G>::K]) {
#pragma unroll
  for (int k = 0; k < CxGroups<N, G>::K; ++k) {
    cx v = x[k * G];
    if constexpr (G == 2)
      if (2 * k + 1 < N) v = cx_mul(v, x[(2 * k + 1 < N) ? 2 * k + 1 : 0]);
    y[k] = v;
  }
}

// prod_k y_k in (Z/p)[i] for two primes at once: cxe_red2(y_0), then one
// cxe_link per further group, the two chains side by side so that each group
// product is read once for both and neither chain waits on its own last result.
template <int K>
__device__ __forceinline__ void cxe_chain2(const cx (&y)[K], double p0, double i0, double p1, double i1, cx& r0,
                                           cx& r1) {
  r0 = cxe_red2(y[0], p0, i0);
  r1 = cxe_red2(y[0], p1, i1);
#pragma unroll
  for (int k = 1; k < K; ++k) {
    r0 = cxe_link(r0, y[k], p0, i0);
    r1 = cxe_link(r1, y[k], p1, i1);
  }
}

// term(x) mod every prime of the launch, added to (SUB false) or subtracted
// from acc.  Primes go in pairs (e.nprimes is even: the host repeats the last
// prime of an odd count and drops its result): one scalar branch per pair.
template <int N, int G, bool SUB>
__device__ __forceinline__ void cxe_terms(const cx (&x)[N], const CxExactParams& e, cx (&acc)[kMaxCxPrimes]) {
  cx y[CxGroups<N, G>::K];
  cxe_group_products<N, G>(x, y);
#pragma unroll
  for (int q = 0; q < kMaxCxPrimes; q += 2)
    if (q < e.nprimes) {
      cx r0, r1;
      cxe_chain2<CxGroups<N, G>::K>(y, e.prime[q], e.pinv[q], e.prime[q + 1], e.pinv[q + 1], r0, r1);
      if constexpr (SUB) {
        acc[q] = cx_sub(acc[q], r0), acc[q + 1] = cx_sub(acc[q + 1], r1);
      } else {
        acc[q] = cx_add(acc[q], r0), acc[q + 1] = cx_add(acc[q + 1], r1);
      }
    }
}

template <int N, int G>
__global__ __launch_bounds__(kBlock) void walk_cplxexact(WalkParams p, CxExactParams e) {
  constexpr int NP = pad8(N);
  constexpr uint32_t kImOff = 2u * (uint32_t)(N > 1 ? N - 1 : 1) * NP * 8u;  // bytes from the Re to the Im plane
  const uint32_t lane = threadIdx.x & 63u;
  const bool lane_valid = lane < (1u << p.L);
  const uint32_t lane_par = __builtin_popcount(lane) & 1u;
  const uint32_t T = 1u << p.m;
  const uint32_t offL = 2u * (uint32_t)p.L * NP * 8u;  // engine bit L = walk bit 0

  auto step = [&](cx(&x)[N], uint32_t off) {
    cx_add_col<N>(x, opaque_c(p.cols, off), opaque_c(p.cols, kImOff + off));
  };

  cx tot[kMaxCxPrimes];  // this lane's share of the wave's chunks, per prime
#pragma unroll
  for (int q = 0; q < kMaxCxPrimes; ++q) tot[q] = cx{0.0, 0.0};

  for (uint32_t g = next_chunk(p.counter); (uint64_t)g < p.chunk_count; g = next_chunk(p.counter)) {
    const uint64_t ga = p.chunk_begin + g;
    // chunk start (walk_cplx's order: x0, high bits ascending, lane bits ascending)
    cx x[N];
    {
      cdbl* x0 = opaque_c(p.x0, 0);
#pragma unroll
      for (int r = 0; r < N; ++r) x[r] = cx{x0[r], x0[NP + r]};
      uint64_t h = ga ^ (ga >> 1);
      const uint32_t hb = (uint32_t)(p.L + p.m);
      while (h) {
        const uint32_t b = (uint32_t)__builtin_ctzll(h);
        h &= h - 1;
        step(x, (2u * (hb + b)) * NP * 8u);
      }
      for (int b = 0; b < p.L; ++b) {
        cdbl* cre = opaque_c(p.cols, (2u * b) * NP * 8u);
        cdbl* cim = opaque_c(p.cols, kImOff + (2u * b) * NP * 8u);
        cx_add_col<N, true>(x, cre, cim, (lane >> b) & 1u);
      }
    }
    // The walk has no peeled first or last step (a second and third copy of the
    // term code outside the loop cost registers at large N): the chunk start
    // subtracts walk bit 0's column (its - entry), and step t = 0 adds it back
    // like any even step, exactly, since X holds integers.  No walk bits
    // (T = 1): the one term, no column.
    const bool walks = T > 1u;
    if (walks) step(x, offL + NP * 8u);
    cx acc[kMaxCxPrimes];
#pragma unroll
    for (int q = 0; q < kMaxCxPrimes; ++q) acc[q] = cx{0.0, 0.0};
    // even t flips walk bit ctz(t) (t = 0: see above; term sign +), odd t walk
    // bit 0 (sign -); steps 256 b .. 256 b + 255 form a block, acc is folded after each
    for (uint32_t t0 = 0; t0 < T; t0 += 256u) {
      const uint32_t lim = t0 + 256u < T ? t0 + 256u : T;
      for (uint32_t t = t0; t < lim; t += 2) {
        if (walks) {
          const uint32_t k = (uint32_t)__builtin_ctz(t | 0x40000000u);  // t < 2^31; t = 0: 30, not used
          const uint32_t neg = (t >> (k + 1)) & 1u;
          step(x, offL + (t ? 2u * k + neg : 0u) * NP * 8u);
        }
        cxe_terms<N, G, false>(x, e, acc);
        if (walks) {
          step(x, offL + ((t >> 1) & 1u) * NP * 8u);  // t + 1
          cxe_terms<N, G, true>(x, e, acc);
        }
      }
#pragma unroll
      for (int q = 0; q < kMaxCxPrimes; ++q)
        if (q < e.nprimes) acc[q] = cxe_red2(acc[q], e.prime[q], e.pinv[q]);
    }
    // subset parity = parity(gray(ga)) ^ parity(lane) ^ parity(g(t)), the last
    // folded into the alternating signs above
    const bool flip = ((uint32_t)ga ^ lane_par) & 1u;
#pragma unroll
    for (int q = 0; q < kMaxCxPrimes; ++q)
      if (q < e.nprimes) {
        const cx a = cxe_red2(acc[q], e.prime[q], e.pinv[q]);
        const cx s = lane_valid ? (flip ? cx_neg(a) : a) : cx{0.0, 0.0};
        tot[q] = cxe_red2(cx_add(tot[q], s), e.prime[q], e.pinv[q]);
      }
  }
  // 64 lanes, |tot| < 1.5 p each part: the plain sum is exact; store it in [0, p)
  const uint32_t wave = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
#pragma unroll
  for (int q = 0; q < kMaxCxPrimes; ++q)
    if (q < e.nprimes) {
      cx v = tot[q];
#pragma unroll
      for (int off = 1; off <= 32; off <<= 1) v = cx_add(v, cx{__shfl_xor(v.re, off, 64), __shfl_xor(v.im, off, 64)});
      const double pq = e.prime[q];
      double r[2] = {cxe_red(v.re, pq, e.pinv[q]), cxe_red(v.im, pq, e.pinv[q])};
#pragma unroll
      for (int part = 0; part < 2; ++part) {
        if (r[part] < 0.0) r[part] += pq;
        if (r[part] < 0.0) r[part] += pq;
        if (r[part] >= pq) r[part] -= pq;
        if (lane == 0) e.wave_out[((uint64_t)wave * kMaxCxPrimes + q) * 2u + part] = r[part];
      }
    }
}

template <int N, int HI>
static hipError_t launch_rec(int n, int g, const WalkParams& p, const CxExactParams& e, int grid, hipStream_t s) {
  if (n == N) {
    switch (g) {
      case 2: hipLaunchKernelGGL((walk_cplxexact<N, 2>), dim3(grid), dim3(kBlock), 0, s, p, e); break;
      case 1: hipLaunchKernelGGL((walk_cplxexact<N, 1>), dim3(grid), dim3(kBlock), 0, s, p, e); break;
      default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
  }
  if constexpr (N < HI) return launch_rec<N + 1, HI>(n, g, p, e, grid, s);
  return hipErrorInvalidValue;
}

template <int N, int HI>
static hipError_t occ_rec(int n, int g, int* blocks_per_cu) {
  if (n == N) {
    switch (g) {
      case 2: return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, walk_cplxexact<N, 2>, kBlock, 0);
      case 1: return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, walk_cplxexact<N, 1>, kBlock, 0);
      default: return hipErrorInvalidValue;
    }
  }
  if constexpr (N < HI) return occ_rec<N + 1, HI>(n, g, blocks_per_cu);
  return hipErrorInvalidValue;
}

#define SUP_CAT2(a, b) a##b
#define SUP_CAT(a, b) SUP_CAT2(a, b)

hipError_t SUP_CAT(launch_cplxexact_, SUP_N_LO)(int n, int g, const WalkParams& p, const CxExactParams& e, int grid,
                                                hipStream_t s) {
  return launch_rec<SUP_N_LO, SUP_N_HI>(n, g, p, e, grid, s);
}
hipError_t SUP_CAT(occupancy_cplxexact_, SUP_N_LO)(int n, int g, int* blocks_per_cu) {
  return occ_rec<SUP_N_LO, SUP_N_HI>(n, g, blocks_per_cu);
}

}  // namespace sup
