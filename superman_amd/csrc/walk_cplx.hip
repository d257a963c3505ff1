// walk_cplx.hip — the dense Ryser / Gray-code walk over complex fp64 values for
// gfx950: permanents of dense complex matrices (boson-sampling amplitudes),
// which the reference refuses ("SUPerman does not support complex type",
// revised_perman/main.cpp:1557).
//
// Enumeration, lane layout and wave-chunk queue are walk_dense.hip's
// (walk_common.hpp); every value of the walk is a cx (cx.hpp):
//   x_j(S) = x0_j + sum_{c in S} a_jc   (cx_add_d2: the column's Re and Im
//                                        planes, each as SGPR operands)
//   term   = prod_j x_j                 (4 strided cx partial products,
//                                        combined as (p0 p1)(p2 p3))
//   acc   +- term by step parity        (cx_add / cx_sub)
// Per Gray step and lane: 2n + 4(n-1) + 2 = 6n - 2 fp64 VALU ops (~3x the
// fp64 walk's 2n + 1).  Each wave-chunk's partial leaves as (re, im); the host
// adds the partials in a fixed pairwise order, and cplx.cpp's host twin runs
// the same cx.hpp operations in the same order: results are bit-identical on
// the GPU, on any device count and on host threads.
//
// Tables: p.cols holds two planes, Re then Im of the signed column table, each
// in the 2(n-1) x NP layout (the Im plane kImOff bytes after the Re plane);
// p.x0 is 2 NP doubles (re block, then im block); p.chunk_out 2 doubles per
// wave-chunk (re, im).  No chunk-end check (WalkParams::umask is not read):
// that serves sparse integer inputs, this walk is for dense complex ones.
//
// Registers: 4n VGPRs hold x (the double-double walk's picture); the compiler
// allocates 4n + ~31.  Compiler resource report and a scan of the generated
// code per N (profiles/complex/walk_cplx_resources.log):
//   N        waves/SIMD asked  VGPRs (+AGPRs)       spilled VGPRs  scratch
//   1..16    2                 21..119              0              0
//   17..32   2                 101..162             0              0
//   33..55   2                 166..255             0              0
//   56..64   1                 256 (+6..64 AGPRs)   0              0
// No N spills a VGPR or touches scratch anywhere in the kernel.  The walk loop
// (one odd + one even Gray step) holds exactly 2(6n - 2) fp64 VALU
// instructions and no readlane at every N; from N = 59 it also moves 8..160
// values between AGPRs and VGPRs per pair of steps (x no longer fits 256
// VGPRs beside the products).  SGPR spills (8..243, to VGPR lanes) are in the
// chunk start only.  Up to N = 55 the kernel is asked for 2 waves per SIMD
// (256 VGPRs); at N = 56 that request spills 6 VGPRs, so 56..64 take 1 wave.
// Measured on 16384-chunk ranges, 2 waves against 1: 23-33 % faster at
// N = 31..52 (profiles/complex/range_scan_*.log).
#include "cx.hpp"
#include "cx_cols.hpp"
#include "kernels.hpp"
#include "walk_common.hpp"

namespace sup {

#ifndef SUP_CPLX_TWO_WAVES_MAX
#define SUP_CPLX_TWO_WAVES_MAX 55  // largest N asked for 2 waves per SIMD (256 VGPRs)
#endif

// Four strided partial products, combined as (p0 p1)(p2 p3) — prod4's shape.
template <int N>
__device__ __forceinline__ cx cx_prod4(const cx (&x)[N]) {
  const cx one{1.0, 0.0};
  cx p0 = x[0];
  cx p1 = N > 1 ? x[1 < N ? 1 : 0] : one;
  cx p2 = N > 2 ? x[2 < N ? 2 : 0] : one;
  cx p3 = N > 3 ? x[3 < N ? 3 : 0] : one;
#pragma unroll
  for (int j = 4; j < N; j += 4) {
    p0 = cx_mul(p0, x[j]);
    if (j + 1 < N) p1 = cx_mul(p1, x[j + 1 < N ? j + 1 : 0]);
    if (j + 2 < N) p2 = cx_mul(p2, x[j + 2 < N ? j + 2 : 0]);
    if (j + 3 < N) p3 = cx_mul(p3, x[j + 3 < N ? j + 3 : 0]);
  }
  if (N == 1) return p0;
  if (N == 2) return cx_mul(p0, p1);
  if (N == 3) return cx_mul(cx_mul(p0, p1), p2);
  return cx_mul(cx_mul(p0, p1), cx_mul(p2, p3));
}

// 64-lane pairwise sum of re and im (ascending xor offsets; IEEE addition is
// commutative, so every lane ends with the same value).
__device__ __forceinline__ cx cx_wave_sum(cx v) {
#pragma unroll
  for (int off = 1; off <= 32; off <<= 1) {
    const cx o{__shfl_xor(v.re, off, 64), __shfl_xor(v.im, off, 64)};
    v = cx_add(v, o);
  }
  return v;
}

template <int N>
__global__ __launch_bounds__(kBlock)
    __attribute__((amdgpu_waves_per_eu(N <= SUP_CPLX_TWO_WAVES_MAX ? 2 : 1))) void walk_cplx(WalkParams p) {
  constexpr int NP = pad8(N);
  constexpr uint32_t kImOff = 2u * (uint32_t)(N > 1 ? N - 1 : 1) * NP * 8u;  // bytes from the Re to the Im plane
  const uint32_t lane = threadIdx.x & 63u;
  const bool lane_valid = lane < (1u << p.L);
  const uint32_t lane_par = __builtin_popcount(lane) & 1u;
  const uint32_t T = 1u << p.m;
  const uint32_t offL = 2u * (uint32_t)p.L * NP * 8u;  // engine bit L = walk bit 0

  // x += the column at byte offset `off` of both planes
  auto step = [&](cx(&x)[N], uint32_t off) {
    cx_add_col<N>(x, opaque_c(p.cols, off), opaque_c(p.cols, kImOff + off));
  };

  for (uint32_t g = next_chunk(p.counter); (uint64_t)g * p.group < p.chunk_count; g = next_chunk(p.counter)) {
    cx keep{0.0, 0.0};  // lane j keeps the partial of chunk g*p.group + j
    for (uint32_t j = 0; j < (uint32_t)p.group; ++j) {
      const uint64_t a = (uint64_t)g * p.group + j;
      if (a >= p.chunk_count) break;
      const uint64_t ga = p.chunk_begin + a;
      // chunk start (chunk_start's order: x0, high bits ascending, lane bits ascending)
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
        for (int e = 0; e < p.L; ++e) {
          cdbl* cre = opaque_c(p.cols, (2u * e) * NP * 8u);
          cdbl* cim = opaque_c(p.cols, kImOff + (2u * e) * NP * 8u);
          cx_add_col<N, true>(x, cre, cim, (lane >> e) & 1u);  // x + (on ? column : 0.0)
        }
      }
      cx acc = cx_prod4<N>(x);  // t = 0
      uint32_t t = 1;
      // odd t flips walk bit 0 (term sign -), even t walk bit ctz(t) (sign +)
      for (; t + 1 < T; t += 2) {
        step(x, offL + ((t >> 1) & 1u) * NP * 8u);
        acc = cx_sub(acc, cx_prod4<N>(x));
        const uint32_t u = t + 1;
        const uint32_t k = (uint32_t)__builtin_ctz(u);
        const uint32_t neg = (u >> (k + 1)) & 1u;
        step(x, offL + (2u * k + neg) * NP * 8u);
        acc = cx_add(acc, cx_prod4<N>(x));
      }
      if (t < T) {
        step(x, offL + ((t >> 1) & 1u) * NP * 8u);
        acc = cx_sub(acc, cx_prod4<N>(x));
      }
      if (((uint32_t)ga ^ lane_par) & 1u) acc = cx_neg(acc);
      const cx part = cx_wave_sum(lane_valid ? acc : cx{0.0, 0.0});
      if (lane == j) keep = part;
    }
    const uint64_t a = (uint64_t)g * p.group + lane;
    if (lane < (uint32_t)p.group && a < p.chunk_count) {
      p.chunk_out[2 * a] = keep.re;
      p.chunk_out[2 * a + 1] = keep.im;
    }
  }
}

template <int N, int HI>
static hipError_t launch_rec(int n, const WalkParams& p, int grid, hipStream_t s) {
  if (n == N) {
    hipLaunchKernelGGL(walk_cplx<N>, dim3(grid), dim3(kBlock), 0, s, p);
    return hipGetLastError();
  }
  if constexpr (N < HI) return launch_rec<N + 1, HI>(n, p, grid, s);
  return hipErrorInvalidValue;
}

template <int N, int HI>
static hipError_t occ_rec(int n, int* blocks_per_cu) {
  if (n == N) return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, walk_cplx<N>, kBlock, 0);
  if constexpr (N < HI) return occ_rec<N + 1, HI>(n, blocks_per_cu);
  return hipErrorInvalidValue;
}

#define SUP_CAT2(a, b) a##b
#define SUP_CAT(a, b) SUP_CAT2(a, b)

hipError_t SUP_CAT(launch_cplx_, SUP_N_LO)(int n, const WalkParams& p, int grid, hipStream_t s) {
  return launch_rec<SUP_N_LO, SUP_N_HI>(n, p, grid, s);
}
hipError_t SUP_CAT(occupancy_cplx_, SUP_N_LO)(int n, int* blocks_per_cu) {
  return occ_rec<SUP_N_LO, SUP_N_HI>(n, blocks_per_cu);
}

}  // namespace sup
