// walk_cplxdd.hip — the dense Ryser / Gray-code walk over complex
// double-double values for gfx950: permanents of dense complex fp64 matrices
// to ~100 bits, the ground truth the fp64 complex walk (walk_cplx.hip) is
// judged against, as walk_dd.hip is for the real walks.
//
// Enumeration, lane layout, wave-chunk queue, chunk start order and sign
// handling are walk_cplx.hip's; every value of the walk is a cxdd (cxdd.hpp):
//   x_j(S) = x0_j + sum_{c in S} a_jc   (cxdd_add_d2: dd_add_d on each part,
//                                        the column's planes as SGPR operands)
//   term   = prod_j x_j                 (4 strided cxdd partial products,
//                                        combined as (p0 p1)(p2 p3))
//   acc   += (-1)^t term                (cxdd_add, cxdd_neg)
// Per Gray step and lane: 18n + 68(n-1) + 40 = 86n - 28 fp64 VALU ops (14.3x
// the fp64 complex walk's 6n - 2 at n = 30).  Each wave-chunk's partial
// leaves as (re.hi, re.lo, im.hi, im.lo); the host adds the partials in a
// fixed pairwise order, and cplx_quad.cpp's host twin runs the same cxdd.hpp
// operations in the same order: results are bit-identical on the GPU, on any
// device count and on host threads.
//
// Tables: p.cols is cplx_plan's (Re plane, then the Im plane kImOff bytes
// after it, each 2(n-1) x NP); p.x0 is 4 NP doubles in four blocks (re.hi,
// re.lo, im.hi, im.lo); p.chunk_out 4 doubles per wave-chunk.  No chunk-end
// check (WalkParams::umask is not read).
//
// The op count follows dd.hpp's nominal figures (dd_add_d 9); dd_add_d is 10
// instructions (a 6-instruction two_sum, an add, a fast_two_sum), so the walk
// loop holds 88n - 28 fp64 VALU instructions per step, which is what the
// resource log checks.
//
// Registers: 8n VGPRs hold x.  Compiler resource report and a scan of the
// generated code per N (profiles/complex_quad/walk_cplxdd_resources.log,
// tools/probes/cplx_resources.py quad):
//   N        waves/SIMD  VGPRs (+AGPRs)        spilled VGPRs  scratch  AGPR moves per pair of steps
//   1..12    8..3        56..165               0              0        0
//   13..23   2           181..254              0              0        0
//   24       1           255 (+8)              0              0        0
//   25..32   1           256 (+18..126)        0              0        10..480
//   33..40   1           256 (+124..226)       0              0        472..1002
//   41, 42   1           256 (+206, 220)       0              0        982, 1028 (41: one v_readlane in the loop)
//   43, 44   1           256 (+256)            12, 30         20, 60   1154, 1358
// The kernel is instantiated for N <= SUP_CPLX_QUAD_MAX_DEVICE_N = 40 only
// (include/superman.h): every N from 1 to 42 compiles with no scratch and no
// spilled VGPR, 43 is the first that spills; 41 reloads a spilled SGPR inside
// the walk loop, so the cap stays at 40, where the loop is clean.  At every
// N <= 40 the walk loop (one odd + one even Gray step) holds exactly
// 2(88n - 28) fp64 VALU instructions, no scratch instruction and no readlane;
// the SGPR spills (4..357, to VGPR lanes) are in the chunk start only.  From
// N = 25 part of x lives in AGPRs and moves every step (x no longer fits 256
// VGPRs beside the four partial products): 1002 moves beside 6984 fp64
// instructions at N = 40, measured as 7.4 % over the instruction ratio against
// walk_cplx.
// Waves per SIMD: up to N = 23 the kernel needs at most 255 VGPRs and no AGPR
// whether it is asked for 2 waves or for 1, so the hardware runs 2 waves
// either way (the request states it; the code is the same but for one VGPR at
// N = 23).  At N = 24 the 2-wave request spills 24 VGPRs to 36 bytes of
// scratch (25: 33, 26: 57; walk_cplxdd_resources_two_waves_asked_to_26.log),
// so 24..40 take 1 wave: there is no N at which both settings compile clean
// and differ, and nothing to scan on the GPU.
#include "cxdd.hpp"
#include "kernels.hpp"
#include "walk_common.hpp"

namespace sup {

#ifndef SUP_CPLXDD_TWO_WAVES_MAX
#define SUP_CPLXDD_TWO_WAVES_MAX 23  // largest N asked for 2 waves per SIMD (256 VGPRs)
#endif

// Rows [LO, HI) of one plane: HI - LO <= 32 doubles = 64 SGPRs of column data.
// SEL (the chunk start's lane bits): a lane whose bit is clear adds 0.0.  The
// column value is pinned in SGPRs before the select, as cx_add_re pins it
// (walk_cplx.hip), so the load stays one unconditional scalar load.
template <int N, int LO, int HI, bool SEL>
__device__ __forceinline__ void cxdd_add_re(cxdd (&x)[N], cdbl* cre, bool on) {
#pragma unroll
  for (int j = LO; j < HI; ++j) {
    double c = cre[j];
    if constexpr (SEL) {
      asm volatile("" : "+s"(c));
      c = on ? c : 0.0;
    }
    x[j].re = dd_add_d(x[j].re, c);
  }
}
template <int N, int LO, int HI, bool SEL>
__device__ __forceinline__ void cxdd_add_im(cxdd (&x)[N], cdbl* cim, bool on) {
#pragma unroll
  for (int j = LO; j < HI; ++j) {
    double c = cim[j];
    if constexpr (SEL) {
      asm volatile("" : "+s"(c));
      c = on ? c : 0.0;
    }
    x[j].im = dd_add_d(x[j].im, c);
  }
}

// Full-column update (cxdd_add_d2 on every row), in cx_add_col's pieces: at
// most 32 rows of one plane (64 SGPRs of column data) between scheduling
// fences.
template <int N, bool SEL = false>
__device__ __forceinline__ void cxdd_add_col(cxdd (&x)[N], cdbl* cre, cdbl* cim, bool on = true) {
  if constexpr (N <= 16) {
    cxdd_add_re<N, 0, N, SEL>(x, cre, on);
    cxdd_add_im<N, 0, N, SEL>(x, cim, on);
  } else if constexpr (N <= 32) {
    cxdd_add_re<N, 0, N, SEL>(x, cre, on);
    __builtin_amdgcn_sched_barrier(0);
    cxdd_add_im<N, 0, N, SEL>(x, cim, on);
  } else {
    cxdd_add_re<N, 0, 32, SEL>(x, cre, on);
    __builtin_amdgcn_sched_barrier(0);
    cxdd_add_im<N, 0, 32, SEL>(x, cim, on);
    __builtin_amdgcn_sched_barrier(0);
    cxdd_add_re<N, 32, N, SEL>(x, cre, on);
    __builtin_amdgcn_sched_barrier(0);
    cxdd_add_im<N, 32, N, SEL>(x, cim, on);
  }
}

// Four strided partial products, combined as (p0 p1)(p2 p3) — cx_prod4's shape.
template <int N>
__device__ __forceinline__ cxdd cxdd_prod4(const cxdd (&x)[N]) {
  const cxdd one{dd{1.0, 0.0}, dd{0.0, 0.0}};
  cxdd p0 = x[0];
  cxdd p1 = N > 1 ? x[1 < N ? 1 : 0] : one;
  cxdd p2 = N > 2 ? x[2 < N ? 2 : 0] : one;
  cxdd p3 = N > 3 ? x[3 < N ? 3 : 0] : one;
#pragma unroll
  for (int j = 4; j < N; j += 4) {
    p0 = cxdd_mul(p0, x[j]);
    if (j + 1 < N) p1 = cxdd_mul(p1, x[j + 1 < N ? j + 1 : 0]);
    if (j + 2 < N) p2 = cxdd_mul(p2, x[j + 2 < N ? j + 2 : 0]);
    if (j + 3 < N) p3 = cxdd_mul(p3, x[j + 3 < N ? j + 3 : 0]);
  }
  if (N == 1) return p0;
  if (N == 2) return cxdd_mul(p0, p1);
  if (N == 3) return cxdd_mul(cxdd_mul(p0, p1), p2);
  return cxdd_mul(cxdd_mul(p0, p1), cxdd_mul(p2, p3));
}

// 64-lane pairwise dd sum (walk_dd.hip's: ascending xor offsets; dd_add is
// commutative, so every lane ends with the same value), on each part.
__device__ __forceinline__ dd dd_wave_sum(dd v) {
#pragma unroll
  for (int off = 1; off <= 32; off <<= 1) {
    const dd o{__shfl_xor(v.hi, off, 64), __shfl_xor(v.lo, off, 64)};
    v = dd_add(v, o);
  }
  return v;
}
__device__ __forceinline__ cxdd cxdd_wave_sum(cxdd v) { return cxdd{dd_wave_sum(v.re), dd_wave_sum(v.im)}; }

template <int N>
__global__ __launch_bounds__(kBlock)
    __attribute__((amdgpu_waves_per_eu(N <= SUP_CPLXDD_TWO_WAVES_MAX ? 2 : 1))) void walk_cplxdd(WalkParams p) {
  constexpr int NP = pad8(N);
  constexpr uint32_t kImOff = 2u * (uint32_t)(N > 1 ? N - 1 : 1) * NP * 8u;  // bytes from the Re to the Im plane
  const cxdd zero{dd{0.0, 0.0}, dd{0.0, 0.0}};
  const uint32_t lane = threadIdx.x & 63u;
  const bool lane_valid = lane < (1u << p.L);
  const uint32_t lane_par = __builtin_popcount(lane) & 1u;
  const uint32_t T = 1u << p.m;
  const uint32_t offL = 2u * (uint32_t)p.L * NP * 8u;  // engine bit L = walk bit 0

  // x += the column at byte offset `off` of both planes
  auto step = [&](cxdd(&x)[N], uint32_t off) {
    cxdd_add_col<N>(x, opaque_c(p.cols, off), opaque_c(p.cols, kImOff + off));
  };

  for (uint32_t g = next_chunk(p.counter); (uint64_t)g * p.group < p.chunk_count; g = next_chunk(p.counter)) {
    cxdd keep = zero;  // lane j keeps the partial of chunk g*p.group + j
    for (uint32_t j = 0; j < (uint32_t)p.group; ++j) {
      const uint64_t a = (uint64_t)g * p.group + j;
      if (a >= p.chunk_count) break;
      const uint64_t ga = p.chunk_begin + a;
      // chunk start (chunk_start's order: x0, high bits ascending, lane bits ascending)
      cxdd x[N];
      {
        cdbl* x0 = opaque_c(p.x0, 0);
#pragma unroll
        for (int r = 0; r < N; ++r) x[r] = cxdd{dd{x0[r], x0[NP + r]}, dd{x0[2 * NP + r], x0[3 * NP + r]}};
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
          cxdd_add_col<N, true>(x, cre, cim, (lane >> e) & 1u);  // x + (on ? column : 0.0)
        }
      }
      cxdd acc = cxdd_prod4<N>(x);  // t = 0
      uint32_t t = 1;
      // odd t flips walk bit 0 (term sign -), even t walk bit ctz(t) (sign +)
      for (; t + 1 < T; t += 2) {
        step(x, offL + ((t >> 1) & 1u) * NP * 8u);
        acc = cxdd_add(acc, cxdd_neg(cxdd_prod4<N>(x)));
        const uint32_t u = t + 1;
        const uint32_t k = (uint32_t)__builtin_ctz(u);
        const uint32_t neg = (u >> (k + 1)) & 1u;
        step(x, offL + (2u * k + neg) * NP * 8u);
        acc = cxdd_add(acc, cxdd_prod4<N>(x));
      }
      if (t < T) {
        step(x, offL + ((t >> 1) & 1u) * NP * 8u);
        acc = cxdd_add(acc, cxdd_neg(cxdd_prod4<N>(x)));
      }
      if (((uint32_t)ga ^ lane_par) & 1u) acc = cxdd_neg(acc);
      const cxdd part = cxdd_wave_sum(lane_valid ? acc : zero);
      if (lane == j) keep = part;
    }
    const uint64_t a = (uint64_t)g * p.group + lane;
    if (lane < (uint32_t)p.group && a < p.chunk_count) {
      p.chunk_out[4 * a] = keep.re.hi;
      p.chunk_out[4 * a + 1] = keep.re.lo;
      p.chunk_out[4 * a + 2] = keep.im.hi;
      p.chunk_out[4 * a + 3] = keep.im.lo;
    }
  }
}

template <int N, int HI>
static hipError_t launch_rec(int n, const WalkParams& p, int grid, hipStream_t s) {
  if (n == N) {
    hipLaunchKernelGGL(walk_cplxdd<N>, dim3(grid), dim3(kBlock), 0, s, p);
    return hipGetLastError();
  }
  if constexpr (N < HI) return launch_rec<N + 1, HI>(n, p, grid, s);
  return hipErrorInvalidValue;
}

template <int N, int HI>
static hipError_t occ_rec(int n, int* blocks_per_cu) {
  if (n == N) return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, walk_cplxdd<N>, kBlock, 0);
  if constexpr (N < HI) return occ_rec<N + 1, HI>(n, blocks_per_cu);
  return hipErrorInvalidValue;
}

#define SUP_CAT2(a, b) a##b
#define SUP_CAT(a, b) SUP_CAT2(a, b)

hipError_t SUP_CAT(launch_cplxdd_, SUP_N_LO)(int n, const WalkParams& p, int grid, hipStream_t s) {
  return launch_rec<SUP_N_LO, SUP_N_HI>(n, p, grid, s);
}
hipError_t SUP_CAT(occupancy_cplxdd_, SUP_N_LO)(int n, int* blocks_per_cu) {
  return occ_rec<SUP_N_LO, SUP_N_HI>(n, blocks_per_cu);
}

}  // namespace sup
