// walk_cplxf.hip — the collision-aware complex fp64 walk for gfx950
// (sup_perman_complex_fock; cplx_fock.cpp).
//
// A matrix gathered from U by index lists that repeat has K < n distinct
// columns b_0..b_K-1 with multiplicities t_k.  Subsets that take the same
// number of copies from every group give the same term, so with one copy of
// the rarest column held (t'_k = t_k - 1 there, t_k elsewhere)
//   per(A) = 2 sum_{0 <= v_k <= t'_k} (-1)^(sum v) prod_k C(t'_k, v_k) prod_j x_j(v)
//   x_j(v) = x_j(0) - sum_k v_k b_k[j],   x_j(0) = 1/2 sum_k t_k b_k[j]
// has T = prod (t'_k + 1) terms instead of 2^(n-1).  The digits v_k split into
// walk digits (the lowest; every lane walks them from 0 in the same reflected
// mixed-radix Gray order, so the column a step adds and the weight of the
// state it reaches are wave-uniform: the step program, read by scalar loads)
// and high digits: the mixed-radix number h = 64 chunk + lane, decoded per
// lane at the chunk start, where x = x(0) - sum v_k b_k is formed with a
// lane-valued multiplier on a scalar-loaded column.  Per step and lane:
//   x    += the step's signed column      2n adds, the column as SGPR operands
//   term  = prod_j x_j                    cx_mul's order, (p0 p1)(p2 p3)
//   acc  += w * term                      2 muls, 2 adds (no fma)
// 6n fp64 VALU ops.  The lane's high-digit weight multiplies acc once at the
// end; lanes with h >= H contribute zero; the 64-lane butterfly gives one
// (re, im) partial per wave-chunk.  cplx_fock.cpp's host twin runs the same
// operations in the same order.
//
// One queue holds the wave-chunks of all matrices of a slab: FockChunk a names
// the matrix and its chunk, FockMat the matrix's tables (cplx_fock.hpp).
// Both are wave-uniform and arrive by scalar loads.  The helpers restate
// walk_cplx.hip's (that file and walk_cplxb.hip stay as they are: their
// generated code is pinned by the resource logs).  Waves per SIMD asked for as
// walk_cplx at each N but 53..55 (below).  Resource report and walk-loop census per N:
// profiles/complex_fock/walk_cplx_fock_resources.log.
#include "cplx_fock.hpp"
#include "cx.hpp"
#include "kernels.hpp"
#include "walk_common.hpp"

namespace sup {

// Largest N asked for 2 waves per SIMD (256 VGPRs).  walk_cplx.hip's limit is
// 55; this kernel also holds the step program's entry and the weights, and at
// N = 53 and 55 the 2-wave request spilled 2 and 4 VGPRs to scratch in the
// chunk start, so 53..55 take 1 wave as 56..64 do.
#ifndef SUP_CPLXF_TWO_WAVES_MAX
#define SUP_CPLXF_TWO_WAVES_MAX 52
#endif

// Rows [LO, HI) of one plane added to x (HI - LO <= 32 doubles = 64 SGPRs).
template <int N, int LO, int HI>
__device__ __forceinline__ void cxf_add_re(cx (&x)[N], cdbl* cre) {
#pragma unroll
  for (int j = LO; j < HI; ++j) x[j].re = x[j].re + cre[j];
}
template <int N, int LO, int HI>
__device__ __forceinline__ void cxf_add_im(cx (&x)[N], cdbl* cim) {
#pragma unroll
  for (int j = LO; j < HI; ++j) x[j].im = x[j].im + cim[j];
}
// x = fma(nv, column, x) on rows [LO, HI): nv is the lane's -v_k.  The column
// value is pinned in SGPRs first, so its load stays one unconditional scalar
// load (walk_cplx.hip cx_add_re).
template <int N, int LO, int HI>
__device__ __forceinline__ void cxf_mad_re(cx (&x)[N], cdbl* cre, double nv) {
#pragma unroll
  for (int j = LO; j < HI; ++j) {
    double c = cre[j];
    asm volatile("" : "+s"(c));
    x[j].re = __builtin_fma(nv, c, x[j].re);
  }
}
template <int N, int LO, int HI>
__device__ __forceinline__ void cxf_mad_im(cx (&x)[N], cdbl* cim, double nv) {
#pragma unroll
  for (int j = LO; j < HI; ++j) {
    double c = cim[j];
    asm volatile("" : "+s"(c));
    x[j].im = __builtin_fma(nv, c, x[j].im);
  }
}

// Full-column update in walk_cplx.hip's pieces: up to 16 rows both planes in
// one piece, up to 32 rows a piece per plane, above that two passes of two
// pieces, a scheduling fence between pieces (at most 64 SGPRs of column data).
template <int N>
__device__ __forceinline__ void cxf_add_col(cx (&x)[N], cdbl* cre, cdbl* cim) {
  if constexpr (N <= 16) {
    cxf_add_re<N, 0, N>(x, cre);
    cxf_add_im<N, 0, N>(x, cim);
  } else if constexpr (N <= 32) {
    cxf_add_re<N, 0, N>(x, cre);
    __builtin_amdgcn_sched_barrier(0);
    cxf_add_im<N, 0, N>(x, cim);
  } else {
    cxf_add_re<N, 0, 32>(x, cre);
    __builtin_amdgcn_sched_barrier(0);
    cxf_add_im<N, 0, 32>(x, cim);
    __builtin_amdgcn_sched_barrier(0);
    cxf_add_re<N, 32, N>(x, cre);
    __builtin_amdgcn_sched_barrier(0);
    cxf_add_im<N, 32, N>(x, cim);
  }
}
template <int N>
__device__ __forceinline__ void cxf_mad_col(cx (&x)[N], cdbl* cre, cdbl* cim, double nv) {
  if constexpr (N <= 16) {
    cxf_mad_re<N, 0, N>(x, cre, nv);
    cxf_mad_im<N, 0, N>(x, cim, nv);
  } else if constexpr (N <= 32) {
    cxf_mad_re<N, 0, N>(x, cre, nv);
    __builtin_amdgcn_sched_barrier(0);
    cxf_mad_im<N, 0, N>(x, cim, nv);
  } else {
    cxf_mad_re<N, 0, 32>(x, cre, nv);
    __builtin_amdgcn_sched_barrier(0);
    cxf_mad_im<N, 0, 32>(x, cim, nv);
    __builtin_amdgcn_sched_barrier(0);
    cxf_mad_re<N, 32, N>(x, cre, nv);
    __builtin_amdgcn_sched_barrier(0);
    cxf_mad_im<N, 32, N>(x, cim, nv);
  }
}

// Four strided partial products, combined as (p0 p1)(p2 p3) (walk_cplx.hip cx_prod4).
template <int N>
__device__ __forceinline__ cx cxf_prod4(const cx (&x)[N]) {
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

// 64-lane pairwise sum of re and im (ascending xor offsets).
__device__ __forceinline__ cx cxf_wave_sum(cx v) {
#pragma unroll
  for (int off = 1; off <= 32; off <<= 1) {
    const cx o{__shfl_xor(v.re, off, 64), __shfl_xor(v.im, off, 64)};
    v = cx_add(v, o);
  }
  return v;
}

// A wave-uniform descriptor read by scalar loads: the base goes through the
// asm as opaque_c's does, the (uniform) index is added after it.
template <class T>
__device__ __forceinline__ const __attribute__((address_space(4))) T* cxf_uniform(const T* base, uint64_t index) {
  uint64_t a = (uint64_t)base;
  asm volatile("" : "+s"(a));
  return (const __attribute__((address_space(4))) T*)(a + index * sizeof(T));
}

template <int N>
__global__ __launch_bounds__(kBlock)
    __attribute__((amdgpu_waves_per_eu(N <= SUP_CPLXF_TWO_WAVES_MAX ? 2 : 1))) void walk_cplx_fock(FockParams p) {
  constexpr int NP = pad8(N);
  const uint32_t lane = threadIdx.x & 63u;

  for (uint32_t g = next_chunk(p.counter); (uint64_t)g * p.group < p.chunk_count; g = next_chunk(p.counter)) {
    cx keep{0.0, 0.0};  // lane j keeps the partial of chunk g*p.group + j
    for (uint32_t j = 0; j < p.group; ++j) {
      const uint64_t a = (uint64_t)g * p.group + j;
      if (a >= p.chunk_count) break;
      const uint32_t mat = cxf_uniform(p.chunks, a)->mat;
      const uint32_t local = cxf_uniform(p.chunks, a)->local;
      const auto* M = cxf_uniform(p.mats, mat);
      const double* cols = p.tabs + M->tab;
      const uint32_t im_off = M->im_off;
      const uint32_t Tw = M->Tw;
      // chunk start: x(0), then the high digits of h, lowest first
      const uint32_t h = 64u * local + lane;
      const bool lane_valid = h < M->H;
      cx x[N];
      double hw = 1.0;
      {
        cdbl* x0 = opaque_c(p.x0s + M->x0, 0);
#pragma unroll
        for (int r = 0; r < N; ++r) x[r] = cx{x0[r], x0[NP + r]};
        uint32_t rem = lane_valid ? h : 0u;
        const uint32_t ndig = M->ndig;
        const uint32_t dig0 = M->dig;
        for (uint32_t d = 0; d < ndig; ++d) {
          const auto* D = cxf_uniform(p.dig, (uint64_t)dig0 + d);
          const uint32_t radix = D->radix, col_off = D->col_off;
          const uint32_t q = rem / radix;
          const uint32_t v = rem - q * radix;
          rem = q;
          hw = hw * p.wts[D->wt_off + v];
          cxf_mad_col<N>(x, opaque_c(cols, col_off), opaque_c(cols, im_off + col_off), -(double)v);
        }
      }
      cx acc = cxf_prod4<N>(x);  // t = 0, weight +1
      if (Tw > 1) {
        const FockStep* prog = p.prog + M->prog;
        uint32_t off = cxf_uniform(prog, 1)->off;
        double w = cxf_uniform(prog, 1)->w;
        for (uint32_t t = 1; t < Tw; ++t) {
          // the next entry is asked for before this step's arithmetic (the
          // program ends with a padding entry)
          const uint32_t off_n = cxf_uniform(prog, (uint64_t)t + 1)->off;
          const double w_n = cxf_uniform(prog, (uint64_t)t + 1)->w;
          cxf_add_col<N>(x, opaque_c(cols, off), opaque_c(cols, im_off + off));
          const cx term = cxf_prod4<N>(x);
          const double mr = w * term.re, mi = w * term.im;
          acc = cx{acc.re + mr, acc.im + mi};
          off = off_n;
          w = w_n;
        }
      }
      acc = cx{acc.re * hw, acc.im * hw};
      const cx part = cxf_wave_sum(lane_valid ? acc : cx{0.0, 0.0});
      if (lane == j) keep = part;
    }
    const uint64_t a = (uint64_t)g * p.group + lane;
    if (lane < p.group && a < p.chunk_count) {
      p.chunk_out[2 * a] = keep.re;
      p.chunk_out[2 * a + 1] = keep.im;
    }
  }
}

template <int N, int HI>
static hipError_t launch_rec(int n, const FockParams& p, int grid, hipStream_t s) {
  if (n == N) {
    hipLaunchKernelGGL(walk_cplx_fock<N>, dim3(grid), dim3(kBlock), 0, s, p);
    return hipGetLastError();
  }
  if constexpr (N < HI) return launch_rec<N + 1, HI>(n, p, grid, s);
  return hipErrorInvalidValue;
}

template <int N, int HI>
static hipError_t occ_rec(int n, int* blocks_per_cu) {
  if (n == N) return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, walk_cplx_fock<N>, kBlock, 0);
  if constexpr (N < HI) return occ_rec<N + 1, HI>(n, blocks_per_cu);
  return hipErrorInvalidValue;
}

#define SUP_CAT2(a, b) a##b
#define SUP_CAT(a, b) SUP_CAT2(a, b)

hipError_t SUP_CAT(launch_cplxf_, SUP_N_LO)(int n, const FockParams& p, int grid, hipStream_t s) {
  return launch_rec<SUP_N_LO, SUP_N_HI>(n, p, grid, s);
}
hipError_t SUP_CAT(occupancy_cplxf_, SUP_N_LO)(int n, int* blocks_per_cu) {
  return occ_rec<SUP_N_LO, SUP_N_HI>(n, blocks_per_cu);
}

}  // namespace sup
