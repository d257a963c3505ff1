// walk_cplxfm.hip — the collision-aware one-walk permanent minors for gfx950
// (sup_perman_complex_fock_minors; cplx_fock_minors.cpp): the N
// minors (B without row j) of N x (N-1) matrices B gathered from U, N <= 32,
// with the repeated columns of B collapsed.
//
// §8c's sum over the column multiplicities (walk_cplxf.hip) and §8d's products
// "all rows but j" (walk_cplxm.hip) fit together because x_i(v) depends on row
// i only: with the distinct columns b_0..b_K-1 over all N rows, multiplicities
// t_k (sum N - 1), one copy of the rarest held,
//   per(minor j) = 2 sum_{0 <= v_k <= t'_k} (-1)^(sum v) prod_k C(t'_k, v_k) prod_{i != j} x_i(v)
//   x_i(v) = x_i(0) - sum_k v_k b_k[i],   x_i(0) = 1/2 sum_k t_k b_k[i]
// one walk of T = prod (t'_k + 1) states instead of 2^(N-2) serves all N minors.
//
// Structure, from walk_cplx_fock: one queue of FockChunks over a slab, the
// wave-uniform descriptors by scalar loads through an opaque base, the chunk
// start with the lane's high digits (h = 64 chunk + lane) and the pinned-SGPR
// multiply-add of a scalar-loaded column, the step program fetched one entry
// ahead.  Arithmetic and output, from walk_cplx_minors: x, acc and the
// prefixes per lane (cxfm.hpp: 16 N - 20 fp64 operations per walked step),
// the lane's high-digit weight once at the end, zeroed invalid lanes, the
// 64-lane butterfly once per output, lane r keeps output r's partial and lanes
// < N write.  The partial of output j of chunk `local` of matrix M goes to
//   p.chunk_out[2 (N M.chunk0 + j M.chunks + local)]
// so each output's partials are contiguous and fock_fold folds them
// (cplx_fock_minors_fold).  The helpers restate the two parents' (those files
// and their pinned resource logs stay as they are).  Resource report and
// walk-loop census per N: profiles/complex_fock_minors/walk_cplx_fock_minors_resources.log.
#include "cplx_fock.hpp"
#include "cxfm.hpp"
#include "kernels.hpp"
#include "walk_common.hpp"

namespace sup {

// State per lane: x, acc and the stored prefixes, 12 N VGPRs, plus the step's
// weight and the lane's high-digit weight.  Two waves per SIMD (256 VGPRs
// each) up to this N; above, one wave with the overflow in AGPRs (no scratch
// at any N; the resources log has the moves).
#ifndef SUP_CPLXFM_TWO_WAVES_MAX
#define SUP_CPLXFM_TWO_WAVES_MAX 21
#endif

template <int N>
__device__ __forceinline__ void cxfm_add_re(cx (&x)[N], cdbl* cre) {
#pragma unroll
  for (int j = 0; j < N; ++j) x[j].re = x[j].re + cre[j];
}
template <int N>
__device__ __forceinline__ void cxfm_add_im(cx (&x)[N], cdbl* cim) {
#pragma unroll
  for (int j = 0; j < N; ++j) x[j].im = x[j].im + cim[j];
}
// x = fma(nv, column, x): nv is the lane's -v_k.  The column value is pinned
// in SGPRs first, so its load stays one unconditional scalar load
// (walk_cplxf.hip cxf_mad_re).
template <int N>
__device__ __forceinline__ void cxfm_mad_re(cx (&x)[N], cdbl* cre, double nv) {
#pragma unroll
  for (int j = 0; j < N; ++j) {
    double c = cre[j];
    asm volatile("" : "+s"(c));
    x[j].re = __builtin_fma(nv, c, x[j].re);
  }
}
template <int N>
__device__ __forceinline__ void cxfm_mad_im(cx (&x)[N], cdbl* cim, double nv) {
#pragma unroll
  for (int j = 0; j < N; ++j) {
    double c = cim[j];
    asm volatile("" : "+s"(c));
    x[j].im = __builtin_fma(nv, c, x[j].im);
  }
}

// Full-column update: up to 16 rows both planes in one piece, up to 32 rows a
// piece per plane with a scheduling fence between them (at most 64 SGPRs of
// column data).
template <int N>
__device__ __forceinline__ void cxfm_add_col(cx (&x)[N], cdbl* cre, cdbl* cim) {
  static_assert(N <= 32, "the minors walk is instantiated for N <= 32");
  cxfm_add_re<N>(x, cre);
  if constexpr (N > 16) __builtin_amdgcn_sched_barrier(0);
  cxfm_add_im<N>(x, cim);
}
template <int N>
__device__ __forceinline__ void cxfm_mad_col(cx (&x)[N], cdbl* cre, cdbl* cim, double nv) {
  static_assert(N <= 32, "the minors walk is instantiated for N <= 32");
  cxfm_mad_re<N>(x, cre, nv);
  if constexpr (N > 16) __builtin_amdgcn_sched_barrier(0);
  cxfm_mad_im<N>(x, cim, nv);
}

// 64-lane pairwise sum of re and im (ascending xor offsets).
__device__ __forceinline__ cx cxfm_wave_sum(cx v) {
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
__device__ __forceinline__ const __attribute__((address_space(4))) T* cxfm_uniform(const T* base, uint64_t index) {
  uint64_t a = (uint64_t)base;
  asm volatile("" : "+s"(a));
  return (const __attribute__((address_space(4))) T*)(a + index * sizeof(T));
}

template <int N>
__global__ __launch_bounds__(kBlock)
    __attribute__((amdgpu_waves_per_eu(N <= SUP_CPLXFM_TWO_WAVES_MAX ? 2 : 1))) void walk_cplx_fock_minors(FockParams p) {
  constexpr int NP = pad8(N);
  const uint32_t lane = threadIdx.x & 63u;

  for (uint32_t g = next_chunk(p.counter); (uint64_t)g * p.group < p.chunk_count; g = next_chunk(p.counter)) {
    for (uint32_t j = 0; j < p.group; ++j) {
      const uint64_t a = (uint64_t)g * p.group + j;
      if (a >= p.chunk_count) break;
      const uint32_t mat = cxfm_uniform(p.chunks, a)->mat;
      const uint32_t local = cxfm_uniform(p.chunks, a)->local;
      const auto* M = cxfm_uniform(p.mats, mat);
      const double* cols = p.tabs + M->tab;
      const uint32_t im_off = M->im_off;
      const uint32_t Tw = M->Tw;
      // chunk start: x(0), then the high digits of h, lowest first
      const uint32_t h = 64u * local + lane;
      const bool lane_valid = h < M->H;
      cx x[N];
      {
        cdbl* x0 = opaque_c(p.x0s + M->x0, 0);
#pragma unroll
        for (int r = 0; r < N; ++r) x[r] = cx{x0[r], x0[NP + r]};
        uint32_t rem = lane_valid ? h : 0u;
        const uint32_t ndig = M->ndig;
        const uint32_t dig0 = M->dig;
        for (uint32_t d = 0; d < ndig; ++d) {
          const auto* D = cxfm_uniform(p.dig, (uint64_t)dig0 + d);
          const uint32_t radix = D->radix, col_off = D->col_off;
          const uint32_t q = rem / radix;
          const uint32_t v = rem - q * radix;
          rem = q;
          cxfm_mad_col<N>(x, opaque_c(cols, col_off), opaque_c(cols, im_off + col_off), -(double)v);
        }
      }
      cx acc[N];
#pragma unroll
      for (int r = 0; r < N; ++r) acc[r] = cx{0.0, 0.0};
      cxm_accumulate<N, false>(x, acc);  // t = 0, weight +1
      if (Tw > 1) {
        const FockStep* prog = p.prog + M->prog;
        uint32_t off = cxfm_uniform(prog, 1)->off;
        double w = cxfm_uniform(prog, 1)->w;
        for (uint32_t t = 1; t < Tw; ++t) {
          // the next entry is asked for before this step's arithmetic (the
          // program ends with a padding entry)
          const uint32_t off_n = cxfm_uniform(prog, (uint64_t)t + 1)->off;
          const double w_n = cxfm_uniform(prog, (uint64_t)t + 1)->w;
          cxfm_add_col<N>(x, opaque_c(cols, off), opaque_c(cols, im_off + off));
          cxfm_accumulate<N>(x, w, acc);
          off = off_n;
          w = w_n;
        }
      }
      // the lane's high-digit weight, lowest digit first: decoded again here
      // and not at the chunk start, so it holds no registers through the walk
      double hw = 1.0;
      {
        uint32_t rem = lane_valid ? h : 0u;
        const uint32_t ndig = M->ndig;
        const uint32_t dig0 = M->dig;
        for (uint32_t d = 0; d < ndig; ++d) {
          const auto* D = cxfm_uniform(p.dig, (uint64_t)dig0 + d);
          const uint32_t radix = D->radix;
          const uint32_t q = rem / radix;
          const uint32_t v = rem - q * radix;
          rem = q;
          hw = hw * p.wts[D->wt_off + v];
        }
      }
      cx keep{0.0, 0.0};  // lane r keeps the partial of output r
#pragma unroll
      for (int r = 0; r < N; ++r) {
        const cx v{acc[r].re * hw, acc[r].im * hw};
        const cx part = cxfm_wave_sum(lane_valid ? v : cx{0.0, 0.0});
        if (lane == (uint32_t)r) keep = part;
      }
      if (lane < (uint32_t)N) {
        const uint64_t o = (uint64_t)N * M->chunk0 + (uint64_t)lane * M->chunks + local;
        p.chunk_out[2 * o] = keep.re;
        p.chunk_out[2 * o + 1] = keep.im;
      }
    }
  }
}

template <int N, int HI>
static hipError_t launch_rec(int n, const FockParams& p, int grid, hipStream_t s) {
  if (n == N) {
    hipLaunchKernelGGL(walk_cplx_fock_minors<N>, dim3(grid), dim3(kBlock), 0, s, p);
    return hipGetLastError();
  }
  if constexpr (N < HI) return launch_rec<N + 1, HI>(n, p, grid, s);
  return hipErrorInvalidValue;
}

template <int N, int HI>
static hipError_t occ_rec(int n, int* blocks_per_cu) {
  if (n == N) return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, walk_cplx_fock_minors<N>, kBlock, 0);
  if constexpr (N < HI) return occ_rec<N + 1, HI>(n, blocks_per_cu);
  return hipErrorInvalidValue;
}

// the 1_16 range starts at N = 2: one row has no walk (its minor is empty)
constexpr int kLo = SUP_N_LO < 2 ? 2 : SUP_N_LO;

#define SUP_CAT2(a, b) a##b
#define SUP_CAT(a, b) SUP_CAT2(a, b)

hipError_t SUP_CAT(launch_cplxfm_, SUP_N_LO)(int n, const FockParams& p, int grid, hipStream_t s) {
  return launch_rec<kLo, SUP_N_HI>(n, p, grid, s);
}
hipError_t SUP_CAT(occupancy_cplxfm_, SUP_N_LO)(int n, int* blocks_per_cu) {
  return occ_rec<kLo, SUP_N_HI>(n, blocks_per_cu);
}

}  // namespace sup
