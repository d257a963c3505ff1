// walk_cplxb.hip — the batched complex fp64 walk for gfx950: the wave-chunks
// of K matrices of one order n <= 32 in one queue and one launch
// (sup_perman_complex_batch, sup_perman_complex_submatrices; cplx.cpp).
//
// One matrix of order n < 26 has fewer than the 2^13 wave-chunks that fill an
// MI355X (one wave at n <= 13, 128 at n = 20), and boson-sampling simulators
// evaluate 10^4..10^7 such permanents per run.  Here global chunk a of the
// queue is chunk a & (2^h - 1) of matrix a >> h, walked exactly as
// walk_cplx<N> (walk_cplx.hip) walks it — the same enumeration, lane layout,
// cx.hpp operations and order — with that matrix's tables:
//   columns  p.cols + (a >> h) * kTab   (Re plane, then Im plane, as walk_cplx)
//   start    p.x0   + (a >> h) * 2 NP   (re block, then im block)
// written on the device by cplx_batch_prepare (cplx_batch.hip).  The chunk's
// partial goes to p.chunk_out[2a], [2a + 1]; cplx_batch_fold folds each
// matrix's 2^h partials.  So result k has the bits of walk_cplx on matrix k
// alone.
//
// The matrix base is wave-uniform (the ticket comes from readfirstlane, the
// group index is a loop counter); it goes through opaque_c like walk_cplx's
// one base, so the column data still arrives by scalar loads as SGPR operands
// in pieces of at most 64 SGPRs.  The helpers below restate walk_cplx.hip's
// for N <= 32 (that file stays as it is: its generated code is pinned by
// profiles/complex/walk_cplx_resources.log).  Instantiated for N = 1..32 only:
// from n = 26 one matrix has 2^13 chunks, and the batch entries run n > 32
// through the single-matrix walk.  Resource report and walk-loop census per N:
// profiles/complex_batch/walk_cplx_batch_resources.log.
#include "cx.hpp"
#include "kernels.hpp"
#include "walk_common.hpp"

namespace sup {

// Rows [0, N) of one plane: N <= 32 doubles = 64 SGPRs of column data.  SEL
// (the chunk start's lane bits): a lane whose bit is clear adds 0.0; the
// column value is pinned in SGPRs before the select, so the load stays one
// unconditional scalar load (walk_cplx.hip cx_add_re).
template <int N, bool SEL>
__device__ __forceinline__ void cxb_add_re(cx (&x)[N], cdbl* cre, bool on) {
#pragma unroll
  for (int j = 0; j < N; ++j) {
    double c = cre[j];
    if constexpr (SEL) {
      asm volatile("" : "+s"(c));
      c = on ? c : 0.0;
    }
    x[j].re = x[j].re + c;
  }
}
template <int N, bool SEL>
__device__ __forceinline__ void cxb_add_im(cx (&x)[N], cdbl* cim, bool on) {
#pragma unroll
  for (int j = 0; j < N; ++j) {
    double c = cim[j];
    if constexpr (SEL) {
      asm volatile("" : "+s"(c));
      c = on ? c : 0.0;
    }
    x[j].im = x[j].im + c;
  }
}

// Full-column update: up to 16 rows both planes in one piece, up to 32 rows a
// piece per plane with a scheduling fence between them (at most 64 SGPRs of
// column data live).
template <int N, bool SEL = false>
__device__ __forceinline__ void cxb_add_col(cx (&x)[N], cdbl* cre, cdbl* cim, bool on = true) {
  static_assert(N <= 32, "the batched walk is instantiated for N <= 32");
  cxb_add_re<N, SEL>(x, cre, on);
  if constexpr (N > 16) __builtin_amdgcn_sched_barrier(0);
  cxb_add_im<N, SEL>(x, cim, on);
}

// Four strided partial products, combined as (p0 p1)(p2 p3) (walk_cplx.hip cx_prod4).
template <int N>
__device__ __forceinline__ cx cxb_prod4(const cx (&x)[N]) {
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
__device__ __forceinline__ cx cxb_wave_sum(cx v) {
#pragma unroll
  for (int off = 1; off <= 32; off <<= 1) {
    const cx o{__shfl_xor(v.re, off, 64), __shfl_xor(v.im, off, 64)};
    v = cx_add(v, o);
  }
  return v;
}

// hbits: log2 of the wave-chunks per matrix (the layout's h); p.chunk_count =
// matrices << hbits, p.chunk_begin is not read (every matrix starts at its
// chunk 0).
template <int N>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(2))) void walk_cplx_batch(WalkParams p,
                                                                                                  int hbits) {
  constexpr int NP = pad8(N);
  constexpr uint32_t kImOff = 2u * (uint32_t)(N > 1 ? N - 1 : 1) * NP * 8u;  // bytes from the Re to the Im plane
  constexpr uint64_t kTab = 2ull * kImOff / 8u;                               // doubles of one matrix's table
  const uint32_t lane = threadIdx.x & 63u;
  const bool lane_valid = lane < (1u << p.L);
  const uint32_t lane_par = __builtin_popcount(lane) & 1u;
  const uint32_t T = 1u << p.m;
  const uint32_t offL = 2u * (uint32_t)p.L * NP * 8u;  // engine bit L = walk bit 0
  const uint64_t hmask = (1ull << hbits) - 1ull;

  for (uint32_t g = next_chunk(p.counter); (uint64_t)g * p.group < p.chunk_count; g = next_chunk(p.counter)) {
    cx keep{0.0, 0.0};  // lane j keeps the partial of chunk g*p.group + j
    for (uint32_t j = 0; j < (uint32_t)p.group; ++j) {
      const uint64_t a = (uint64_t)g * p.group + j;
      if (a >= p.chunk_count) break;
      const uint64_t mat = a >> hbits;  // wave-uniform
      const uint64_t ga = a & hmask;    // the chunk of that matrix
      const double* cols = p.cols + mat * kTab;
      // x += the column at byte offset `off` of both planes
      auto step = [&](cx(&x)[N], uint32_t off) {
        cxb_add_col<N>(x, opaque_c(cols, off), opaque_c(cols, kImOff + off));
      };
      // chunk start (chunk_start's order: x0, high bits ascending, lane bits ascending)
      cx x[N];
      {
        cdbl* x0 = opaque_c(p.x0 + mat * (uint64_t)(2 * NP), 0);
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
          cdbl* cre = opaque_c(cols, (2u * e) * NP * 8u);
          cdbl* cim = opaque_c(cols, kImOff + (2u * e) * NP * 8u);
          cxb_add_col<N, true>(x, cre, cim, (lane >> e) & 1u);  // x + (on ? column : 0.0)
        }
      }
      cx acc = cxb_prod4<N>(x);  // t = 0
      uint32_t t = 1;
      // odd t flips walk bit 0 (term sign -), even t walk bit ctz(t) (sign +)
      for (; t + 1 < T; t += 2) {
        step(x, offL + ((t >> 1) & 1u) * NP * 8u);
        acc = cx_sub(acc, cxb_prod4<N>(x));
        const uint32_t u = t + 1;
        const uint32_t k = (uint32_t)__builtin_ctz(u);
        const uint32_t neg = (u >> (k + 1)) & 1u;
        step(x, offL + (2u * k + neg) * NP * 8u);
        acc = cx_add(acc, cxb_prod4<N>(x));
      }
      if (t < T) {
        step(x, offL + ((t >> 1) & 1u) * NP * 8u);
        acc = cx_sub(acc, cxb_prod4<N>(x));
      }
      if (((uint32_t)ga ^ lane_par) & 1u) acc = cx_neg(acc);
      const cx part = cxb_wave_sum(lane_valid ? acc : cx{0.0, 0.0});
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
static hipError_t launch_rec(int n, const WalkParams& p, int hbits, int grid, hipStream_t s) {
  if (n == N) {
    hipLaunchKernelGGL(walk_cplx_batch<N>, dim3(grid), dim3(kBlock), 0, s, p, hbits);
    return hipGetLastError();
  }
  if constexpr (N < HI) return launch_rec<N + 1, HI>(n, p, hbits, grid, s);
  return hipErrorInvalidValue;
}

template <int N, int HI>
static hipError_t occ_rec(int n, int* blocks_per_cu) {
  if (n == N) return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, walk_cplx_batch<N>, kBlock, 0);
  if constexpr (N < HI) return occ_rec<N + 1, HI>(n, blocks_per_cu);
  return hipErrorInvalidValue;
}

#define SUP_CAT2(a, b) a##b
#define SUP_CAT(a, b) SUP_CAT2(a, b)

hipError_t SUP_CAT(launch_cplxb_, SUP_N_LO)(int n, const WalkParams& p, int hbits, int grid, hipStream_t s) {
  return launch_rec<SUP_N_LO, SUP_N_HI>(n, p, hbits, grid, s);
}
hipError_t SUP_CAT(occupancy_cplxb_, SUP_N_LO)(int n, int* blocks_per_cu) {
  return occ_rec<SUP_N_LO, SUP_N_HI>(n, blocks_per_cu);
}

}  // namespace sup
