// walk_cplxm.hip — the one-walk permanent minors for gfx950: the N minors
// (B without row j, j < N) of N x (N-1) complex matrices B, N <= 32, all from
// one Gray walk per matrix (sup_perman_complex_minors, cplx_minors.cpp).
//
// The boson sampler (boson.cpp) needs, per stage, the permanents of the N
// minors of one matrix; N calls of the plain walk repeat the same 2^(N-3) Gray
// states with the same row sums x.  Here every state forms the N products
// "all rows but j" from prefix and suffix products (cxm.hpp): 16 N - 24 fp64
// operations per step for N results instead of N (6 (N-1) - 2).
//
// Structure: walk_cplx_batch's (walk_cplxb.hip) throughout — one queue of
// K 2^h wave-chunks (global chunk a is chunk a & (2^h - 1) of matrix a >> h),
// the wave-uniform matrix base through opaque_c, column data as SGPR operands
// in pieces of at most 64 SGPRs, the pinned-SGPR lane-bit select, pair-unrolled
// steps with the sub/add sign pattern, the chunk sign, zeroed invalid lanes and
// the 64-lane butterfly (once per output).  Only the table geometry differs:
// the enumeration is the layout of order q = N - 1 (engine bit e = column e,
// column q - 1 held), so a matrix has q - 1 engine columns of N rows:
//   columns  p.cols + mat * kTab   Re plane, then Im plane, each 2 max(q-1, 1) x NP
//   start    p.x0   + mat * 2 NP   (re block, then im block)
// written by cplx_minors_prepare (cplx_minors.hip).  The partial of output j of
// queue entry a goes to p.chunk_out[2 ((mat N + j) ostride + a - (mat << h))]:
// each output's partials are contiguous, so cplx_batch_fold over K N "matrices"
// of order q folds them.  The helpers restate walk_cplxb.hip's (that file and
// its pinned resource log stay as they are).  Resource report and walk-loop
// census per N: profiles/complex_minors/walk_cplx_minors_resources.log.
#include "cxm.hpp"
#include "kernels.hpp"
#include "walk_common.hpp"

namespace sup {

// State per lane: x, acc and the stored prefixes, 12 N VGPRs (252 at N = 21).
// Two waves per SIMD (256 VGPRs each) up to this N; above, one wave with the
// overflow in AGPRs (no scratch at any N; the resources log has the moves).
#ifndef SUP_CPLXM_TWO_WAVES_MAX
#define SUP_CPLXM_TWO_WAVES_MAX 21
#endif

template <int N, bool SEL>
__device__ __forceinline__ void cxm_add_re(cx (&x)[N], cdbl* cre, bool on) {
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
__device__ __forceinline__ void cxm_add_im(cx (&x)[N], cdbl* cim, bool on) {
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
// piece per plane with a scheduling fence between them.
template <int N, bool SEL = false>
__device__ __forceinline__ void cxm_add_col(cx (&x)[N], cdbl* cre, cdbl* cim, bool on = true) {
  static_assert(N <= 32, "the minors walk is instantiated for N <= 32");
  cxm_add_re<N, SEL>(x, cre, on);
  if constexpr (N > 16) __builtin_amdgcn_sched_barrier(0);
  cxm_add_im<N, SEL>(x, cim, on);
}

// 64-lane pairwise sum of re and im (ascending xor offsets).
__device__ __forceinline__ cx cxm_wave_sum(cx v) {
#pragma unroll
  for (int off = 1; off <= 32; off <<= 1) {
    const cx o{__shfl_xor(v.re, off, 64), __shfl_xor(v.im, off, 64)};
    v = cx_add(v, o);
  }
  return v;
}

// hbits: log2 of the wave-chunks per matrix (the order-(N-1) layout's h).
// Queue entry a walks global chunk p.chunk_begin + a; ostride: partials per
// output in p.chunk_out.  The batch form has p.chunk_begin = 0 and ostride =
// 2^hbits; the range form one matrix, chunks [p.chunk_begin, + p.chunk_count)
// and ostride = p.chunk_count.
template <int N>
__global__ __launch_bounds__(kBlock)
    __attribute__((amdgpu_waves_per_eu(N <= SUP_CPLXM_TWO_WAVES_MAX ? 2 : 1))) void walk_cplx_minors(
        WalkParams p, int hbits, unsigned long long ostride) {
  constexpr int NP = pad8(N);
  constexpr uint32_t kImOff = 2u * (uint32_t)(N > 2 ? N - 2 : 1) * NP * 8u;  // bytes from the Re to the Im plane
  constexpr uint64_t kTab = 2ull * kImOff / 8u;                               // doubles of one matrix's table
  const uint32_t lane = threadIdx.x & 63u;
  const bool lane_valid = lane < (1u << p.L);
  const uint32_t lane_par = __builtin_popcount(lane) & 1u;
  const uint32_t T = 1u << p.m;
  const uint32_t offL = 2u * (uint32_t)p.L * NP * 8u;  // engine bit L = walk bit 0
  const uint64_t hmask = (1ull << hbits) - 1ull;

  for (uint32_t g = next_chunk(p.counter); (uint64_t)g * p.group < p.chunk_count; g = next_chunk(p.counter)) {
    for (uint32_t j = 0; j < (uint32_t)p.group; ++j) {
      const uint64_t a = (uint64_t)g * p.group + j;
      if (a >= p.chunk_count) break;
      const uint64_t mat = (p.chunk_begin + a) >> hbits;  // wave-uniform
      const uint64_t ga = (p.chunk_begin + a) & hmask;    // the chunk of that matrix
      const double* cols = p.cols + mat * kTab;
      // x += the column at byte offset `off` of both planes
      auto step = [&](cx(&x)[N], uint32_t off) {
        cxm_add_col<N>(x, opaque_c(cols, off), opaque_c(cols, kImOff + off));
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
          cxm_add_col<N, true>(x, cre, cim, (lane >> e) & 1u);  // x + (on ? column : 0.0)
        }
      }
      cx acc[N];
#pragma unroll
      for (int r = 0; r < N; ++r) acc[r] = cx{0.0, 0.0};
      cxm_accumulate<N, false>(x, acc);  // t = 0
      uint32_t t = 1;
      // odd t flips walk bit 0 (term sign -), even t walk bit ctz(t) (sign +)
      for (; t + 1 < T; t += 2) {
        step(x, offL + ((t >> 1) & 1u) * NP * 8u);
        cxm_accumulate<N, true>(x, acc);
        const uint32_t u = t + 1;
        const uint32_t k = (uint32_t)__builtin_ctz(u);
        const uint32_t neg = (u >> (k + 1)) & 1u;
        step(x, offL + (2u * k + neg) * NP * 8u);
        cxm_accumulate<N, false>(x, acc);
      }
      if (t < T) {
        step(x, offL + ((t >> 1) & 1u) * NP * 8u);
        cxm_accumulate<N, true>(x, acc);
      }
      const bool flip = (((uint32_t)ga ^ lane_par) & 1u) != 0;
      cx keep{0.0, 0.0};  // lane r keeps the partial of output r
#pragma unroll
      for (int r = 0; r < N; ++r) {
        cx v = flip ? cx_neg(acc[r]) : acc[r];
        const cx part = cxm_wave_sum(lane_valid ? v : cx{0.0, 0.0});
        if (lane == (uint32_t)r) keep = part;
      }
      if (lane < (uint32_t)N) {
        // batch form: a - (mat << hbits) = ga; range form: mat = 0, the index in the range
        const uint64_t o = (mat * (uint64_t)N + lane) * ostride + (a - (mat << hbits));
        p.chunk_out[2 * o] = keep.re;
        p.chunk_out[2 * o + 1] = keep.im;
      }
    }
  }
}

template <int N, int HI>
static hipError_t launch_rec(int n, const WalkParams& p, int hbits, unsigned long long ostride, int grid,
                             hipStream_t s) {
  if (n == N) {
    hipLaunchKernelGGL(walk_cplx_minors<N>, dim3(grid), dim3(kBlock), 0, s, p, hbits, ostride);
    return hipGetLastError();
  }
  if constexpr (N < HI) return launch_rec<N + 1, HI>(n, p, hbits, ostride, grid, s);
  return hipErrorInvalidValue;
}

template <int N, int HI>
static hipError_t occ_rec(int n, int* blocks_per_cu) {
  if (n == N) return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, walk_cplx_minors<N>, kBlock, 0);
  if constexpr (N < HI) return occ_rec<N + 1, HI>(n, blocks_per_cu);
  return hipErrorInvalidValue;
}

// the 1_16 range starts at N = 2: one row has no walk (its minor is empty)
constexpr int kLo = SUP_N_LO < 2 ? 2 : SUP_N_LO;

#define SUP_CAT2(a, b) a##b
#define SUP_CAT(a, b) SUP_CAT2(a, b)

hipError_t SUP_CAT(launch_cplxm_, SUP_N_LO)(int n, const WalkParams& p, int hbits, unsigned long long ostride, int grid,
                                            hipStream_t s) {
  return launch_rec<kLo, SUP_N_HI>(n, p, hbits, ostride, grid, s);
}
hipError_t SUP_CAT(occupancy_cplxm_, SUP_N_LO)(int n, int* blocks_per_cu) {
  return occ_rec<kLo, SUP_N_HI>(n, blocks_per_cu);
}

}  // namespace sup
