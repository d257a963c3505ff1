// walk_hafdd.hip — the hafnian / loop hafnian walk in complex double-double
// for gfx950 (sup_hafnian_complex_quad, sup_loop_hafnian_complex_quad;
// hafnian_quad.cpp): hafnians to ~100 bits, the truth the fp64
// Kan walk (walk_haf.hip) and the power-trace kernel are judged against on
// matrices that are not Gaussian integers.
//
// Enumeration, digits, step program order, wave-chunk queue and chunk start
// order are walk_haf.hip's (haf_walk.hpp); every running value is a cxdd and
// every operation is hafdd.hpp's, listed at the top of that file: a lane holds
// Q, r, ten G_e, the accumulator (4 doubles each) and its dd high-digit weight,
// 58 doubles, beside the temporaries of cxdd_mul.  One kernel per form serves
// every n <= 64.  A program entry (32 bytes: row, digit and direction, the dd
// weight) arrives as two 16-byte scalar loads, a step row as 64-byte scalar
// loads; G_d is picked by a uniform switch and the high digits already decoded
// are kept packed in three 64-bit registers: no indexed register array.  All
// wave-uniform data is read by scalar loads; everything written goes through
// ordinary vector stores.  hafnian_quad.cpp's host twin runs the same
// operations in the same order.
// Resource report: profiles/hafnian_quad/walk_hafdd_resources.log.
#include "cxdd.hpp"
#include "haf_walk.hpp"
#include "hafdd.hpp"
#include "hafnian_quad.hpp"
#include "kernels.hpp"
#include "walk_common.hpp"

namespace sup {

#define HAFDD_KARG(field) karg_at<decltype(HafddParams::field)>((uint32_t)__builtin_offsetof(HafddParams, field))

// The cxdd at doubles [4 slot, 4 slot + 4) of a scalar-loaded row.
__device__ __forceinline__ cxdd hafdd_ld4(cdbl* row, int slot) {
  return cxdd{dd{row[4 * slot], row[4 * slot + 1]}, dd{row[4 * slot + 2], row[4 * slot + 3]}};
}

__device__ __forceinline__ dd hafdd_dd_wave_sum(dd v) {
#pragma unroll
  for (int off = 1; off <= 32; off <<= 1) {
    const dd o{__shfl_xor(v.hi, off, 64), __shfl_xor(v.lo, off, 64)};
    v = dd_add(v, o);
  }
  return v;
}
// 64-lane pairwise sum (ascending xor offsets) of each part: cxdd_add per level.
__device__ __forceinline__ cxdd hafdd_wave_sum(cxdd v) {
  return cxdd{hafdd_dd_wave_sum(v.re), hafdd_dd_wave_sum(v.im)};
}

// G_e = dd_add_d per part with the four pairs of one 64-byte piece of a step
// row, e = E0 .. E0 + CNT - 1 (haf_walk.hpp haf_add_g).
template <int E0, int CNT>
__device__ __forceinline__ void hafdd_add_g(cxdd (&G)[kHafWalkDigits], const dbl8& c) {
#pragma unroll
  for (int e = 0; e < CNT; ++e) G[E0 + e] = cxdd_add_d2(G[E0 + e], c[2 * e], c[2 * e + 1]);
}
// G_e = G_e + dv B(j, e) on e in [LO, HI): the high row's pairs 4 + e.
template <int LO, int HI>
__device__ __forceinline__ void hafdd_mad_g(cxdd (&G)[kHafWalkDigits], cdbl* row, double dv) {
#pragma unroll
  for (int e = LO; e < HI; ++e) {
    const cx b = haf_ld(row, 4 + e);
    G[e] = hafdd_mad(G[e], dv, b.re, b.im);
  }
}

__device__ __forceinline__ cxdd hafdd_pick(const cxdd (&G)[kHafWalkDigits], uint32_t d) {
  switch (d) {
    case 0: return G[0];
    case 1: return G[1];
    case 2: return G[2];
    case 3: return G[3];
    case 4: return G[4];
    case 5: return G[5];
    case 6: return G[6];
    case 7: return G[7];
    case 8: return G[8];
    default: return G[9];
  }
}

template <bool LOOP>
__device__ __forceinline__ cxdd hafdd_term(cxdd Q, cxdd r, uint32_t m, uint32_t n, const double* coef) {
  if constexpr (LOOP) {
    return hafdd_loop_poly(Q, r, opaque_c(coef, 0), n);
  } else {
    return hafdd_pow(Q, m);
  }
}

template <bool LOOP>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(2))) void walk_hafdd(HafddParams) {  // arguments: HAFDD_KARG
  const uint32_t lane = threadIdx.x & 63u;
  const cxdd zero{dd{0.0, 0.0}, dd{0.0, 0.0}};

  for (uint32_t g = next_chunk(HAFDD_KARG(counter)); (uint64_t)g * HAFDD_KARG(group) < HAFDD_KARG(chunk_count);
       g = next_chunk(HAFDD_KARG(counter))) {
    cxdd keep = zero;  // lane j keeps the partial of chunk g * group + j
    for (uint32_t j = 0; j < HAFDD_KARG(group); ++j) {
      const uint64_t a = (uint64_t)g * HAFDD_KARG(group) + j;
      if (a >= HAFDD_KARG(chunk_count)) break;
      const uint32_t mat = haf_uniform(HAFDD_KARG(chunks), a)->mat;
      const uint32_t local = haf_uniform(HAFDD_KARG(chunks), a)->local;
      const auto* M = haf_uniform(HAFDD_KARG(mats), mat);
      const double* tab = HAFDD_KARG(tabs) + M->tab;
      const uint32_t Tw = M->Tw, W = M->W;
      const uint32_t n = HAFDD_KARG(n);
      const double* coef = HAFDD_KARG(coef);
      const uint32_t m = n >> 1;
      const uint32_t h = 64u * local + lane;
      const bool lane_valid = h < M->H;
      // chunk start: the state at v = 0, then the high digits of h, lowest first
      cxdd Q, r, G[kHafWalkDigits];
      dd hw{1.0, 0.0};
      {
        cdbl* st = opaque_c(tab, 0);
        Q = hafdd_ld4(st, 0);
        r = hafdd_ld4(st, 1);
#pragma unroll
        for (int e = 0; e < kHafWalkDigits; ++e) G[e] = hafdd_ld4(st, 2 + e);
        uint32_t rem = lane_valid ? h : 0u;
        const uint32_t ndig = M->ndig, dig0 = M->dig;
        const uint32_t hs = 16u * ((uint32_t)kHafddHigh + ndig);
        const uint32_t high0 = 16u * ((uint32_t)kHafddStart + 2u * W * (uint32_t)kHafRow);
        uint64_t pk0 = 0, pk1 = 0, pk2 = 0;  // the digits decoded so far, 6 bits each, 10 per word
        for (uint32_t d = 0; d < ndig; ++d) {
          const auto* D = haf_uniform(HAFDD_KARG(dig), (uint64_t)dig0 + d);
          const uint32_t radix = D->radix;
          const uint32_t qd = rem / radix;
          const uint32_t v = rem - qd * radix;
          rem = qd;
          const double* wt = HAFDD_KARG(wts) + 2u * (D->wt_off + v);
          hw = dd_mul(hw, dd{wt[0], wt[1]});
          const double dvd = -(double)v;
          cdbl* row = opaque_c(tab, high0 + d * hs);
          cxdd t = hafdd_ld4(row, 0);
          for (uint32_t e = 0; e < d; ++e) {
            const uint64_t word = e < 10u ? pk0 : e < 20u ? pk1 : pk2;
            const double dve = -(double)(uint32_t)((word >> (6u * (e % 10u))) & 63u);
            const cx b = haf_ld(row, kHafddHigh + (int)e);
            t = hafdd_mad(t, dve, b.re, b.im);
          }
          const double d2 = dvd + dvd, dsq = dvd * dvd;
          const cx bjj = haf_ld(row, 2);
          Q = hafdd_mad_dd(Q, d2, t);
          Q = hafdd_mad(Q, dsq, bjj.re, bjj.im);
          if constexpr (LOOP) {
            const cx u = haf_ld(row, 3);
            r = hafdd_mad(r, dvd, u.re, u.im);
          }
          hafdd_mad_g<0, 4>(G, row, dvd);
          if (W > 4u) hafdd_mad_g<4, kHafWalkDigits>(G, row, dvd);
          const uint64_t bits = (uint64_t)v << (6u * (d % 10u));
          if (d < 10u) pk0 |= bits;
          else if (d < 20u) pk1 |= bits;
          else pk2 |= bits;
        }
      }
      cxdd acc = hafdd_term<LOOP>(Q, r, m, n, coef);  // t = 0, weight +1
      if (Tw > 1) {
        const HafddStep* prog = HAFDD_KARG(prog) + M->prog;
        // an entry is two 16-byte scalar loads
        cu32x4* pe = (cu32x4*)haf_uniform(prog, 1);
        u32x4 e0 = pe[0], e1 = pe[1];
        uint32_t off = e0[0], dsg = e0[1];
        dd w{__hiloint2double((int)e1[1], (int)e1[0]), __hiloint2double((int)e1[3], (int)e1[2])};
        for (uint32_t t = 1; t < Tw; ++t) {
          // the next entry is asked for before this step's arithmetic (the
          // program ends with a padding entry)
          pe = (cu32x4*)haf_uniform(prog, (uint64_t)t + 1);
          e0 = pe[0], e1 = pe[1];
          const uint32_t off_n = e0[0], dsg_n = e0[1];
          const dd w_n{__hiloint2double((int)e1[1], (int)e1[0]), __hiloint2double((int)e1[3], (int)e1[2])};
          cdbl8* row = (cdbl8*)opaque_c(tab, off);
          const dbl8 c0 = row[0], c2 = row[2];  // pairs 0..3 and 8..11 (G_8, G_9, B_dd, -delta mu_d)
          const double m2 = (dsg & 1u) ? 2.0 : -2.0;  // -2 delta
          Q = hafdd_step_q(Q, hafdd_pick(G, dsg >> 1), m2, c2[4], c2[5]);
          hafdd_add_g<0, 4>(G, c0);
          if (W > 4u) {
            const dbl8 c1 = row[1];
            hafdd_add_g<4, 4>(G, c1);
            hafdd_add_g<8, 2>(G, c2);
          }
          if constexpr (LOOP) r = cxdd_add_d2(r, c2[6], c2[7]);
          acc = hafdd_accum(acc, w, hafdd_term<LOOP>(Q, r, m, n, coef));
          off = off_n;
          dsg = dsg_n;
          w = w_n;
        }
      }
      acc = hafdd_scale(acc, hw);
      const cxdd part = hafdd_wave_sum(lane_valid ? acc : zero);
      if (lane == j) keep = part;
    }
    const uint64_t a = (uint64_t)g * HAFDD_KARG(group) + lane;
    if (lane < HAFDD_KARG(group) && a < HAFDD_KARG(chunk_count)) {
      double* o = HAFDD_KARG(chunk_out) + 4 * a;
      o[0] = keep.re.hi;
      o[1] = keep.re.lo;
      o[2] = keep.im.hi;
      o[3] = keep.im.lo;
    }
  }
}

// hafdd_prepare: one block per matrix writes its table (hafdd.hpp hafdd_entry,
// the host twin's own function) from A, mu and the recorded groups.
__global__ __launch_bounds__(kBlock) void hafdd_prepare(const double* __restrict__ A, int Mo,
                                                        const double* __restrict__ mu,
                                                        const int32_t* __restrict__ grp,
                                                        const HafMat* __restrict__ mats, double* __restrict__ tabs) {
  const HafMat M = mats[blockIdx.x];
  double* t = tabs + M.tab;
  const int32_t* g = grp + M.grp;
  for (uint32_t e = threadIdx.x; e < M.pairs; e += kBlock) {
    const cx v = hafdd_entry(A, Mo, mu, g, (int)M.K, (int)M.W, (int)M.ndig, e);
    t[2 * (uint64_t)e] = v.re;
    t[2 * (uint64_t)e + 1] = v.im;
  }
}

// hafdd_fold: one thread per matrix folds the matrix's chunk partials
// (hafdd_fold_tree) and writes hafdd_finish of the sum: 4 doubles.
__global__ __launch_bounds__(kBlock) void hafdd_fold(const double* __restrict__ parts, const HafMat* __restrict__ mats,
                                                     uint64_t K, double div_hi, double div_lo, int loop,
                                                     double* __restrict__ out) {
  const uint64_t k = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (k >= K) return;
  const cxdd v = hafdd_finish(hafdd_fold_tree(parts + 4 * (uint64_t)mats[k].chunk0, mats[k].chunks),
                              dd{div_hi, div_lo}, loop != 0);
  out[4 * k] = v.re.hi;
  out[4 * k + 1] = v.re.lo;
  out[4 * k + 2] = v.im.hi;
  out[4 * k + 3] = v.im.lo;
}

hipError_t launch_hafdd(bool loop, const HafddParams& p, int grid, hipStream_t s) {
  if (p.n < 1 || p.n > 64 || (!loop && (p.n & 1u)) || grid < 1) return hipErrorInvalidValue;
  if (loop)
    hipLaunchKernelGGL(walk_hafdd<true>, dim3(grid), dim3(kBlock), 0, s, p);
  else
    hipLaunchKernelGGL(walk_hafdd<false>, dim3(grid), dim3(kBlock), 0, s, p);
  return hipGetLastError();
}

hipError_t hafdd_occupancy(bool loop, int* blocks_per_cu) {
  return loop ? hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, walk_hafdd<true>, kBlock, 0)
              : hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, walk_hafdd<false>, kBlock, 0);
}

hipError_t launch_hafdd_prepare(const double* A, int M, const double* mu, const int32_t* grp, const HafMat* mats,
                                uint64_t K, double* tabs, hipStream_t s) {
  if (M < 1 || K == 0 || K > 0x7fffffffull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(hafdd_prepare, dim3((unsigned)K), dim3(kBlock), 0, s, A, M, mu, grp, mats, tabs);
  return hipGetLastError();
}

hipError_t launch_hafdd_fold(const double* parts, const HafMat* mats, uint64_t K, double div_hi, double div_lo,
                             bool loop, double* out, hipStream_t s) {
  if (K == 0) return hipErrorInvalidValue;
  const uint64_t blocks = (K + kBlock - 1) / kBlock;
  if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(hafdd_fold, dim3((unsigned)blocks), dim3(kBlock), 0, s, parts, mats, K, div_hi, div_lo,
                     loop ? 1 : 0, out);
  return hipGetLastError();
}

}  // namespace sup
