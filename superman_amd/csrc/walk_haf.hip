// walk_haf.hip — the hafnian / loop hafnian walk for gfx950
// (sup_hafnian_complex, sup_loop_hafnian_complex; hafnian.cpp).
//
// Kan's sum over multiplicity vectors v (haf.hpp) is walked as walk_cplxf.hip
// walks its sum: the walk digits in reflected mixed-radix Gray order, the same
// for every lane (the step program: digit, direction and the weight of the
// state reached, read by scalar loads), the high digits h = 64 chunk + lane
// decoded per lane at the chunk start.  The summand is a power of one running
// quadratic form, so a lane holds Q = q / 2, G_e = (B h)_e for the W <= 10 walk
// digits, r (loop form), the accumulator and its high-digit weight: no array
// of n row sums, and one kernel for every n, templated on LOOP only.
//
// Per step and lane (the step row's entries are wave-uniform SGPR operands):
//   Q    = fma(-2 delta, G_d, Q) + B_dd     G_d picked by a uniform switch
//   G_e += -delta B_ed, e < 4 or e < 10     r += -delta mu_d (LOOP)
// (a step row arrives as 64-byte scalar loads, a program entry as one of 16)
//   term = Q^m (haf_pow) or the loop polynomial (haf_loop_poly)
//   acc += w * term                         2 muls, 2 adds (no fma)
// Chunk start: with dv_j = -v_j the lane's high digits,
//   t  = (B h(0))_j + sum_{j' < j} dv_j' B(j, j')      fma per part, j' ascending
//   Q  = fma(dv_j^2, B_jj, fma(2 dv_j, t, Q));  r = fma(dv_j, mu_j, r)
//   G_e = fma(dv_j, B(j, e), G_e), e < 4 or e < 10     for j ascending
// The digits already decoded are kept packed (6 bits each) in three 64-bit
// registers and picked by the uniform j': no indexed register array.
// hafnian.cpp's host twin runs the same operations in the same order.
// Resource report and op census: profiles/hafnian/walk_haf_resources.log.
#include "cx.hpp"
#include "haf.hpp"
#include "kernels.hpp"
#include "walk_common.hpp"

namespace sup {

// A wave-uniform descriptor read by scalar loads (walk_cplxf.hip cxf_uniform).
template <class T>
__device__ __forceinline__ const __attribute__((address_space(4))) T* haf_uniform(const T* base, uint64_t index) {
  uint64_t a = (uint64_t)base;
  asm volatile("" : "+s"(a));
  return (const __attribute__((address_space(4))) T*)(a + index * sizeof(T));
}

// A kernel argument read where it is used (walk_common.hpp karg_at): not held
// in SGPRs across the walk.
#define HAF_KARG(field) karg_at<decltype(HafParams::field)>((uint32_t)__builtin_offsetof(HafParams, field))

__device__ __forceinline__ cx haf_ld(cdbl* row, int pair) { return cx{row[2 * pair], row[2 * pair + 1]}; }

// 64-lane pairwise sum of re and im (ascending xor offsets).
__device__ __forceinline__ cx haf_wave_sum(cx v) {
#pragma unroll
  for (int off = 1; off <= 32; off <<= 1) {
    const cx o{__shfl_xor(v.re, off, 64), __shfl_xor(v.im, off, 64)};
    v = cx_add(v, o);
  }
  return v;
}

typedef const __attribute__((address_space(4))) dbl8 cdbl8;
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(4))) u32x4 cu32x4;

// G_e += the four pairs of one 64-byte piece of a step row, e = E0 .. E0 + 3.
// The walk updates e < 4 always and e in [4, 10) when W > 4 (one uniform
// branch): the entries of e >= W are +0, and G_e stays +0 there.  A step row
// is read as 64-byte pieces (one scalar load each; rows start on 64 bytes).
template <int E0, int CNT>
__device__ __forceinline__ void haf_add_g(cx (&G)[kHafWalkDigits], const dbl8& c) {
#pragma unroll
  for (int e = 0; e < CNT; ++e) G[E0 + e] = cx{G[E0 + e].re + c[2 * e], G[E0 + e].im + c[2 * e + 1]};
}
// G_e = fma(dv, row[3 + e], G_e) on e in [LO, HI), likewise.
template <int LO, int HI>
__device__ __forceinline__ void haf_mad_g(cx (&G)[kHafWalkDigits], cdbl* row, double dv) {
#pragma unroll
  for (int e = LO; e < HI; ++e) {
    const cx b = haf_ld(row, 3 + e);
    G[e] = cx{__builtin_fma(dv, b.re, G[e].re), __builtin_fma(dv, b.im, G[e].im)};
  }
}

// G_d for a wave-uniform d < 10: a uniform switch, no indexed register array.
__device__ __forceinline__ cx haf_pick(const cx (&G)[kHafWalkDigits], uint32_t d) {
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
__device__ __forceinline__ cx haf_term(cx Q, cx r, uint32_t m, uint32_t n, const double* coef) {
  if constexpr (LOOP) {
    return haf_loop_poly(Q, r, opaque_c(coef, 0), n);
  } else {
    return haf_pow(Q, m);
  }
}

template <bool LOOP>
__global__ __launch_bounds__(kBlock) void walk_haf(HafParams) {  // arguments: HAF_KARG
  const uint32_t lane = threadIdx.x & 63u;

  for (uint32_t g = next_chunk(HAF_KARG(counter)); (uint64_t)g * HAF_KARG(group) < HAF_KARG(chunk_count);
       g = next_chunk(HAF_KARG(counter))) {
    cx keep{0.0, 0.0};  // lane j keeps the partial of chunk g * group + j
    for (uint32_t j = 0; j < HAF_KARG(group); ++j) {
      const uint64_t a = (uint64_t)g * HAF_KARG(group) + j;
      if (a >= HAF_KARG(chunk_count)) break;
      const uint32_t mat = haf_uniform(HAF_KARG(chunks), a)->mat;
      const uint32_t local = haf_uniform(HAF_KARG(chunks), a)->local;
      const auto* M = haf_uniform(HAF_KARG(mats), mat);
      const double* tab = HAF_KARG(tabs) + M->tab;
      const uint32_t Tw = M->Tw, W = M->W;
      const uint32_t n = HAF_KARG(n), m = n >> 1;
      const double* coef = HAF_KARG(coef);
      const uint32_t h = 64u * local + lane;
      const bool lane_valid = h < M->H;
      // chunk start: the state at v = 0, then the high digits of h, lowest first
      cx Q, r, G[kHafWalkDigits];
      double hw = 1.0;
      {
        cdbl* st = opaque_c(tab, 0);
        Q = haf_ld(st, 0);
        r = haf_ld(st, 1);
#pragma unroll
        for (int e = 0; e < kHafWalkDigits; ++e) G[e] = haf_ld(st, 2 + e);
        uint32_t rem = lane_valid ? h : 0u;
        const uint32_t ndig = M->ndig, dig0 = M->dig;
        const uint32_t hs = 16u * ((uint32_t)kHafHigh + ndig);
        const uint32_t high0 = 16u * ((uint32_t)kHafStart + 2u * W * (uint32_t)kHafRow);
        uint64_t pk0 = 0, pk1 = 0, pk2 = 0;  // the digits decoded so far, 6 bits each, 10 per word
        for (uint32_t d = 0; d < ndig; ++d) {
          const auto* D = haf_uniform(HAF_KARG(dig), (uint64_t)dig0 + d);
          const uint32_t radix = D->radix;
          const uint32_t qd = rem / radix;
          const uint32_t v = rem - qd * radix;
          rem = qd;
          hw = hw * HAF_KARG(wts)[D->wt_off + v];
          const double dvd = -(double)v;
          cdbl* row = opaque_c(tab, high0 + d * hs);
          cx t = haf_ld(row, 0);
          for (uint32_t e = 0; e < d; ++e) {
            const uint64_t word = e < 10u ? pk0 : e < 20u ? pk1 : pk2;
            const double dve = -(double)(uint32_t)((word >> (6u * (e % 10u))) & 63u);
            const cx b = haf_ld(row, kHafHigh + (int)e);
            t = cx{__builtin_fma(dve, b.re, t.re), __builtin_fma(dve, b.im, t.im)};
          }
          const double d2 = dvd + dvd, dd = dvd * dvd;
          const cx bjj = haf_ld(row, 1);
          Q = cx{__builtin_fma(d2, t.re, Q.re), __builtin_fma(d2, t.im, Q.im)};
          Q = cx{__builtin_fma(dd, bjj.re, Q.re), __builtin_fma(dd, bjj.im, Q.im)};
          if constexpr (LOOP) {
            const cx u = haf_ld(row, 2);
            r = cx{__builtin_fma(dvd, u.re, r.re), __builtin_fma(dvd, u.im, r.im)};
          }
          haf_mad_g<0, 4>(G, row, dvd);
          if (W > 4u) haf_mad_g<4, kHafWalkDigits>(G, row, dvd);
          const uint64_t bits = (uint64_t)v << (6u * (d % 10u));
          if (d < 10u) pk0 |= bits;
          else if (d < 20u) pk1 |= bits;
          else pk2 |= bits;
        }
      }
      cx acc = haf_term<LOOP>(Q, r, m, n, coef);  // t = 0, weight +1
      if (Tw > 1) {
        const HafStep* prog = HAF_KARG(prog) + M->prog;
        // an entry is one 16-byte scalar load
        u32x4 en = *(cu32x4*)haf_uniform(prog, 1);
        uint32_t off = en[0], dsg = en[1];
        double w = __hiloint2double((int)en[3], (int)en[2]);
        for (uint32_t t = 1; t < Tw; ++t) {
          // the next entry is asked for before this step's arithmetic (the
          // program ends with a padding entry)
          en = *(cu32x4*)haf_uniform(prog, (uint64_t)t + 1);
          const uint32_t off_n = en[0], dsg_n = en[1];
          const double w_n = __hiloint2double((int)en[3], (int)en[2]);
          cdbl8* row = (cdbl8*)opaque_c(tab, off);
          const dbl8 c0 = row[0], c2 = row[2];  // pairs 0..3 and 8..11 (G_8, G_9, B_dd, -delta mu_d)
          const double m2 = (dsg & 1u) ? 2.0 : -2.0;  // -2 delta
          const cx gd = haf_pick(G, dsg >> 1);
          Q = cx{__builtin_fma(m2, gd.re, Q.re), __builtin_fma(m2, gd.im, Q.im)};
          Q = cx{Q.re + c2[4], Q.im + c2[5]};
          haf_add_g<0, 4>(G, c0);
          if (W > 4u) {
            const dbl8 c1 = row[1];
            haf_add_g<4, 4>(G, c1);
            haf_add_g<8, 2>(G, c2);
          }
          if constexpr (LOOP) r = cx{r.re + c2[6], r.im + c2[7]};
          const cx term = haf_term<LOOP>(Q, r, m, n, coef);
          const double mr = w * term.re, mi = w * term.im;
          acc = cx{acc.re + mr, acc.im + mi};
          off = off_n;
          dsg = dsg_n;
          w = w_n;
        }
      }
      acc = cx{acc.re * hw, acc.im * hw};
      const cx part = haf_wave_sum(lane_valid ? acc : cx{0.0, 0.0});
      if (lane == j) keep = part;
    }
    const uint64_t a = (uint64_t)g * HAF_KARG(group) + lane;
    if (lane < HAF_KARG(group) && a < HAF_KARG(chunk_count)) {
      HAF_KARG(chunk_out)[2 * a] = keep.re;
      HAF_KARG(chunk_out)[2 * a + 1] = keep.im;
    }
  }
}

// haf_prepare: one block per matrix writes its table (haf.hpp haf_entry, the
// host twin's own function) from A, mu and the recorded groups.
__global__ __launch_bounds__(kBlock) void haf_prepare(const double* __restrict__ A, int Mo,
                                                      const double* __restrict__ mu,
                                                      const int32_t* __restrict__ grp,
                                                      const HafMat* __restrict__ mats, double* __restrict__ tabs) {
  const HafMat M = mats[blockIdx.x];
  double* t = tabs + M.tab;
  const int32_t* g = grp + M.grp;
  for (uint32_t e = threadIdx.x; e < M.pairs; e += kBlock) {
    const cx v = haf_entry(A, Mo, mu, g, (int)M.K, (int)M.W, (int)M.ndig, e);
    t[2 * (uint64_t)e] = v.re;
    t[2 * (uint64_t)e + 1] = v.im;
  }
}

// haf_fold: one thread per matrix runs fock_fold over the matrix's chunk
// partials and writes (2 x the sum) / div: div = m! for the hafnian, 1 for the
// loop hafnian.
__global__ __launch_bounds__(kBlock) void haf_fold(const double* __restrict__ parts, const HafMat* __restrict__ mats,
                                                   uint64_t K, double div, double* __restrict__ out) {
  const uint64_t k = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (k >= K) return;
  const cx v = fock_fold(parts + 2 * (uint64_t)mats[k].chunk0, mats[k].chunks);
  out[2 * k] = (2.0 * v.re) / div;
  out[2 * k + 1] = (2.0 * v.im) / div;
}

hipError_t launch_haf(bool loop, const HafParams& p, int grid, hipStream_t s) {
  if (p.n < 1 || p.n > 64 || (!loop && (p.n & 1u)) || grid < 1) return hipErrorInvalidValue;
  if (loop)
    hipLaunchKernelGGL(walk_haf<true>, dim3(grid), dim3(kBlock), 0, s, p);
  else
    hipLaunchKernelGGL(walk_haf<false>, dim3(grid), dim3(kBlock), 0, s, p);
  return hipGetLastError();
}

hipError_t haf_occupancy(bool loop, int* blocks_per_cu) {
  return loop ? hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, walk_haf<true>, kBlock, 0)
              : hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, walk_haf<false>, kBlock, 0);
}

hipError_t launch_haf_prepare(const double* A, int M, const double* mu, const int32_t* grp, const HafMat* mats,
                              uint64_t K, double* tabs, hipStream_t s) {
  if (M < 1 || K == 0 || K > 0x7fffffffull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(haf_prepare, dim3((unsigned)K), dim3(kBlock), 0, s, A, M, mu, grp, mats, tabs);
  return hipGetLastError();
}

hipError_t launch_haf_fold(const double* parts, const HafMat* mats, uint64_t K, double div, double* out,
                           hipStream_t s) {
  if (K == 0) return hipErrorInvalidValue;
  const uint64_t blocks = (K + kBlock - 1) / kBlock;
  if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(haf_fold, dim3((unsigned)blocks), dim3(kBlock), 0, s, parts, mats, K, div, out);
  return hipGetLastError();
}

}  // namespace sup
