// haf_walk.hpp — the device side of the hafnian walk that walk_haf.hip (one
// order per launch) and walk_lhafe.hip (ragged: an order, a Horner bound and a
// coefficient row per matrix) share: the scalar-load helpers, the G updates and
// the walk over a slab's wave-chunk queue, haf_walk_queue<LOOP, EACH>.  The
// operations and their order are stated at the top of walk_haf.hip; EACH only
// changes where n and the coefficient row come from (HafMat::ord instead of
// HafParams::n and ::coef), both wave-uniform scalar loads per wave-chunk.
// Device code only.
#pragma once
#include "cx.hpp"
#include "haf.hpp"
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

// The walk over the queue of HafParams (the kernel's only argument, read by
// HAF_KARG).  EACH (with LOOP): the matrices of the slab differ in order.
template <bool LOOP, bool EACH>
__device__ __forceinline__ void haf_walk_queue() {
  static_assert(LOOP || !EACH, "ragged slabs hold loop hafnians");
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
      uint32_t n;
      const double* coef;
      if constexpr (EACH) {  // the matrix's own order and coefficient row: scalars of this wave-chunk
        const uint32_t ord = M->ord;
        n = ord & 0xffu;
        coef = HAF_KARG(coef) + (ord >> 8);
      } else {
        n = HAF_KARG(n);
        coef = HAF_KARG(coef);
      }
      const uint32_t m = n >> 1;
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

}  // namespace sup
