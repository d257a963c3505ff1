// walk_hafexact.hip — the exact hafnian / loop hafnian walk for gfx950
// (sup_hafnian_complex_exact; hafnian_exact.cpp).
//
// walk_haf.hip's walk of Kan's sum (the same slab descriptors, step programs,
// ticket queue and lane layout) on integers: a lane holds q' = H^T Abar H,
// G'_e = (Abar H)_e for the W <= 10 walk digits and r' (loop form), all exact
// in fp64 (hafexact.hpp), and per prime of the launch an accumulator and the
// residue of its high-digit weight.  Per state, shared by the primes:
//   q'   = fma(-4 delta, G'_d, q') + 4 Abar_dd    G'_d picked by a uniform switch
//   G'_e += -2 delta Abar_ed, e < 4 or e < 10     r' += -2 delta mubar_d (LOOP)
// and per prime p (its constants are wave-uniform scalar loads from ptab):
//   Q = cxe_red2(q'), (r = cxe_red2(r'))
//   term = Q^m (hafx_pow) or the loop polynomial (hafx_loop_poly), cxe_link for every product
//   acc += cxe_red2(w term)                        w = the step weight mod p
//   acc = cxe_red2(acc) every 256 states           (|acc| grows by < 1.5 p a state)
// Chunk end, per prime: acc times the lane's high-digit weight mod p, the
// lane-valid mask, the exact 64-lane sum (64 x 1.5 p), canonicalisation into
// [0, p) and one vector store per wave-chunk, prime and part.  hafx_fold adds
// a matrix's chunk residues (below 2^24 chunks x 2^25: exact); the host takes
// them modulo p.  Every operation is exact, so the host twin
// (hafnian_exact.cpp) agrees residue for residue whatever the split.
// One kernel per form serves every n <= 64: no device cap.
//
// Primes per launch: kHafxPrimes = 8, chosen from the compiled code.  A prime
// costs about 6 VGPRs (its accumulator, its high-digit weight, and what the
// unrolled prime loop keeps in flight) and its constants are scalar loads; more
// primes in a launch share the integer step.  Compiler resource report per
// scanned value (tools/probes/hafexact_resources.py,
// profiles/hafnian_exact/walk_hafexact_resources.log):
//   primes  plain: VGPRs  waves/SIMD  spilled SGPRs   loop: VGPRs  waves/SIMD  spilled SGPRs
//   4              86     5           0                      105    4           10
//   8              111    4           25                     129    3           35
//   12             135    3           56                     153    3           60
//   16             160    3           82                     178    2           91
// No scratch, no spilled VGPR and no AGPR at any of them.  8 is the largest
// that keeps 4 waves per SIMD in the plain form.  The spilled SGPRs (VGPR
// lanes) are hoisted table addresses: the plain form reads none back inside
// the walk loop, the loop form five.  More primes than 8 take several launches
// over the same tables (engine.cpp run_hafnian_exact).
#include "cx.hpp"
#include "hafexact.hpp"
#include "hafnian_exact.hpp"
#include "kernels.hpp"
#include "walk_common.hpp"

namespace sup {

template <class T>
__device__ __forceinline__ const __attribute__((address_space(4))) T* hafx_uniform(const T* base, uint64_t index) {
  uint64_t a = (uint64_t)base;
  asm volatile("" : "+s"(a));
  return (const __attribute__((address_space(4))) T*)(a + index * sizeof(T));
}

// A kernel argument read where it is used (walk_common.hpp karg_at).
#define HAFX_KARG(field) karg_at<decltype(HafxParams::field)>((uint32_t)__builtin_offsetof(HafxParams, field))

__device__ __forceinline__ cx hafx_ld(cdbl* row, int pair) { return cx{row[2 * pair], row[2 * pair + 1]}; }

typedef const __attribute__((address_space(4))) dbl8 cdbl8;
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(4))) u32x4 cu32x4;

template <int E0, int CNT>
__device__ __forceinline__ void hafx_add_g(cx (&G)[kHafWalkDigits], const dbl8& c) {
#pragma unroll
  for (int e = 0; e < CNT; ++e) G[E0 + e] = cx{G[E0 + e].re + c[2 * e], G[E0 + e].im + c[2 * e + 1]};
}
template <int LO, int HI>
__device__ __forceinline__ void hafx_mad_g(cx (&G)[kHafWalkDigits], cdbl* row, double dv) {
#pragma unroll
  for (int e = LO; e < HI; ++e) {
    const cx b = hafx_ld(row, 3 + e);
    G[e] = cx{__builtin_fma(dv, b.re, G[e].re), __builtin_fma(dv, b.im, G[e].im)};
  }
}

// G'_d for a wave-uniform d < 10: a uniform switch, no indexed register array.
__device__ __forceinline__ cx hafx_pick(const cx (&G)[kHafWalkDigits], uint32_t d) {
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

// The term of the state (q', r') modulo the prime whose constants start at pc.
template <bool LOOP>
__device__ __forceinline__ cx hafx_term(cx q, cx r, uint32_t m, uint32_t n, cdbl* pc, double p, double pinv) {
  const cx Q = cxe_red2(q, p, pinv);
  if constexpr (LOOP) {
    return hafx_loop_poly(Q, cxe_red2(r, p, pinv), pc + kHafxCoef, n, p, pinv);
  } else {
    return hafx_pow(Q, m, p, pinv);
  }
}

template <bool LOOP>
__global__ __launch_bounds__(kBlock) void walk_hafexact(HafxParams) {  // arguments: HAFX_KARG
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t np = HAFX_KARG(nprimes);
  const uint32_t pstride = 8u * HAFX_KARG(stride);  // bytes per prime in ptab

  for (uint32_t g = next_chunk(HAFX_KARG(counter)); (uint64_t)g * HAFX_KARG(group) < HAFX_KARG(chunk_count);
       g = next_chunk(HAFX_KARG(counter))) {
    for (uint32_t j = 0; j < HAFX_KARG(group); ++j) {
      const uint64_t a = (uint64_t)g * HAFX_KARG(group) + j;
      if (a >= HAFX_KARG(chunk_count)) break;
      const uint32_t mat = hafx_uniform(HAFX_KARG(chunks), a)->mat;
      const uint32_t local = hafx_uniform(HAFX_KARG(chunks), a)->local;
      const auto* M = hafx_uniform(HAFX_KARG(mats), mat);
      const double* tab = HAFX_KARG(tabs) + M->tab;
      const uint32_t Tw = M->Tw, W = M->W;
      const uint32_t n = HAFX_KARG(n), m = n >> 1;
      const uint32_t h = 64u * local + lane;
      const bool lane_valid = h < M->H;
      // chunk start: the state at v = 0, then the high digits of h, lowest first
      cx Q, r, G[kHafWalkDigits];
      double hw[kHafxPrimes];  // the lane's high-digit weight mod each prime, in (-1.5 p, 1.5 p)
#pragma unroll
      for (int q = 0; q < kHafxPrimes; ++q) hw[q] = 1.0;
      {
        cdbl* st = opaque_c(tab, 0);
        Q = hafx_ld(st, 0);
        r = hafx_ld(st, 1);
#pragma unroll
        for (int e = 0; e < kHafWalkDigits; ++e) G[e] = hafx_ld(st, 2 + e);
        uint32_t rem = lane_valid ? h : 0u;
        const uint32_t ndig = M->ndig, dig0 = M->dig;
        const uint32_t hs = 16u * ((uint32_t)kHafHigh + ndig);
        const uint32_t high0 = 16u * ((uint32_t)kHafStart + 2u * W * (uint32_t)kHafRow);
        uint64_t pk0 = 0, pk1 = 0, pk2 = 0;  // the digits decoded so far, 6 bits each, 10 per word
        for (uint32_t d = 0; d < ndig; ++d) {
          const auto* D = hafx_uniform(HAFX_KARG(dig), (uint64_t)dig0 + d);
          const uint32_t radix = D->radix;
          const uint32_t qd = rem / radix;
          const uint32_t v = rem - qd * radix;  // v < radix <= 64: inside the binomial row
          rem = qd;
          const uint32_t wi = (uint32_t)kHafxBinom + D->wt_off + v;
#pragma unroll
          for (int q = 0; q < kHafxPrimes; ++q)
            if ((uint32_t)q < np) {
              cdbl* pc = opaque_c(HAFX_KARG(ptab), (uint32_t)q * pstride);
              const double bw = HAFX_KARG(ptab)[(uint64_t)q * (pstride / 8u) + wi];  // per lane
              hw[q] = cxe_red(hw[q] * bw, pc[0], pc[1]);
            }
          const double dvd = -(double)v;
          cdbl* row = opaque_c(tab, high0 + d * hs);
          cx t = hafx_ld(row, 0);
          for (uint32_t e = 0; e < d; ++e) {
            const uint64_t word = e < 10u ? pk0 : e < 20u ? pk1 : pk2;
            const double dve = -(double)(uint32_t)((word >> (6u * (e % 10u))) & 63u);
            const cx b = hafx_ld(row, kHafHigh + (int)e);
            t = cx{__builtin_fma(dve, b.re, t.re), __builtin_fma(dve, b.im, t.im)};
          }
          const double d4 = 4.0 * dvd, dd = dvd * dvd;
          const cx bjj = hafx_ld(row, 1);
          Q = cx{__builtin_fma(d4, t.re, Q.re), __builtin_fma(d4, t.im, Q.im)};
          Q = cx{__builtin_fma(dd, bjj.re, Q.re), __builtin_fma(dd, bjj.im, Q.im)};
          if constexpr (LOOP) {
            const cx u = hafx_ld(row, 2);
            r = cx{__builtin_fma(dvd, u.re, r.re), __builtin_fma(dvd, u.im, r.im)};
          }
          hafx_mad_g<0, 4>(G, row, dvd);
          if (W > 4u) hafx_mad_g<4, kHafWalkDigits>(G, row, dvd);
          const uint64_t bits = (uint64_t)v << (6u * (d % 10u));
          if (d < 10u) pk0 |= bits;
          else if (d < 20u) pk1 |= bits;
          else pk2 |= bits;
        }
      }
      cx acc[kHafxPrimes];
#pragma unroll
      for (int q = 0; q < kHafxPrimes; ++q) {
        acc[q] = cx{0.0, 0.0};
        if ((uint32_t)q < np) {  // t = 0, weight +1
          cdbl* pc = opaque_c(HAFX_KARG(ptab), (uint32_t)q * pstride);
          acc[q] = hafx_term<LOOP>(Q, r, m, n, pc, pc[0], pc[1]);
        }
      }
      if (Tw > 1) {
        const uint32_t prog0 = M->prog;
        const HafStep* prog = HAFX_KARG(prog) + prog0;
        // an entry is one 16-byte scalar load (its fp64 weight is not used)
        u32x4 en = *(cu32x4*)hafx_uniform(prog, 1);
        uint32_t off = en[0], dsg = en[1];
        for (uint32_t t = 1; t < Tw; ++t) {
          // the next entry is asked for before this step's arithmetic (the
          // program ends with a padding entry)
          en = *(cu32x4*)hafx_uniform(prog, (uint64_t)t + 1);
          const uint32_t off_n = en[0], dsg_n = en[1];
          cdbl8* row = (cdbl8*)opaque_c(tab, off);
          const dbl8 c0 = row[0], c2 = row[2];  // pairs 0..3 and 8..11 (G'_8, G'_9, 4 Abar_dd, -2 delta mubar_d)
          const double m4 = (dsg & 1u) ? 4.0 : -4.0;  // -4 delta
          const cx gd = hafx_pick(G, dsg >> 1);
          Q = cx{__builtin_fma(m4, gd.re, Q.re), __builtin_fma(m4, gd.im, Q.im)};
          Q = cx{Q.re + c2[4], Q.im + c2[5]};
          hafx_add_g<0, 4>(G, c0);
          if (W > 4u) {
            const dbl8 c1 = row[1];
            hafx_add_g<4, 4>(G, c1);
            hafx_add_g<8, 2>(G, c2);
          }
          if constexpr (LOOP) r = cx{r.re + c2[6], r.im + c2[7]};
          const bool fold = (t & 255u) == 0u;
#pragma unroll
          for (int q = 0; q < kHafxPrimes; ++q)
            if ((uint32_t)q < np) {
              cdbl* pc = opaque_c(HAFX_KARG(ptab), (uint32_t)q * pstride);
              const double p = pc[0], pinv = pc[1];
              const double w = pc[(uint32_t)kHafxStepW + prog0 + t];
              const cx term = hafx_weigh(hafx_term<LOOP>(Q, r, m, n, pc, p, pinv), w, p, pinv);
              acc[q] = cx_add(acc[q], term);
              if (fold) acc[q] = cxe_red2(acc[q], p, pinv);
            }
          off = off_n;
          dsg = dsg_n;
        }
      }
      // chunk end: per prime the weighted, masked, exact 64-lane sum in [0, p)
#pragma unroll
      for (int q = 0; q < kHafxPrimes; ++q)
        if ((uint32_t)q < np) {
          cdbl* pc = opaque_c(HAFX_KARG(ptab), (uint32_t)q * pstride);
          const double p = pc[0], pinv = pc[1];
          const cx s = hafx_weigh(cxe_red2(acc[q], p, pinv), hw[q], p, pinv);  // 2.25 p^2 < 2^52
          cx v = lane_valid ? s : cx{0.0, 0.0};
#pragma unroll
          for (int o = 1; o <= 32; o <<= 1) v = cx_add(v, cx{__shfl_xor(v.re, o, 64), __shfl_xor(v.im, o, 64)});
          double res[2] = {cxe_red(v.re, p, pinv), cxe_red(v.im, p, pinv)};
#pragma unroll
          for (int part = 0; part < 2; ++part) {
            if (res[part] < 0.0) res[part] += p;
            if (res[part] < 0.0) res[part] += p;
            if (res[part] >= p) res[part] -= p;
            if (lane == 0) HAFX_KARG(chunk_out)[(a * (uint64_t)kHafxPrimes + (uint64_t)q) * 2u + (uint64_t)part] = res[part];
          }
        }
    }
  }
}

// hafx_prepare: one block per matrix writes its integer table (hafexact.hpp
// hafx_entry, the host twin's own function) from A, mu and the recorded groups.
__global__ __launch_bounds__(kBlock) void hafx_prepare(const double* __restrict__ A, int Mo,
                                                       const double* __restrict__ mu,
                                                       const int32_t* __restrict__ grp,
                                                       const HafMat* __restrict__ mats, double* __restrict__ tabs) {
  const HafMat M = mats[blockIdx.x];
  double* t = tabs + M.tab;
  const int32_t* g = grp + M.grp;
  for (uint32_t e = threadIdx.x; e < M.pairs; e += kBlock) {
    const cx v = hafx_entry(A, Mo, mu, g, (int)M.K, (int)M.W, (int)M.ndig, e);
    t[2 * (uint64_t)e] = v.re;
    t[2 * (uint64_t)e + 1] = v.im;
  }
}

// hafx_fold: one thread per (matrix, prime, part) adds the matrix's chunk
// residues (each in [0, p), p < 2^25, at most 2^24 chunks: the sum is exact);
// the host reduces it modulo p.  out[(k kHafxPrimes + q) 2 + part].
__global__ __launch_bounds__(kBlock) void hafx_fold(const double* __restrict__ parts, const HafMat* __restrict__ mats,
                                                    uint64_t K, uint32_t nprimes, double* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  constexpr uint64_t per = 2u * (uint64_t)kHafxPrimes;
  if (i >= K * per) return;
  const uint64_t k = i / per, qp = i - k * per;
  if (qp >= 2u * (uint64_t)nprimes) {  // a prime the launch does not have: nothing was stored
    out[i] = 0.0;
    return;
  }
  const double* src = parts + (uint64_t)mats[k].chunk0 * per + qp;
  double s = 0.0;
  for (uint32_t c = 0; c < mats[k].chunks; ++c) s += src[(uint64_t)c * per];
  out[i] = s;
}

hipError_t launch_hafexact(bool loop, const HafxParams& p, int grid, hipStream_t s) {
  if (p.n < 1 || p.n > 64 || (!loop && (p.n & 1u)) || grid < 1 || p.nprimes < 1 || p.nprimes > (unsigned)kHafxPrimes)
    return hipErrorInvalidValue;
  if (loop)
    hipLaunchKernelGGL(walk_hafexact<true>, dim3(grid), dim3(kBlock), 0, s, p);
  else
    hipLaunchKernelGGL(walk_hafexact<false>, dim3(grid), dim3(kBlock), 0, s, p);
  return hipGetLastError();
}

hipError_t hafexact_occupancy(bool loop, int* blocks_per_cu) {
  return loop ? hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, walk_hafexact<true>, kBlock, 0)
              : hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, walk_hafexact<false>, kBlock, 0);
}

hipError_t launch_hafexact_prepare(const double* A, int M, const double* mu, const int32_t* grp, const HafMat* mats,
                                   uint64_t K, double* tabs, hipStream_t s) {
  if (M < 1 || K == 0 || K > 0x7fffffffull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(hafx_prepare, dim3((unsigned)K), dim3(kBlock), 0, s, A, M, mu, grp, mats, tabs);
  return hipGetLastError();
}

hipError_t launch_hafexact_fold(const double* parts, const HafMat* mats, uint64_t K, uint32_t nprimes, double* out,
                                hipStream_t s) {
  if (K == 0 || nprimes < 1 || nprimes > (uint32_t)kHafxPrimes) return hipErrorInvalidValue;
  const uint64_t blocks = (K * 2u * (uint64_t)kHafxPrimes + kBlock - 1) / kBlock;
  if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(hafx_fold, dim3((unsigned)blocks), dim3(kBlock), 0, s, parts, mats, K, nprimes, out);
  return hipGetLastError();
}

}  // namespace sup
