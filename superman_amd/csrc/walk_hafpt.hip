// walk_hafpt.hip — the power-trace hafnian / loop hafnian kernel for gfx950
// (sup_hafnian_complex_pt, sup_loop_hafnian_complex_pt and the range entry;
// hafnian_pt.cpp).  hafpt.hpp states the sum and the order of
// every operation; hafnian_pt.cpp's host twin runs the same operations.
//
// One wave (a block of 64 threads) takes one subset z at a time.  Lane i < 2k
// owns compact row i (actual row r_i).  The row being produced, cur[c], is a
// statically indexed register array over the ACTUAL columns c < KP, KP =
// hafpt_kpad(z) in {8, .., 64} picked per subset by a wave-uniform switch: the
// rows of C are then read where prepare wrote them, by scalar loads (64 bytes
// each, wave-uniform operands of the fmas), and no per-subset gather exists.
// The columns outside z are computed and never read: they enter no sum.
// The previous power lives in LDS, T[l][i] at pair l np + i: lanes read and
// write consecutive pairs (conflict-free ds_read_b128 / ds_write_b128), and
// the traces read T[l ^ 1][i ^ 1] the same way.
//   power step:  per l of z:  p = T[l][i];  cur[c] = cx_fma(p, C[l][c], cur[c]), c < KP
//   odd trace:   sum_l cx_fma(cur[l], T[l ^ 1][i ^ 1], .)   (T = P_(a-1))
//   store cur over T;  even trace likewise (T = P_a):  one tile suffices
// The loop part's y lives in 64 pairs of LDS by actual row; x_j, jc_j and g_s
// in 33 pairs each (every lane writes and reads the same values).
// Lanes >= 2k compute on row 0's addresses, store nothing and enter the
// butterflies as +0.
// Above 32 columns the row is produced in two halves, each in its own pass
// over l: an fp64 fma addresses the 256 architectural VGPRs only, and a half
// (at most 128 of them) is parked while the other is produced.
// Two kernels per form, for np <= 32 and np <= 64: the first lets two waves
// share a SIMD.  A matrix's chunks leave the queue from the last down (the
// subsets with the high pairs set cost the most); partials keep their index.
// Resource report: profiles/hafnian_pt/walk_hafpt_resources.log.
#include "cx.hpp"
#include "hafnian_pt.hpp"
#include "hafpt.hpp"
#include "walk_common.hpp"

namespace sup {

constexpr int kPtBlock = 64;

#define PT_KARG(field) karg_at<decltype(PtParams::field)>((uint32_t)__builtin_offsetof(PtParams, field))

typedef const __attribute__((address_space(4))) dbl8 pt_cdbl8;

__device__ __forceinline__ cx pt_ld(const double* p, uint32_t pair) { return cx{p[2 * pair], p[2 * pair + 1]}; }
__device__ __forceinline__ void pt_st(double* p, uint32_t pair, cx v) {
  p[2 * pair] = v.re;
  p[2 * pair + 1] = v.im;
}

// 64-lane pairwise sum of re and im (ascending xor offsets).
__device__ __forceinline__ cx pt_wave_sum(cx v) {
#pragma unroll
  for (int off = 1; off <= 32; off <<= 1) {
    const cx o{__shfl_xor(v.re, off, 64), __shfl_xor(v.im, off, 64)};
    v = cx_add(v, o);
  }
  return v;
}

// s + the sum over the rows l of z in [OFF, OFF + H), ascending, of
// cur[l - OFF] T[l ^ 1][i1] (i1 = i ^ 1).
template <int OFF, int H>
__device__ __forceinline__ cx pt_trace(cx s, const cx (&cur)[H], const double* tile, uint32_t np, uint32_t i1,
                                       uint32_t z) {
#pragma unroll
  for (int c = 0; c < H; c += 2) {
    if ((z >> ((OFF + c) >> 1)) & 1u) {  // wave-uniform
      s = cx_fma(cur[c], pt_ld(tile, (uint32_t)(OFF + c + 1) * np + i1), s);
      s = cx_fma(cur[c + 1], pt_ld(tile, (uint32_t)(OFF + c) * np + i1), s);
    }
  }
  return s;
}

// cur[c - OFF] = sum over the rows l of z, ascending, of T[l][li] C[l][c], c in
// [OFF, OFF + H): one ds_read_b128 and H / 4 scalar loads of 64 bytes per l.
template <int OFF, int H>
__device__ __forceinline__ void pt_power(cx (&cur)[H], const double* tile, const double* tab, uint32_t np, uint32_t NP,
                                         uint32_t li, uint32_t z) {
#pragma unroll
  for (int c = 0; c < H; ++c) cur[c] = cx{0.0, 0.0};
  for (uint32_t zz = z; zz; zz &= zz - 1u) {
    const uint32_t b = (uint32_t)__builtin_ctz(zz);
#pragma unroll
    for (uint32_t h = 0; h < 2u; ++h) {
      const uint32_t l = 2u * b + h;
      const cx p = pt_ld(tile, l * np + li);
      pt_cdbl8* row = (pt_cdbl8*)opaque_c(tab, l * NP * 16u + (uint32_t)OFF * 16u);
#pragma unroll
      for (int q = 0; q < H / 4; ++q) {
        const dbl8 c8 = row[q];
#pragma unroll
        for (int e = 0; e < 4; ++e) cur[4 * q + e] = cx_fma(p, cx{c8[2 * e], c8[2 * e + 1]}, cur[4 * q + e]);
      }
    }
  }
}

template <int OFF, int H>
__device__ __forceinline__ void pt_store(const cx (&cur)[H], double* tile, uint32_t np, uint32_t li) {
#pragma unroll
  for (int c = 0; c < H; ++c)
    if ((uint32_t)(OFF + c) < np) pt_st(tile, (uint32_t)(OFF + c) * np + li, cur[c]);  // the tile has np rows, not NP
}

// f(z).  tab: the matrix's table (wave-uniform); lds: the block's shared memory.
template <bool LOOP, int KP>
__device__ __forceinline__ cx pt_subset(uint32_t z, const double* tab, uint32_t np, uint32_t m, const double* coef,
                                        double* lds) {
  const uint32_t lane = threadIdx.x;
  const uint32_t NP = (np + 7u) & ~7u;
  const uint32_t R = 2u * (uint32_t)__builtin_popcount(z);
  const bool active = lane < R;
  uint32_t ri = 0;  // the lane's actual row (row 0's for the lanes past 2k)
  {
    uint32_t cnt = 0;
    for (uint32_t zz = z; zz; zz &= zz - 1u, ++cnt)
      if (cnt == (lane >> 1) && active) ri = 2u * (uint32_t)__builtin_ctz(zz) + (lane & 1u);
  }
  const uint32_t li = active ? lane : 0u, li1 = li ^ 1u;
  double* tile = lds;
  double* yv = lds + 2 * (size_t)np * np;
  double* xs = yv + 2 * 64;
  double* jc = xs + 2 * (kPtMaxM + 1);
  double* gs = jc + 2 * (kPtMaxM + 1);
  const double* crow = tab + 2 * (size_t)ri * NP;  // the lane's own row of C
  const cx zero{0.0, 0.0};

  if constexpr (LOOP) {
    const double* dv = tab + 2 * (size_t)np * NP;
    cx y = pt_ld(dv, ri);
    const cx dsw = pt_ld(dv, ri ^ 1u);
    for (uint32_t j = 1; j <= m; ++j) {
      const cx x = pt_wave_sum(active ? cx_mul(dsw, y) : zero);
      pt_st(xs, j, x);
      if (j < m) {
        if (active) pt_st(yv, ri, y);
        __syncthreads();
        cx acc{0.0, 0.0};
#pragma unroll
        for (int c = 0; c < KP; c += 2) {
          if ((z >> (c >> 1)) & 1u) {
            acc = cx_fma(pt_ld(crow, (uint32_t)c), pt_ld(yv, (uint32_t)c), acc);
            acc = cx_fma(pt_ld(crow, (uint32_t)c + 1u), pt_ld(yv, (uint32_t)c + 1u), acc);
          }
        }
        __syncthreads();
        y = acc;
      }
    }
  }

  // c_j and jc_j of trace j
  auto emit = [&](uint32_t j, cx term) {
    const cx t = pt_wave_sum(active ? term : zero);
    const cx x = LOOP ? pt_ld(xs, j) : zero;
    const cx c = hafpt_cj(t, x, coef[j], LOOP);
    pt_st(jc, j, hafpt_scale((double)j, c));
  };

  // the row in two halves when KP > 32: a half is at most 128 registers, and
  // the half not being produced is only parked (the fmas cannot address the
  // upper half of the register file)
  constexpr bool TWO = KP > 32;
  constexpr int H = TWO ? KP / 2 : KP, H2 = TWO ? KP / 2 : 2, OFF2 = TWO ? KP / 2 : 0;
  cx lo[H], hi[H2];
  auto trace = [&]() {
    cx s = pt_trace<0, H>(zero, lo, tile, np, li1, z);
    if constexpr (TWO) s = pt_trace<OFF2, H2>(s, hi, tile, np, li1, z);
    return s;
  };
  auto store = [&]() {
    __syncthreads();
    if (active) {
      pt_store<0, H>(lo, tile, np, li);
      if constexpr (TWO) pt_store<OFF2, H2>(hi, tile, np, li);
    }
    __syncthreads();
  };
#pragma unroll
  for (int c = 0; c < H; ++c) lo[c] = pt_ld(crow, (uint32_t)c);
  if constexpr (TWO) {
#pragma unroll
    for (int c = 0; c < H2; ++c) hi[c] = pt_ld(crow, (uint32_t)(OFF2 + c));
  }
  emit(1u, pt_ld(crow, ri));
  if (m >= 2u) {
    store();
    emit(2u, trace());
  }
  const uint32_t A = (m + 1u) >> 1;
  for (uint32_t a = 2; a <= A; ++a) {
    pt_power<0, H>(lo, tile, tab, np, NP, li, z);
    if constexpr (TWO) pt_power<OFF2, H2>(hi, tile, tab, np, NP, li, z);
    emit(2u * a - 1u, trace());
    if (2u * a <= m) {
      store();
      emit(2u * a, trace());
    }
  }
  __syncthreads();

  // g_s: every lane the same values through its own LDS writes
  pt_st(gs, 0u, cx{1.0, 0.0});
  const double* invs = coef + (kPtMaxM + 1);
  for (uint32_t s = 1; s <= m; ++s) {
    cx acc{0.0, 0.0};
    for (uint32_t j = 1; j <= s; ++j) acc = cx_fma(pt_ld(jc, j), pt_ld(gs, s - j), acc);
    pt_st(gs, s, hafpt_scale(invs[s], acc));
  }
  const cx f = pt_ld(gs, m);
  __syncthreads();
  return f;
}

template <bool LOOP, int NPMAX>
__device__ __forceinline__ cx pt_dispatch(uint32_t z, const double* tab, uint32_t np, uint32_t m, const double* coef,
                                          double* lds) {
  const uint32_t kp = (uint32_t)hafpt_kpad(z);
  if constexpr (NPMAX > 32) {
    switch (kp) {
      case 40: return pt_subset<LOOP, 40>(z, tab, np, m, coef, lds);
      case 48: return pt_subset<LOOP, 48>(z, tab, np, m, coef, lds);
      case 56: return pt_subset<LOOP, 56>(z, tab, np, m, coef, lds);
      case 64: return pt_subset<LOOP, 64>(z, tab, np, m, coef, lds);
      default: break;
    }
  }
  switch (kp) {
    case 8: return pt_subset<LOOP, 8>(z, tab, np, m, coef, lds);
    case 16: return pt_subset<LOOP, 16>(z, tab, np, m, coef, lds);
    case 24: return pt_subset<LOOP, 24>(z, tab, np, m, coef, lds);
    default: return pt_subset<LOOP, 32>(z, tab, np, m, coef, lds);
  }
}

template <bool LOOP, int NPMAX>
__global__ __launch_bounds__(kPtBlock) void walk_hafpt(PtParams) {  // arguments: PT_KARG
  extern __shared__ double pt_lds[];
  const uint32_t lane = threadIdx.x;
  const uint32_t np = PT_KARG(np), m = PT_KARG(m), llog = PT_KARG(llog), cm = PT_KARG(cm);
  for (uint32_t g = next_chunk(PT_KARG(counter)); (uint64_t)g * PT_KARG(group) < PT_KARG(chunk_count);
       g = next_chunk(PT_KARG(counter))) {
    cx keep{0.0, 0.0};  // lane j keeps the partial of chunk g * group + j
    for (uint32_t j = 0; j < PT_KARG(group); ++j) {
      const uint64_t a = (uint64_t)g * PT_KARG(group) + j;
      if (a >= PT_KARG(chunk_count)) break;
      // the queue hands a matrix's chunks out from the last down: the subsets
      // with the high pairs set are the dear ones, and they go first
      const uint32_t mat = __builtin_amdgcn_readfirstlane((uint32_t)a / cm), local = cm - 1u - ((uint32_t)a - mat * cm);
      const double* tab = PT_KARG(tabs) + (uint64_t)mat * PT_KARG(tab_doubles);
      const double* coef = PT_KARG(coef);
      const uint64_t c = PT_KARG(chunk_first) + local;
      uint64_t zlo = c << llog, zhi = (c + 1ull) << llog;
      if (zlo < PT_KARG(z_begin)) zlo = PT_KARG(z_begin);
      if (zlo == 0) zlo = 1;  // z = 0 is no subset
      if (zhi > PT_KARG(z_end)) zhi = PT_KARG(z_end);
      cx acc{0.0, 0.0};
      for (uint64_t zz = zlo; zz < zhi; ++zz) {
        const uint32_t z = __builtin_amdgcn_readfirstlane((uint32_t)zz);
        const cx f = pt_dispatch<LOOP, NPMAX>(z, tab, np, m, coef, pt_lds);
        const bool neg = ((m - (uint32_t)__builtin_popcount(z)) & 1u) != 0u;
        acc = cx_add(acc, neg ? cx_neg(f) : f);
      }
      if (lane == j) keep = acc;
    }
    const uint64_t a = (uint64_t)g * PT_KARG(group) + lane;
    if (lane < PT_KARG(group) && a < PT_KARG(chunk_count)) {
      const uint32_t mat = (uint32_t)a / cm;
      const uint64_t at = (uint64_t)mat * cm + (cm - 1u - ((uint32_t)a - mat * cm));  // the chunk's own place
      PT_KARG(chunk_out)[2 * at] = keep.re;
      PT_KARG(chunk_out)[2 * at + 1] = keep.im;
    }
  }
}

// hafpt_prepare: one block per matrix writes its table (hafpt.hpp hafpt_entry,
// the host twin's own function) from A, mu and the matrix's index list.
__global__ __launch_bounds__(256) void hafpt_prepare(const double* __restrict__ A, int Mo,
                                                     const double* __restrict__ mu,
                                                     const int32_t* __restrict__ idx, int n, int np,
                                                     uint32_t tab_doubles, double* __restrict__ tabs) {
  double* t = tabs + (uint64_t)blockIdx.x * tab_doubles;
  const int32_t* ix = idx + (uint64_t)blockIdx.x * (uint64_t)n;
  const uint32_t pairs = tab_doubles / 2u;
  for (uint32_t e = threadIdx.x; e < pairs; e += 256u) {
    const cx v = hafpt_entry(A, Mo, mu, ix, n, np, e);
    t[2 * (uint64_t)e] = v.re;
    t[2 * (uint64_t)e + 1] = v.im;
  }
}

// hafpt_fold: one thread per matrix runs fock_fold over its cm chunk partials.
__global__ __launch_bounds__(256) void hafpt_fold(const double* __restrict__ parts, uint32_t cm, uint64_t K,
                                                  double* __restrict__ out) {
  const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (k >= K) return;
  const cx v = fock_fold(parts + 2 * k * (uint64_t)cm, cm);
  out[2 * k] = v.re;
  out[2 * k + 1] = v.im;
}

static bool pt_params_ok(const PtParams& p) {
  return p.np >= 2 && p.np <= 64 && !(p.np & 1u) && p.m == p.np / 2 && hafpt_lds_bytes((int)p.np) <= 65536 &&
         p.llog == (unsigned)hafpt_chunk_log((int)p.m) && p.cm >= 1 && p.z_begin < p.z_end &&
         p.z_end <= (1ull << p.m) && p.tab_doubles == 2 * hafpt_pairs((int)p.np) && p.group >= 1 && p.group <= 64 &&
         p.chunk_count >= 1 && p.chunk_count <= 0x7fffffffull && p.chunk_count % p.cm == 0 &&
         p.chunk_first == (p.z_begin >> p.llog) &&
         p.chunk_first + p.cm == ((p.z_end + (1ull << p.llog) - 1) >> p.llog);
}

hipError_t launch_hafpt(bool loop, const PtParams& p, int grid, hipStream_t s) {
  if (!pt_params_ok(p) || grid < 1) return hipErrorInvalidValue;
  const size_t lds = hafpt_lds_bytes((int)p.np);
  if (p.np <= 32) {
    if (loop) hipLaunchKernelGGL((walk_hafpt<true, 32>), dim3(grid), dim3(kPtBlock), lds, s, p);
    else hipLaunchKernelGGL((walk_hafpt<false, 32>), dim3(grid), dim3(kPtBlock), lds, s, p);
  } else {
    if (loop) hipLaunchKernelGGL((walk_hafpt<true, 64>), dim3(grid), dim3(kPtBlock), lds, s, p);
    else hipLaunchKernelGGL((walk_hafpt<false, 64>), dim3(grid), dim3(kPtBlock), lds, s, p);
  }
  return hipGetLastError();
}

hipError_t hafpt_occupancy(bool loop, int np, int* blocks_per_cu) {
  const size_t lds = hafpt_lds_bytes(np);
  if (np <= 32)
    return loop ? hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, walk_hafpt<true, 32>, kPtBlock, lds)
                : hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, walk_hafpt<false, 32>, kPtBlock, lds);
  return loop ? hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, walk_hafpt<true, 64>, kPtBlock, lds)
              : hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, walk_hafpt<false, 64>, kPtBlock, lds);
}

hipError_t launch_hafpt_prepare(const double* A, int M, const double* mu, const int32_t* idx, int n, int np,
                                uint64_t K, uint32_t tab_doubles, double* tabs, hipStream_t s) {
  if (M < 1 || n < 1 || np < n || np > 64 || K == 0 || K > 0x7fffffffull || tab_doubles != 2 * hafpt_pairs(np))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(hafpt_prepare, dim3((unsigned)K), dim3(256), 0, s, A, M, mu, idx, n, np, tab_doubles, tabs);
  return hipGetLastError();
}

hipError_t launch_hafpt_fold(const double* parts, uint32_t cm, uint64_t K, double* out, hipStream_t s) {
  if (K == 0 || cm == 0) return hipErrorInvalidValue;
  const uint64_t blocks = (K + 255) / 256;
  if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(hafpt_fold, dim3((unsigned)blocks), dim3(256), 0, s, parts, cm, K, out);
  return hipGetLastError();
}

}  // namespace sup
