// cplx_batch.hip — the two small kernels around the batched complex walk
// (walk_cplxb.hip) and its N-range dispatch: a slab of K matrices is prepared,
// walked and folded by three launches on one stream with no host work between
// them (engine.cpp run_cplx_batch).
//
// cplx_batch_prepare writes, per matrix, what cplx.cpp's cplx_plan builds on
// the host for walk_cplx — the same values in the same layout:
//   table   Re plane, then Im plane of the signed column table, each
//           2 max(n-1, 1) x NP doubles: engine bit e = column e, +v at row 2e,
//           -v at row 2e + 1, padding zero
//   x0      2 NP doubles (re block, im block); per component nw_start's order:
//           rs = 0.0; rs += a[j][k] for k ascending; a[j][n-1] - rs / 2
// from the slab's raw matrices or, for the submatrix form, from U and the
// slab's index lists: entry (j, c) of matrix k is read as
// U[rows[k n + j]][cols[k n + c]], the submatrix is never materialised.
// Built with -ffp-contract=off like every device file (no fma in x0).
//
// cplx_batch_fold folds each matrix's 2^h (re, im) chunk partials by the
// pairwise tree cplx.cpp's cx_pairwise runs over a power-of-two count
// (cx_add, lower index first), scales by 4(n&1) - 2 and writes 2 doubles.
#include "cx.hpp"
#include "kernels.hpp"
#include "walk_common.hpp"

namespace sup {

// One thread per (matrix, e, j): e < E = max(n-1, 1) writes the four table
// entries of column e, row j; e == E writes x0 of row j.  j < NP.
__global__ __launch_bounds__(kBlock) void cplx_batch_prepare(CplxBatchSrc src, int n, uint64_t K, double* tabs,
                                                             double* x0s) {
  const int NP = pad8(n), E = n > 1 ? n - 1 : 1;
  const uint64_t per = (uint64_t)(E + 1) * NP;
  const uint64_t tid = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (tid >= K * per) return;
  const uint64_t k = tid / per;
  const int rem = (int)(tid - k * per), e = rem / NP, j = rem - e * NP;
  // entry (r, c) of matrix k: its (re, im) pair
  const double* row = nullptr;  // row r's first entry (raw form) or U's row (submatrix form)
  if (j < n)
    row = src.U ? src.U + 2 * (size_t)src.rows[k * n + j] * src.C : src.mats + 2 * ((size_t)k * n + j) * n;
  auto at = [&](int c) { return row + 2 * (size_t)(src.U ? src.cols[k * n + c] : c); };
  const size_t plane = (size_t)2 * E * NP;
  if (e < E) {
    double* t = tabs + k * 2 * plane;
    double pre = 0.0, pim = 0.0, nre = 0.0, nim = 0.0;
    if (j < n && e < n - 1) {
      const double* v = at(e);
      pre = v[0], pim = v[1], nre = -v[0], nim = -v[1];
    }
    t[(size_t)(2 * e) * NP + j] = pre;
    t[(size_t)(2 * e + 1) * NP + j] = nre;
    t[plane + (size_t)(2 * e) * NP + j] = pim;
    t[plane + (size_t)(2 * e + 1) * NP + j] = nim;
  } else {
    double xr = 0.0, xi = 0.0;
    if (j < n) {
      double rs = 0.0, is = 0.0;
      for (int c = 0; c < n; ++c) {
        const double* v = at(c);
        rs += v[0];
        is += v[1];
      }
      const double* last = at(n - 1);
      xr = last[0] - rs / 2;
      xi = last[1] - is / 2;
    }
    x0s[k * 2 * NP + j] = xr;
    x0s[k * 2 * NP + NP + j] = xi;
  }
}

hipError_t launch_cplx_batch_prepare(const CplxBatchSrc& src, int n, uint64_t K, double* tabs, double* x0s,
                                     hipStream_t s) {
  if (n < 1 || n > 32 || K == 0) return hipErrorInvalidValue;
  const uint64_t threads = K * (uint64_t)(n > 1 ? n : 2) * pad8(n);
  const uint64_t blocks = (threads + kBlock - 1) / kBlock;
  if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(cplx_batch_prepare, dim3((unsigned)blocks), dim3(kBlock), 0, s, src, n, K, tabs, x0s);
  return hipGetLastError();
}

// The pairwise tree over the 2^sb consecutive (re, im) pairs at src, one
// thread: a binary counter of finished subtrees (st[l]: a subtree of 2^l
// values waiting for its right sibling), lower index first in every add.
constexpr int kFoldStack = 16;  // 2^24 partials per matrix at most (n <= 32, walk_log2 >= 1), 2^8 threads
__device__ __forceinline__ cx cxb_subtree(const double* src, uint32_t sb) {
  cx st[kFoldStack];
#pragma unroll
  for (int l = 0; l < kFoldStack; ++l) st[l] = cx{0.0, 0.0};
  cx c{0.0, 0.0};
  const uint32_t cnt = 1u << sb;
  for (uint32_t i = 0; i < cnt; ++i) {
    c = cx{src[2 * (size_t)i], src[2 * (size_t)i + 1]};
    bool placed = false;
#pragma unroll
    for (int l = 0; l < kFoldStack; ++l) {
      if (!placed && (uint32_t)l < sb) {
        if ((i >> l) & 1u) {
          c = cx_add(st[l], c);
        } else {
          st[l] = c;
          placed = true;
        }
      }
    }
  }
  return c;  // the last i has every bit below sb set: c went through every level
}

// A team of T = 2^min(h, 8) threads per matrix, 256 / T matrices per block:
// each thread folds its 2^(h - min(h, 8)) consecutive partials, then the team
// folds its T values through LDS (one level per pass).
__global__ __launch_bounds__(kBlock) void cplx_batch_fold(const double* __restrict__ parts, int hbits, uint64_t K,
                                                          double scale, double* __restrict__ out) {
  __shared__ double lre[kBlock], lim[kBlock];
  const uint32_t tb = hbits < 8 ? (uint32_t)hbits : 8u, T = 1u << tb, sb = (uint32_t)hbits - tb;
  const uint32_t t = threadIdx.x & (T - 1u);
  const uint64_t k = (uint64_t)blockIdx.x * (kBlock >> tb) + (threadIdx.x >> tb);
  cx v{0.0, 0.0};
  if (k < K) v = cxb_subtree(parts + 2 * ((k << hbits) + ((uint64_t)t << sb)), sb);
  lre[threadIdx.x] = v.re;
  lim[threadIdx.x] = v.im;
  for (uint32_t s = 1; s < T; s <<= 1) {  // block-uniform trip count
    __syncthreads();
    if ((t & (2u * s - 1u)) == 0) {  // reads slot t + s, which no thread writes at this level
      const cx w = cx_add(cx{lre[threadIdx.x], lim[threadIdx.x]}, cx{lre[threadIdx.x + s], lim[threadIdx.x + s]});
      lre[threadIdx.x] = w.re;
      lim[threadIdx.x] = w.im;
    }
  }
  if (t == 0 && k < K) {
    out[2 * k] = scale * lre[threadIdx.x];
    out[2 * k + 1] = scale * lim[threadIdx.x];
  }
}

hipError_t launch_cplx_batch_fold(const double* parts, int n, int hbits, uint64_t K, double* out, hipStream_t s) {
  if (hbits < 0 || hbits > 8 + kFoldStack || K == 0) return hipErrorInvalidValue;
  const uint32_t per_block = (uint32_t)kBlock >> (hbits < 8 ? hbits : 8);
  const uint64_t blocks = (K + per_block - 1) / per_block;
  if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
  const double scale = 4.0 * (n & 1) - 2.0;  // perm = (4(n&1) - 2) * total: a power-of-two scale, exact
  hipLaunchKernelGGL(cplx_batch_fold, dim3((unsigned)blocks), dim3(kBlock), 0, s, parts, hbits, K, scale, out);
  return hipGetLastError();
}

hipError_t launch_cplx_batch(int n, const WalkParams& p, int hbits, int grid, hipStream_t s) {
  if (n < 1 || n > 32) return hipErrorInvalidValue;
  return n <= 16 ? launch_cplxb_1(n, p, hbits, grid, s) : launch_cplxb_17(n, p, hbits, grid, s);
}

hipError_t cplx_batch_occupancy(int n, int* blocks_per_cu) {
  if (n < 1 || n > 32) return hipErrorInvalidValue;
  return n <= 16 ? occupancy_cplxb_1(n, blocks_per_cu) : occupancy_cplxb_17(n, blocks_per_cu);
}

}  // namespace sup
