// cplx_fock.hip — the two small kernels around the collision-aware complex
// walk (walk_cplxf.hip) and that walk's N-range dispatch.  A slab is prepared,
// walked and folded by three launches on one stream with no host work between
// them (engine.cpp run_cplx_fock), so it comes down in one download of 16
// bytes per matrix.
//
// cplx_fock_prepare: one block per matrix writes the signed table of its K
// distinct columns (Re plane, then Im plane, +b_k at row 2k, -b_k at row
// 2k + 1, padding zero) and x(0)_j = s / 2, s = fma(t_k, b_k[j], s) for k
// ascending, from U and the index lists — the values and the order of
// cplx_fock.cpp's fock_append (built with -ffp-contract=off: that fma is the
// only one).  The grouping itself is host work.
//
// cplx_fock_fold: one thread per matrix runs fock_fold (cplx_fock.hpp, the
// host twin's own function) over the matrix's chunk partials and writes
// 2 x the sum: per(A) = 2 sum, a power-of-two scale, exact.
//
// The collision-aware one-walk minors (walk_cplxfm.hip) use the
// same prepare (side 0, tables of n rows) and a fold over n outputs per
// matrix, cplx_fock_minors_fold; their N-range dispatch is here too.
#include "cplx_fock.hpp"
#include "cx.hpp"
#include "kernels.hpp"

namespace sup {

__global__ __launch_bounds__(kBlock) void cplx_fock_prepare(const double* __restrict__ U, int C,
                                                            const int32_t* __restrict__ rows,
                                                            const int32_t* __restrict__ cols,
                                                            const int32_t* __restrict__ grp,
                                                            const FockMat* __restrict__ mats, int n,
                                                            double* __restrict__ tabs, double* __restrict__ x0s) {
  const uint64_t k = blockIdx.x;
  const int NP = pad8(n), K = (int)mats[k].K;
  const bool by_rows = mats[k].side != 0;
  const int32_t* r = rows + k * n;
  const int32_t* c = cols + k * n;
  const int32_t* g = grp + mats[k].grp;  // g[2 kk] the index value, g[2 kk + 1] its multiplicity
  // b_kk[j]: columns collapsed U[rows[j]][val_kk], rows collapsed U[val_kk][cols[j]]
  auto at = [&](int kk, int j) {
    return by_rows ? U + 2 * ((size_t)g[2 * kk] * C + (size_t)c[j]) : U + 2 * ((size_t)r[j] * C + (size_t)g[2 * kk]);
  };
  double* t = tabs + mats[k].tab;
  const size_t plane = (size_t)2 * K * NP;
  for (int e = threadIdx.x; e < K * NP; e += kBlock) {
    const int kk = e / NP, j = e - kk * NP;
    double pre = 0.0, pim = 0.0, nre = 0.0, nim = 0.0;
    if (j < n) {
      const double* v = at(kk, j);
      pre = v[0], pim = v[1], nre = -v[0], nim = -v[1];
    }
    t[(size_t)(2 * kk) * NP + j] = pre;
    t[(size_t)(2 * kk + 1) * NP + j] = nre;
    t[plane + (size_t)(2 * kk) * NP + j] = pim;
    t[plane + (size_t)(2 * kk + 1) * NP + j] = nim;
  }
  double* x0 = x0s + mats[k].x0;
  for (int j = threadIdx.x; j < NP; j += kBlock) {
    double sr = 0.0, si = 0.0;
    if (j < n)
      for (int kk = 0; kk < K; ++kk) {
        const double* v = at(kk, j);
        const double tk = (double)g[2 * kk + 1];
        sr = __builtin_fma(tk, v[0], sr);
        si = __builtin_fma(tk, v[1], si);
      }
    x0[j] = 0.5 * sr;
    x0[NP + j] = 0.5 * si;
  }
}

hipError_t launch_cplx_fock_prepare(const double* U, int C, const int32_t* rows, const int32_t* cols, const int32_t* grp,
                                    const FockMat* mats, int n, uint64_t K, double* tabs, double* x0s, hipStream_t s) {
  if (n < 1 || n > 64 || K == 0 || K > 0x7fffffffull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(cplx_fock_prepare, dim3((unsigned)K), dim3(kBlock), 0, s, U, C, rows, cols, grp, mats, n, tabs,
                     x0s);
  return hipGetLastError();
}

__global__ __launch_bounds__(kBlock) void cplx_fock_fold(const double* __restrict__ parts,
                                                         const FockMat* __restrict__ mats, uint64_t K,
                                                         double* __restrict__ out) {
  const uint64_t k = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (k >= K) return;
  const uint32_t chunk0 = mats[k].chunk0, chunks = mats[k].chunks;
  const cx v = fock_fold(parts + 2 * (uint64_t)chunk0, chunks);
  out[2 * k] = 2.0 * v.re;
  out[2 * k + 1] = 2.0 * v.im;
}

hipError_t launch_cplx_fock_fold(const double* parts, const FockMat* mats, uint64_t K, double* out, hipStream_t s) {
  if (K == 0) return hipErrorInvalidValue;
  const uint64_t blocks = (K + kBlock - 1) / kBlock;
  if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(cplx_fock_fold, dim3((unsigned)blocks), dim3(kBlock), 0, s, parts, mats, K, out);
  return hipGetLastError();
}

hipError_t launch_cplx_fock(int n, const FockParams& p, int grid, hipStream_t s) {
  if (n < 1 || n > 64) return hipErrorInvalidValue;
  return n <= 16   ? launch_cplxf_1(n, p, grid, s)
         : n <= 32 ? launch_cplxf_17(n, p, grid, s)
         : n <= 48 ? launch_cplxf_33(n, p, grid, s)
                   : launch_cplxf_49(n, p, grid, s);
}

hipError_t cplx_fock_occupancy(int n, int* blocks_per_cu) {
  if (n < 1 || n > 64) return hipErrorInvalidValue;
  return n <= 16   ? occupancy_cplxf_1(n, blocks_per_cu)
         : n <= 32 ? occupancy_cplxf_17(n, blocks_per_cu)
         : n <= 48 ? occupancy_cplxf_33(n, blocks_per_cu)
                   : occupancy_cplxf_49(n, blocks_per_cu);
}

// cplx_fock_minors_fold: the collision-aware one-walk minors (walk_cplxfm.hip)
// leave n outputs per matrix, output j's partials at 2 (n chunk0 + j chunks);
// one thread per output runs fock_fold over them and writes 2 x the sum
// (DESIGN.md §8e).
__global__ __launch_bounds__(kBlock) void cplx_fock_minors_fold(const double* __restrict__ parts,
                                                                const FockMat* __restrict__ mats, uint64_t K, int n,
                                                                double* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= K * (uint64_t)n) return;
  const uint64_t k = i / (uint64_t)n, j = i - k * (uint64_t)n;
  const uint32_t chunk0 = mats[k].chunk0, chunks = mats[k].chunks;
  const cx v = fock_fold(parts + 2 * ((uint64_t)n * chunk0 + j * chunks), chunks);
  out[2 * i] = 2.0 * v.re;
  out[2 * i + 1] = 2.0 * v.im;
}

hipError_t launch_cplx_fock_minors_fold(const double* parts, const FockMat* mats, uint64_t K, int n, double* out,
                                        hipStream_t s) {
  if (K == 0 || n < 2 || n > 32) return hipErrorInvalidValue;
  const uint64_t blocks = (K * (uint64_t)n + kBlock - 1) / kBlock;
  if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(cplx_fock_minors_fold, dim3((unsigned)blocks), dim3(kBlock), 0, s, parts, mats, K, n, out);
  return hipGetLastError();
}

hipError_t launch_cplx_fock_minors(int n, const FockParams& p, int grid, hipStream_t s) {
  if (n < 2 || n > 32) return hipErrorInvalidValue;
  return n <= 16 ? launch_cplxfm_1(n, p, grid, s) : launch_cplxfm_17(n, p, grid, s);
}

hipError_t cplx_fock_minors_occupancy(int n, int* blocks_per_cu) {
  if (n < 2 || n > 32) return hipErrorInvalidValue;
  return n <= 16 ? occupancy_cplxfm_1(n, blocks_per_cu) : occupancy_cplxfm_17(n, blocks_per_cu);
}

}  // namespace sup
