// cplx_minors.hip — the prepare kernel of the one-walk minors (walk_cplxm.hip)
// and its N-range dispatch: a slab of K matrices is prepared, walked and
// folded by three launches on one stream with no host work between them
// (engine.cpp run_cplx_minors).
//
// cplx_minors_prepare writes, per matrix B (N rows, q = N - 1 columns, entry
// (j, c) read as U[rows[k N + j]][cols[k q + c]]; no B is materialised), what
// cplx_minors.cpp's minors_tables builds on the host — the same values in the
// same layout:
//   table   Re plane, then Im plane of the signed column table, each
//           2 max(q-1, 1) x NP doubles: engine bit e = column e < q - 1, +v at
//           row 2e, -v at row 2e + 1, padding zero
//   x0      2 NP doubles (re block, im block); per component nw_start's order
//           over the q columns: rs = 0.0; rs += b[j][c] for c ascending;
//           b[j][q-1] - rs / 2
// Built with -ffp-contract=off like every device file (no fma in x0).
//
// The fold is cplx_batch_fold (cplx_batch.hip) over K N "matrices" of order q:
// the partials of output (k, j) are the 2^h consecutive pairs at
// 2 ((k N + j) << h), and its scale 4(q&1) - 2 is this sum's.
#include "kernels.hpp"
#include "walk_common.hpp"

namespace sup {

// One thread per (matrix, e, j): e < E = max(q-1, 1) writes the four table
// entries of column e, row j; e == E writes x0 of row j.  j < NP.
__global__ __launch_bounds__(kBlock) void cplx_minors_prepare(CplxBatchSrc src, int n, uint64_t K, double* tabs,
                                                              double* x0s) {
  const int q = n - 1, NP = pad8(n), E = q > 1 ? q - 1 : 1;
  const uint64_t per = (uint64_t)(E + 1) * NP;
  const uint64_t tid = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (tid >= K * per) return;
  const uint64_t k = tid / per;
  const int rem = (int)(tid - k * per), e = rem / NP, j = rem - e * NP;
  const double* row = nullptr;  // U's row behind row j of matrix k
  if (j < n) row = src.U + 2 * (size_t)src.rows[k * n + j] * src.C;
  auto at = [&](int c) { return row + 2 * (size_t)src.cols[k * q + c]; };
  const size_t plane = (size_t)2 * E * NP;
  if (e < E) {
    double* t = tabs + k * 2 * plane;
    double pre = 0.0, pim = 0.0, nre = 0.0, nim = 0.0;
    if (j < n && e < q - 1) {
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
      for (int c = 0; c < q; ++c) {
        const double* v = at(c);
        rs += v[0];
        is += v[1];
      }
      const double* last = at(q - 1);
      xr = last[0] - rs / 2;
      xi = last[1] - is / 2;
    }
    x0s[k * 2 * NP + j] = xr;
    x0s[k * 2 * NP + NP + j] = xi;
  }
}

hipError_t launch_cplx_minors_prepare(const CplxBatchSrc& src, int n, uint64_t K, double* tabs, double* x0s,
                                      hipStream_t s) {
  if (n < 2 || n > 32 || K == 0 || !src.U || !src.rows || !src.cols) return hipErrorInvalidValue;
  const uint64_t threads = K * (uint64_t)(n > 2 ? n - 1 : 2) * pad8(n);
  const uint64_t blocks = (threads + kBlock - 1) / kBlock;
  if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(cplx_minors_prepare, dim3((unsigned)blocks), dim3(kBlock), 0, s, src, n, K, tabs, x0s);
  return hipGetLastError();
}

hipError_t launch_cplx_minors(int n, const WalkParams& p, int hbits, unsigned long long ostride, int grid,
                              hipStream_t s) {
  if (n < 2 || n > 32) return hipErrorInvalidValue;
  return n <= 16 ? launch_cplxm_1(n, p, hbits, ostride, grid, s) : launch_cplxm_17(n, p, hbits, ostride, grid, s);
}

hipError_t cplx_minors_occupancy(int n, int* blocks_per_cu) {
  if (n < 2 || n > 32) return hipErrorInvalidValue;
  return n <= 16 ? occupancy_cplxm_1(n, blocks_per_cu) : occupancy_cplxm_17(n, blocks_per_cu);
}

}  // namespace sup
