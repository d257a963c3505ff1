// walk_lhafe.hip — the ragged loop-hafnian batch for gfx950
// (sup_loop_hafnian_complex_each; hafnian.cpp).
//
// One slab holds loop hafnians of one matrix A whose orders differ and whose
// displacement vectors differ: the items of one chain-rule step of the PNR
// Gaussian boson sampler (gbs.cpp).  The walk is walk_haf.hip's, operation for
// operation (haf_walk.hpp haf_walk_queue), with three values taken per matrix
// instead of per launch: the order n, the Horner bound m = n / 2 with the odd-n
// final multiply, and the coefficient row 1 / (j! (n - 2j)!).  HafMat::ord
// carries n and the row's offset in the pool HafParams::coef points at; both are
// scalar loads at the start of a wave-chunk, so wave-chunks of different order
// sit next to each other in one queue and no register is indexed dynamically.
// Item k so has the bits of walk_haf<true> on that item alone.
// lhafe_prepare is haf_prepare with the item's own mu row.  The fold is
// walk_haf.hip's haf_fold (div = 1).
// Resource report: profiles/gbs/walk_lhafe_resources.log.
#include "cx.hpp"
#include "haf.hpp"
#include "haf_walk.hpp"
#include "kernels.hpp"
#include "walk_common.hpp"

namespace sup {

__global__ __launch_bounds__(kBlock) void walk_lhafe(HafParams) {  // arguments: HAF_KARG
  haf_walk_queue<true, true>();
}

// One block per matrix writes its table (haf.hpp haf_entry) from A, row
// mu_row[matrix] of mus (M complex each) and the recorded groups.
__global__ __launch_bounds__(kBlock) void lhafe_prepare(const double* __restrict__ A, int Mo,
                                                        const double* __restrict__ mus,
                                                        const int32_t* __restrict__ mu_row,
                                                        const int32_t* __restrict__ grp,
                                                        const HafMat* __restrict__ mats, double* __restrict__ tabs) {
  const HafMat M = mats[blockIdx.x];
  const double* mu = mus + 2 * (uint64_t)Mo * (uint64_t)mu_row[blockIdx.x];
  double* t = tabs + M.tab;
  const int32_t* g = grp + M.grp;
  for (uint32_t e = threadIdx.x; e < M.pairs; e += kBlock) {
    const cx v = haf_entry(A, Mo, mu, g, (int)M.K, (int)M.W, (int)M.ndig, e);
    t[2 * (uint64_t)e] = v.re;
    t[2 * (uint64_t)e + 1] = v.im;
  }
}

hipError_t launch_lhafe(const HafParams& p, int grid, hipStream_t s) {
  if (!p.coef || grid < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(walk_lhafe, dim3(grid), dim3(kBlock), 0, s, p);
  return hipGetLastError();
}

hipError_t lhafe_occupancy(int* blocks_per_cu) {
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, walk_lhafe, kBlock, 0);
}

hipError_t launch_lhafe_prepare(const double* A, int M, const double* mus, const int32_t* mu_row, const int32_t* grp,
                                const HafMat* mats, uint64_t K, double* tabs, hipStream_t s) {
  if (M < 1 || !mus || !mu_row || K == 0 || K > 0x7fffffffull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(lhafe_prepare, dim3((unsigned)K), dim3(kBlock), 0, s, A, M, mus, mu_row, grp, mats, tabs);
  return hipGetLastError();
}

}  // namespace sup
