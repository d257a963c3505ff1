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
#include "haf_walk.hpp"
#include "kernels.hpp"
#include "walk_common.hpp"

namespace sup {

// The walk itself is haf_walk.hpp's haf_walk_queue, shared with the ragged
// loop-hafnian batch (walk_lhafe.hip).
template <bool LOOP>
__global__ __launch_bounds__(kBlock) void walk_haf(HafParams) {  // arguments: HAF_KARG
  haf_walk_queue<LOOP, false>();
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
