// lhaftab.hip — the loop-hafnian table t[0 .. prod d_i) on one device
// (lhaftab.hpp states the entries and the slabs; lhaf_table.cpp's host twin
// runs the same header slab by slab).  DESIGN.md §8o.
//
// Low kernel (lhaftab_low): ONE work-group of 256 threads computes the prefix
// of the table that fits its LDS tile: every slab of the leading modes p with
// prod_{i<=p} d_i <= low, a barrier between slabs, in a tile of (re, im) pairs
// (consecutive lanes on consecutive 16-byte values: each 16-lane group of a
// b128 access covers one 256-byte bank row, no conflict).  It then stores the
// tile with consecutive lanes on consecutive entries.  The many slabs of a few
// entries each cost barriers here instead of launches.
// Slab kernel (lhaftab_slab): one launch per remaining slab (p, c) in order on
// the stream.  A thread owns one entry y of the slab: lanes are on consecutive
// addresses for t[m], for the loads at -stride_j and for the store.  The digits
// of y come off one multiply and shift each (lhaftab.hpp), as the loop over j
// uses them: nothing is kept per digit.  Row p of A, zeta_p, the dims and the
// strides are kernel arguments: scalar operands.  No LDS, no barrier.
#include <hip/hip_runtime.h>

#include "lhaf_table.hpp"

namespace sup {

namespace {

struct LhafDevTab {
  const double2* t;
  __device__ __forceinline__ cx load(uint32_t x) const {
    const double2 v = t[x];
    return cx{v.x, v.y};
  }
};

}  // namespace

__global__ __launch_bounds__(256) void lhaftab_low(const double* __restrict__ A, int M, const double* __restrict__ zeta,
                                                   const double* __restrict__ s, const double* __restrict__ r,
                                                   LhafModes md, int plow, uint32_t count, double2* __restrict__ t) {
  __shared__ double2 tile[kLhafLowTile];
  const uint32_t tid = threadIdx.x;
  if (tid == 0) tile[0] = make_double2(1.0, 0.0);
  __syncthreads();
  const LhafDevTab tab{tile};
  for (int p = 0; p < plow; ++p) {
    const uint32_t S = md.stride[p], d = md.d[p];
    const cx zp{zeta[2 * p], zeta[2 * p + 1]};
    const double* arow = A + 2 * (size_t)p * M;
    for (uint32_t c = 1; c < d; ++c) {
      const double rc = r[c];
      for (uint32_t y = tid; y < S; y += 256u) {
        const cx v = lhaf_tab_entry(tab, md, arow, zp, s, rc, p, c, S, y);
        tile[c * S + y] = make_double2(v.re, v.im);
      }
      __syncthreads();
    }
  }
  for (uint32_t x = tid; x < count; x += 256u) t[x] = tile[x];
}

__global__ __launch_bounds__(256) void lhaftab_slab(double2* __restrict__ t, LhafModes md, LhafRow row, double zre,
                                                    double zim, const double* __restrict__ s, double rc, int p, uint32_t c,
                                                    uint32_t S) {
  const uint32_t y = blockIdx.x * 256u + threadIdx.x;
  if (y >= S) return;
  const cx v = lhaf_tab_entry(LhafDevTab{t}, md, row.a, cx{zre, zim}, s, rc, p, c, S, y);
  t[c * S + y] = make_double2(v.re, v.im);
}

// Every launch of one table on stream s.  A and zeta are the host's (the rows
// and zeta_p travel as kernel arguments, and r[c] from hr); dA, dzeta, ds, dr
// their device copies and the two root tables; t the table, 16-byte aligned.
hipError_t launch_lhaf_table(const double* A, const double* zeta, const double* hr, const int32_t* dims, int M,
                             uint32_t low, const double* dA, const double* dzeta, const double* ds, const double* dr, double* t,
                             hipStream_t s, uint64_t* launches, int* grid) {
  if (!A || !zeta || !hr || !dims || M < 1 || M > kLhafTabMaxM || low < 1 || low > kLhafLowTile || !dA || !dzeta || !ds || !dr ||
      !t || ((uintptr_t)t & 15u))
    return hipErrorInvalidValue;
  const LhafModes md = lhaf_modes(dims, M);
  uint32_t count = 1;
  const int plow = lhaf_low_modes(dims, M, low, &count);
  double2* t2 = reinterpret_cast<double2*>(t);
  hipLaunchKernelGGL(lhaftab_low, dim3(1), dim3(256), 0, s, dA, M, dzeta, ds, dr, md, plow, count, t2);
  hipError_t e = hipGetLastError();
  uint64_t n = 1;
  int g = 1;
  for (int p = plow; p < M && e == hipSuccess; ++p) {
    if (dims[p] < 2) continue;
    LhafRow row{};
    for (int j = 0; j <= p; ++j) row.a[2 * j] = A[2 * ((size_t)p * M + j)], row.a[2 * j + 1] = A[2 * ((size_t)p * M + j) + 1];
    const uint32_t S = md.stride[p], blocks = (S + 255u) / 256u;
    if ((int)blocks > g) g = (int)blocks;
    for (uint32_t c = 1; c < (uint32_t)dims[p] && e == hipSuccess; ++c, ++n) {
      hipLaunchKernelGGL(lhaftab_slab, dim3(blocks), dim3(256), 0, s, t2, md, row, zeta[2 * p], zeta[2 * p + 1], ds,
                         hr[c], p, c, S);
      e = hipGetLastError();
    }
  }
  if (launches) *launches = n;
  if (grid) *grid = g;
  return e;
}

}  // namespace sup
