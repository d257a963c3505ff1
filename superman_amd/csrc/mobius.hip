// mobius.hip — the subset Moebius transform of a table of 2^n doubles, in place
// (tortab.hpp states the stages and their order; torontonian_table.cpp's host
// twin runs them one at a time).  DESIGN.md §8m.
//
// Low pass (mobius_low<L>): a work-group of 256 threads takes contiguous tiles
// of 2^L doubles.  Thread t holds elements t + 256 i of its tile in registers,
// so every load and store is a run of consecutive addresses over consecutive
// lanes.  Bits 0..5 of an element's index are its lane: stages 0..5 are
// cross-lane exchanges in registers.  Bits 6, 7 are its wave: stages 6 and 7
// go through LDS (the tile, 32 KiB at L = 12; consecutive lanes on consecutive doubles: no bank
// conflict by the 64-bank rule of ds_read_b64).  Bits 8.. are i: stages 8..L-1
// are the thread's own.
// High pass (mobius_high): stages [b0, b0 + kb), b0 >= 6.  A thread owns one
// column: the 2^kb values at stride 2^b0 above its base, in registers;
// consecutive lanes own consecutive addresses.  No LDS, no barrier.
#include <hip/hip_runtime.h>

#include "tortab.hpp"

namespace sup {

template <int L>
__global__ __launch_bounds__(256) void mobius_low(double* __restrict__ t, uint64_t count, int stages) {
  constexpr int E = L > 8 ? 1 << (L - 8) : 1;
  constexpr uint32_t TILE = 1u << L;
  __shared__ double s[256 * E];
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  for (uint64_t tile = blockIdx.x; tile * TILE < count; tile += gridDim.x) {
    double* base = t + tile * TILE;
    const uint64_t left = count - tile * TILE;  // count < 2^L: one short tile
    double v[E];
#pragma unroll
    for (int i = 0; i < E; ++i) {
      const uint32_t idx = tid + 256u * (uint32_t)i;
      v[i] = (idx < TILE && idx < left) ? base[idx] : 0.0;
    }
#pragma unroll
    for (int b = 0; b < 6; ++b)
      if (b < stages) {
#pragma unroll
        for (int i = 0; i < E; ++i) {
          const double o = __shfl_xor(v[i], 1 << b, 64);
          if ((lane >> b) & 1u) v[i] = mobius_sub(v[i], o);
        }
      }
#pragma unroll
    for (int b = 6; b < 8; ++b)
      if (b < L && b < stages) {  // uniform over the work-group
#pragma unroll
        for (int i = 0; i < E; ++i) s[256 * i + tid] = v[i];
        __syncthreads();
        if ((tid >> b) & 1u) {
#pragma unroll
          for (int i = 0; i < E; ++i) v[i] = mobius_sub(v[i], s[256 * i + (tid ^ (1u << b))]);
        }
        __syncthreads();
      }
#pragma unroll
    for (int b = 8; b < L; ++b)
      if (b < stages) {
#pragma unroll
        for (int i = 0; i < E; ++i)
          if ((i >> (b - 8)) & 1) v[i] = mobius_sub(v[i], v[i ^ (1 << (b - 8))]);
      }
#pragma unroll
    for (int i = 0; i < E; ++i) {
      const uint32_t idx = tid + 256u * (uint32_t)i;
      if (idx < TILE && idx < left) base[idx] = v[i];
    }
  }
}

// columns = count >> kb threads; column c: low b0 bits of c stay, the others
// move above the kb bits of the pass.
__global__ __launch_bounds__(256) void mobius_high(double* __restrict__ t, uint64_t columns, int b0, int kb) {
  constexpr int E = 1 << kMobiusPassMax;
  const uint64_t c = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (c >= columns) return;
  const uint64_t lowmask = (1ull << b0) - 1ull;
  double* base = t + ((c & lowmask) | ((c >> b0) << (b0 + kb)));
  const int m = 1 << kb;
  double v[E];
#pragma unroll
  for (int j = 0; j < E; ++j)
    if (j < m) v[j] = base[(uint64_t)j << b0];
#pragma unroll
  for (int b = 0; b < kMobiusPassMax; ++b)
    if (b < kb) {
#pragma unroll
      for (int j = 0; j < E; ++j)
        if (((j >> b) & 1) && j < m) v[j] = mobius_sub(v[j], v[j ^ (1 << b)]);
    }
#pragma unroll
  for (int j = 0; j < E; ++j)
    if (j < m) base[(uint64_t)j << b0] = v[j];
}

template <int L>
static void launch_low(double* t, uint64_t count, int stages, int grid, hipStream_t s) {
  hipLaunchKernelGGL(mobius_low<L>, dim3(grid), dim3(256), 0, s, t, count, stages);
}

// The whole transform of t[0 .. 2^n) with tile bits L and pass bits K.
hipError_t launch_mobius(double* t, int n, int L, int K, int max_grid, hipStream_t s) {
  if (!t || n < 0 || n > kTorTabMaxN || L < kMobiusTileMin || L > kMobiusTileMax || K < kMobiusPassMin ||
      K > kMobiusPassMax || max_grid < 1)
    return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  const uint64_t count = 1ull << n;
  const int stages = n < L ? n : L;
  const uint64_t tiles = (count + (1ull << L) - 1) >> L;
  const int grid = (int)(tiles < (uint64_t)max_grid ? tiles : (uint64_t)max_grid);
  switch (L) {
    case 6: launch_low<6>(t, count, stages, grid, s); break;
    case 7: launch_low<7>(t, count, stages, grid, s); break;
    case 8: launch_low<8>(t, count, stages, grid, s); break;
    case 9: launch_low<9>(t, count, stages, grid, s); break;
    case 10: launch_low<10>(t, count, stages, grid, s); break;
    case 11: launch_low<11>(t, count, stages, grid, s); break;
    default: launch_low<12>(t, count, stages, grid, s); break;
  }
  hipError_t e = hipGetLastError();
  for (int b0 = L; b0 < n && e == hipSuccess; b0 += K) {
    const int kb = n - b0 < K ? n - b0 : K;
    const uint64_t columns = count >> kb, blocks = (columns + 255) / 256;
    hipLaunchKernelGGL(mobius_high, dim3((unsigned)blocks), dim3(256), 0, s, t, columns, b0, kb);
    e = hipGetLastError();
  }
  return e;
}

}  // namespace sup
