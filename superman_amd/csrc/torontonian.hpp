// torontonian.hpp — the host side of the torontonians (torontonian.cpp,
// engine.cpp run_torontonian, walk_tor.hip's launchers).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/superman.h"
#include "tor.hpp"

namespace sup {

// One wave's LDS in walk_tor.hip, PM = 2 (nn - W) prefix rows at most: the
// packed strictly lower prefix factor, the 2W tail rows' prefix columns, the
// paused tail blocks of the 64 >> W settings a wave holds, rho and the running
// product, the prefix rows' full indices.
inline size_t tor_lds_bytes(int n) {
  const size_t PM = 2 * (size_t)(tor_nn(n) - kTorW), R = 2 * kTorW, E = (size_t)kTorW * (R + 1), SUB = 64 >> kTorW;
  return 16 * (PM * (PM > 0 ? PM - 1 : 0) / 2 + R * PM + SUB * E) + 8 * (PM + (PM + 1) + SUB) + 4 * ((PM + 1) & ~(size_t)1) + 16;
}

struct TorIn {
  const double* O = nullptr;      // 2M x 2M complex, row-major
  int M = 0;
  const int32_t* modes = nullptr;  // count lists of n
};

// One slab on device `dev`: lists [first, first + K) of in.modes, subsets z in
// [z_begin, z_end) of each.  out[k] = Re fock_fold over list first + k's chunk
// partials, bit-identical to the host twin.  *kernel_ms: prepare + walk +
// fold; *grid: blocks of the walk launch.
int run_torontonian(int dev, const TorIn& in, int n, uint64_t first, uint64_t K, uint64_t z_begin, uint64_t z_end,
                    double* out, double* kernel_ms, int* grid);

struct TorInfo {
  double kernel_ms = 0.0;
  int devices = 0, grid = 0;
  uint64_t subsets = 0;
  double ops = 0.0;
};
// sup_torontonian (range false: every z in [0, 2^n) of count lists) and
// sup_torontonian_range (range true: one list, z in [z_begin, z_end)).
int torontonian(const TorIn& in, int n, uint64_t count, bool range, uint64_t z_begin, uint64_t z_end,
                const sup_opts& o, bool on_cpu, double* out, TorInfo* info);
int torontonian_plan(int n, uint64_t* subsets, double* est_ops);

// walk_tor.hip
hipError_t launch_tor(const TorParams& p, int grid, hipStream_t s);
hipError_t tor_occupancy(int n, int* blocks_per_cu);
// G + k tor_g_doubles(n) = the gathered matrix of list k (tor.hpp tor_entry).
hipError_t launch_tor_prepare(const double* O, int M, const int32_t* modes, int n, uint64_t K, double* G, hipStream_t s);
// out[k] = Re fock_fold over parts + 2 k cm, cm partials.
hipError_t launch_tor_fold(const double* parts, uint32_t cm, uint64_t K, double* out, hipStream_t s);

}  // namespace sup
