// loop_torontonian.hpp — the host side of the loop torontonians
// (loop_torontonian.cpp, engine.cpp run_loop_torontonian, walk_ltor.hip's
// launchers).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/superman.h"
#include "ltor.hpp"
#include "torontonian.hpp"

namespace sup {

// One wave's LDS in walk_ltor.hip, PM = 2 (nn - W) prefix rows at most: the
// packed strictly lower prefix factor, the prefix columns of the 2W tail rows
// and of the border row, the paused chains of the 64 >> W settings a wave
// holds ((2W + 1)(2W + 2) / 2 each: the tail block, the border's 2W
// off-diagonal chains and its diagonal chain), rho and the running product,
// the prefix rows' full indices.
inline size_t ltor_lds_bytes(int n) {
  const size_t PM = 2 * (size_t)(tor_nn(n) - kLtorW), R = 2 * kLtorW, E = (R + 1) * (R + 2) / 2, SUB = 64 >> kLtorW;
  return 16 * (PM * (PM > 0 ? PM - 1 : 0) / 2 + (R + 1) * PM + SUB * E) + 8 * (PM + (PM + 1) + SUB) + 4 * ((PM + 1) & ~(size_t)1) + 16;
}

struct LtorIn {
  const double* O = nullptr;       // 2M x 2M complex, row-major
  int M = 0;
  const double* gamma = nullptr;   // 2M complex
  const int32_t* modes = nullptr;  // count lists of n
};

// One slab on device `dev`, as run_torontonian: out[k] = Re fock_fold over
// list first + k's chunk partials, bit-identical to the host twin.
int run_loop_torontonian(int dev, const LtorIn& in, int n, uint64_t first, uint64_t K, uint64_t z_begin, uint64_t z_end,
                         double* out, double* kernel_ms, int* grid);
// out[i] = ltor_exp(x[i]) on device `dev` (the test harness' helper).
int run_ltor_exp(int dev, const double* x, uint64_t count, double* out);

// sup_loop_torontonian (range false) and sup_loop_torontonian_range (range
// true: one list, z in [z_begin, z_end)).
int loop_torontonian(const LtorIn& in, int n, uint64_t count, bool range, uint64_t z_begin, uint64_t z_end,
                     const sup_opts& o, bool on_cpu, double* out, TorInfo* info);
int loop_torontonian_plan(int n, uint64_t* subsets, double* est_ops);

// walk_ltor.hip.  p.G: ltor_g_doubles(n) doubles per list.
hipError_t launch_ltor(const TorParams& p, int grid, hipStream_t s);
hipError_t ltor_occupancy(int n, int* blocks_per_cu);
// G + k ltor_g_doubles(n) = the gathered matrix and border of list k.
hipError_t launch_ltor_prepare(const double* O, int M, const double* gamma, const int32_t* modes, int n, uint64_t K,
                               double* G, hipStream_t s);
hipError_t launch_ltor_exp(const double* x, uint64_t count, double* out, hipStream_t s);

}  // namespace sup
