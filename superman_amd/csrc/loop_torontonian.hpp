// loop_torontonian.hpp — the host side of the loop torontonians
// (loop_torontonian.cpp, engine.cpp run_loop_torontonian, walk_ltor.hip's
// launchers).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

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

// ---- the ragged batch: sup_loop_torontonian_each ----
// Item k is the loop torontonian of the list modes[k stride .. + n[k]) with row
// gamma_of[k] (null: row k) of gamma (ngamma rows of 2M complex).
struct LtorEachIn {
  const double* O = nullptr;
  int M = 0;
  const double* gamma = nullptr;
  uint64_t ngamma = 0;
  const int32_t* gamma_of = nullptr;
  const int32_t* modes = nullptr;
  int stride = 0;
  const int32_t* n = nullptr;
};
// A slab of walking items: their descriptors, their lists (stride entries
// each) and the rows [row_lo, row_lo + rows) of gamma their descriptors count from.
struct LtorEachSlab {
  std::vector<LtorItem> items;
  std::vector<int32_t> modes;
  int stride = 0, max_n = 0;
  uint64_t row_lo = 0, rows = 0, g_doubles = 0, chunks = 0;
};
// out[k] = item k: the bits of loop_torontonian on that item alone, exactly 1.0
// at n[k] = 0.  Everything is checked before any work.
int loop_torontonian_each(const LtorEachIn& in, uint64_t count, const sup_opts& o, bool on_cpu, double* out, TorInfo* info);
// The bytes an item of order n >= 1 adds to a slab and the cap a slab is filled to.
size_t ltor_item_bytes(int n, int stride);
size_t ltor_slab_cap_bytes();
// One slab on device `dev`: out[i] = item i of the slab.
int run_loop_torontonian_each(int dev, const LtorEachIn& in, const LtorEachSlab& S, double* out, double* kernel_ms, int* grid);

struct ThrInfo {
  double kernel_ms = 0.0, each_ms = 0.0, host_ms = 0.0;
  int devices = 0;
  uint64_t visited = 0, failed = 0;
  double ops = 0.0;  // the subset-weighted mean of ltor_ops over every call's items
};
// nsamples click patterns of the pure Gaussian state (B, zeta[s]) on threshold
// detectors by the chain rule with the heterodyne outcomes het
// (sup_threshold_sample; threshold_sample.cpp).
int threshold_sample(const double* B, int M, const double* zeta, const double* het, uint64_t nsamples, uint64_t sample0,
                     uint64_t seed, const sup_opts& o, bool on_cpu, int32_t* out, double* weights, ThrInfo* info);

// walk_ltor.hip.  The ragged batch's launchers.
hipError_t launch_ltore(const LtorEachParams& p, int max_n, int grid, hipStream_t s);
hipError_t ltore_occupancy(int max_n, int* blocks_per_cu);
hipError_t launch_ltore_prepare(const double* O, int M, const double* gammas, const int32_t* modes, int stride,
                                const LtorItem* items, uint64_t K, double* G, hipStream_t s);
hipError_t launch_ltore_fold(const double* parts, const LtorItem* items, uint64_t K, double* out, hipStream_t s);

// walk_ltor.hip.  p.G: ltor_g_doubles(n) doubles per list.
hipError_t launch_ltor(const TorParams& p, int grid, hipStream_t s);
hipError_t ltor_occupancy(int n, int* blocks_per_cu);
// G + k ltor_g_doubles(n) = the gathered matrix and border of list k.
hipError_t launch_ltor_prepare(const double* O, int M, const double* gamma, const int32_t* modes, int n, uint64_t K,
                               double* G, hipStream_t s);
hipError_t launch_ltor_exp(const double* x, uint64_t count, double* out, hipStream_t s);

}  // namespace sup
