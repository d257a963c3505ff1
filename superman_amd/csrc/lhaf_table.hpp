// lhaf_table.hpp — the host side of the loop-hafnian table (lhaf_table.cpp,
// engine.cpp run_lhaf_table, lhaftab.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/superman.h"
#include "lhaftab.hpp"

namespace sup {

struct LhafTabInfo {
  uint64_t entries = 0;
  uint64_t launches = 0;  // the low kernel and one per slab above its prefix
  double ops = 0.0;       // fp64 operations per entry (an fma counts once)
  double kernel_ms = 0.0;
  int grid = 0;  // work-groups of the largest launch
  int devices = 0;
};

// sup_loop_hafnian_table: out[0 .. 2 prod dims) = the table of lhaftab.hpp;
// mu null: zeta = 0, the hafnian table.
int loop_hafnian_table(const double* A, int M, const double* mu, const int32_t* dims, const sup_opts& o, bool on_cpu,
                       double* out, LhafTabInfo* info);
// sup_loop_hafnian_table_plan: entries (saturating at 2^64 - 1), launches of
// the device path and operations per entry; reads SUP_LHAF_TABLE_LOW.
int loop_hafnian_table_plan(const int32_t* dims, int M, uint64_t* entries, uint64_t* launches, double* ops_per_entry);

// engine.cpp: A, zeta and the root tables go up, the low kernel and the slab
// launches run on the context's stream, and one download brings the table
// into out, bit-identical to the host twin.  zeta is never null here.
int run_lhaf_table(int dev, const double* A, int M, const double* zeta, const int32_t* dims, uint64_t entries, uint32_t low,
                   double* out, double* kernel_ms, int* grid, uint64_t* launches);

// lhaftab.hip: every launch of one table on stream s.
hipError_t launch_lhaf_table(const double* A, const double* zeta, const double* hr, const int32_t* dims, int M,
                             uint32_t low, const double* dA, const double* dzeta, const double* ds, const double* dr, double* t,
                             hipStream_t s, uint64_t* launches, int* grid);

}  // namespace sup
