// hafnian_pt.hpp — the host side of the power-trace hafnians (hafnian_pt.cpp,
// engine.cpp run_hafnian_pt, walk_hafpt.hip's launchers).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/superman.h"
#include "hafpt.hpp"

namespace sup {

struct HafIn;

// The device path serves padded orders whose tile (np x np pairs) and vectors
// fit one 64 KiB workgroup allocation (walk_hafpt.hip).
constexpr int kPtLdsExtraPairs = 64 + 3 * (kPtMaxM + 1);
inline size_t hafpt_lds_bytes(int np) { return 16 * ((size_t)np * (size_t)np + (size_t)kPtLdsExtraPairs); }

// One slab on device `dev`: matrices [first, first + K) of in.idx (order n,
// padded np), subsets z in [z_begin, z_end) of each.  out[2k], out[2k + 1] =
// fock_fold over matrix first + k's chunk partials, bit-identical to the host
// twin.  *kernel_ms: prepare + walk + fold; *grid: blocks of the walk launch.
int run_hafnian_pt(int dev, const HafIn& in, int n, int np, uint64_t first, uint64_t K, uint64_t z_begin,
                   uint64_t z_end, const double* coef, double* out, double* kernel_ms, int* grid);

struct PtInfo {
  double kernel_ms = 0.0;
  int devices = 0, grid = 0;
  uint64_t subsets = 0;
  double ops = 0.0;
};
// sup_hafnian_complex_pt, sup_loop_hafnian_complex_pt (range false: every z in
// [1, 2^m) of count matrices) and sup_hafnian_complex_pt_range (range true: one
// matrix, z in [max(1, z_begin), z_end)).
int hafnian_pt(const HafIn& in, int n, uint64_t count, bool range, uint64_t z_begin, uint64_t z_end,
               const sup_opts& o, bool on_cpu, double* out, PtInfo* info);
int hafnian_pt_plan(int n, int loop, uint64_t* subsets, double* est_ops);

// walk_hafpt.hip
hipError_t launch_hafpt(bool loop, const PtParams& p, int grid, hipStream_t s);
hipError_t hafpt_occupancy(bool loop, int np, int* blocks_per_cu);
// tabs + k tab_doubles = the table of matrix k (hafpt.hpp hafpt_entry) from A
// (M x M), mu (M, or null) and idx (K lists of n).
hipError_t launch_hafpt_prepare(const double* A, int M, const double* mu, const int32_t* idx, int n, int np,
                                uint64_t K, uint32_t tab_doubles, double* tabs, hipStream_t s);
// out[2k], out[2k + 1] = fock_fold over parts + 2 k cm, cm partials.
hipError_t launch_hafpt_fold(const double* parts, uint32_t cm, uint64_t K, double* out, hipStream_t s);

}  // namespace sup
