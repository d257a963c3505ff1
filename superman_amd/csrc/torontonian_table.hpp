// torontonian_table.hpp — the host side of the torontonian tables
// (torontonian_table.cpp, engine.cpp run_torontonian_table and run_mobius, the
// table launchers of walk_tor.hip and walk_ltor.hip, mobius.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/superman.h"
#include "loop_torontonian.hpp"
#include "torontonian.hpp"
#include "tortab.hpp"

namespace sup {

// sup_torontonian_table (in.gamma null) and sup_loop_torontonian_table: one
// list of n modes, out[0 .. 2^n) = raw (transform false) or the table of the
// sub-lists' torontonians.
int torontonian_table(const LtorIn& in, bool loop, int n, bool transform, const sup_opts& o, bool on_cpu, double* out,
                      TorInfo* info);
// sup_mobius_subsets: t[0 .. 2^n) in place, n in [0, 28].
int mobius_subsets(double* t, int n, const sup_opts& o, bool on_cpu);
// SUP_MOBIUS_BITS=L,K (read per call) or the compiled defaults; a shape
// mobius.hip was not compiled for: SUP_EINVAL.
int mobius_shape(int* L, int* K);

// The twins' raw tables (torontonian.cpp, loop_torontonian.cpp).
void tor_table_raw_cpu(const TorIn& in, int n, int threads, double* out);
void ltor_table_raw_cpu(const LtorIn& in, int n, int threads, double* out);

// engine.cpp: prepare, the table walk, the transform (if asked) and one
// download of 2^n doubles on device `dev`, bit-identical to the host twin.
// *kernel_ms: prepare + walk + transform; *grid: blocks of the walk launch.
int run_torontonian_table(int dev, const LtorIn& in, bool loop, int n, bool transform, int L, int K, double* out,
                          double* kernel_ms, int* grid);
// t[0 .. 2^n) up, the transform, and down again.
int run_mobius(int dev, double* t, int n, int L, int K);

// walk_tor.hip, walk_ltor.hip: p.chunk_out is the table, one list, every z.
hipError_t launch_tor_table(const TorParams& p, int grid, hipStream_t s);
hipError_t tor_table_occupancy(int n, int* blocks_per_cu);
hipError_t launch_ltor_table(const TorParams& p, int grid, hipStream_t s);
hipError_t ltor_table_occupancy(int n, int* blocks_per_cu);
// mobius.hip: every pass of the transform on stream s.
hipError_t launch_mobius(double* t, int n, int L, int K, int max_grid, hipStream_t s);

}  // namespace sup
