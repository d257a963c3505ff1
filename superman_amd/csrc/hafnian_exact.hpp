// hafnian_exact.hpp — the host side of the exact hafnians (hafnian_exact.cpp,
// engine.cpp run_hafnian_exact, walk_hafexact.hip's launchers).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/superman.h"
#include "hafexact.hpp"

namespace sup {

struct HafIn;
struct HafSlab;

// The residues of slab S (built by haf_fill_slab without host tables) on
// device `dev`: prepare (the integer tables, once), then per launch of at most
// kHafxPrimes primes the walk over the slab's queue and the per-matrix fold.
// ptab: primes.size() blocks of hafx_stride(S.prog.size()) doubles (hafexact.hpp).
// res[(k np + q) 2 + part] = the residue in [0, p_q) of matrix k's sum, np =
// primes.size(), equal to the host twin's.  *kernel_ms: every kernel of the
// call; *grid: blocks of a walk launch; *launches: walk launches.
int run_hafnian_exact(int dev, const HafSlab& S, const HafIn& in, const std::vector<double>& primes,
                      const std::vector<double>& ptab, uint64_t* res, double* kernel_ms, int* grid, int* launches);

struct HafxInfo {
  double kernel_ms = 0.0;
  int devices = 0, grid = 0;
  uint64_t terms = 0;  // sum over the matrices of T
  double ops = 0.0;    // the T-weighted mean of hafx_ops over the matrices
  int primes = 0, launches = 0;
};
// sup_hafnian_complex_exact: re[k], im[k] = the decimal strings of result k
// (in.mu null: the plain hafnian; in.loop is set from it).
int hafnian_exact(const HafIn& in, int n, uint64_t count, const sup_opts& o, bool on_cpu, std::vector<std::string>& re,
                  std::vector<std::string>& im, HafxInfo* info);

// walk_hafexact.hip
hipError_t launch_hafexact(bool loop, const HafxParams& p, int grid, hipStream_t s);
hipError_t hafexact_occupancy(bool loop, int* blocks_per_cu);
hipError_t launch_hafexact_prepare(const double* A, int M, const double* mu, const int32_t* grp, const HafMat* mats,
                                   uint64_t K, double* tabs, hipStream_t s);
// out[(k kHafxPrimes + q) 2 + part] = the plain sum of matrix k's chunk
// residues of prime q < nprimes (0 for the others).
hipError_t launch_hafexact_fold(const double* parts, const HafMat* mats, uint64_t K, uint32_t nprimes, double* out,
                                hipStream_t s);

}  // namespace sup
