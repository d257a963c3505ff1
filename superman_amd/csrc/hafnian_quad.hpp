// hafnian_quad.hpp — the host side of the double-double hafnians
// (hafnian_quad.cpp, engine.cpp run_hafnian_quad, walk_hafdd.hip's launchers;
// DESIGN.md §8q).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/superman.h"
#include "hafdd.hpp"

namespace sup {

struct HafIn;
struct HafInfo;

// A slab of matrices of order n as walk_hafdd.hip reads it (hafdd.hpp), built
// by hafnian_quad.cpp from haf_fill_slab's slab: the same digits, groups,
// chunks and program order, with the dd table's offsets in mats, the dd
// program and the dd coefficients.
struct HafddSlab {
  int n = 0;
  bool loop = false;
  uint64_t tab_doubles = 0;
  std::vector<double> tabs;  // filled for the host twin only: the device writes its own
  std::vector<HafddStep> prog;
  std::vector<HafDigit> dig;
  std::vector<int32_t> grp;
  std::vector<HafMat> mats;
  std::vector<FockChunk> chunks;
  std::vector<double> coef;  // loop form: 1 / (j! (n - 2j)!) as (hi, lo) pairs
  dd div{1.0, 0.0};          // m! (hafnian; exact in a dd for m <= 32); unused for the loop hafnian
};

// The dd weight triangle: (hi, lo) of (-1)^v C(t, v) at 2 (t (t + 1) / 2 + v),
// t < 64, each the exact integer (HafDigit::wt_off indexes it).
const std::vector<double>& hafdd_weights();

// Prepares, walks and folds slab S on device `dev`: out[4k .. 4k + 3] = re.hi,
// re.lo, im.hi, im.lo of the (loop) hafnian of its matrix k, bit-identical to
// the host twin.  *kernel_ms: prepare + walk + fold kernel time; *grid: blocks
// of the walk launch.
int run_hafnian_quad(int dev, const HafddSlab& S, const HafIn& in, double* out, double* kernel_ms, int* grid);

// sup_hafnian_complex_quad / sup_loop_hafnian_complex_quad (in.loop): 4 doubles
// per matrix.  Checks, their order and the messages are hafnian_complex's; n
// above SUP_HAFNIAN_QUAD_MAX_DEVICE_N with on_cpu false is SUP_EUNSUPPORTED
// before the device is looked for.
int hafnian_quad(const HafIn& in, int n, uint64_t count, const sup_opts& o, bool on_cpu, double* out, HafInfo* info);

// walk_hafdd.hip
hipError_t launch_hafdd(bool loop, const HafddParams& p, int grid, hipStream_t s);
hipError_t hafdd_occupancy(bool loop, int* blocks_per_cu);
hipError_t launch_hafdd_prepare(const double* A, int M, const double* mu, const int32_t* grp, const HafMat* mats,
                                uint64_t K, double* tabs, hipStream_t s);
// out[4k .. 4k + 3] = hafdd_finish of hafdd_fold_tree over matrix k's partials.
hipError_t launch_hafdd_fold(const double* parts, const HafMat* mats, uint64_t K, double div_hi, double div_lo,
                             bool loop, double* out, hipStream_t s);

}  // namespace sup
