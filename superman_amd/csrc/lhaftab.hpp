// lhaftab.hpp — what the loop-hafnian table's kernels (lhaftab.hip), its host
// twin (lhaf_table.cpp) and its device runner (engine.cpp run_lhaf_table)
// share: the definition of the table, every floating operation of an entry and
// the decoding of an index.  DESIGN.md §8o.
//
// For a complex symmetric M x M matrix A (its diagonal counts pairs of copies
// of one mode), a loop weight zeta per mode (haf.hpp's convention: self-loops
// only) and dims d_0 .. d_{M-1}, the table holds, for every n with n_i < d_i,
//   t(n) = lhaf(A gathered with n_i copies of i, zeta) / sqrt(prod n_i!)
// at index x = sum_i n_i prod_{k<i} d_k (mode 0 fastest), as (re, im) pairs.
//   t[0]  = 1 + 0i exactly.
//   t[x], x > 0: p = the highest i with n_i > 0, m = n - e_p;
//         acc = zeta_p * t[m]                                  (cx_mul, zeta first)
//         for j = 0 .. p ascending with m_j > 0:
//           k   = (s[m_j] * A_pj.re, s[m_j] * A_pj.im)         one product per part
//           acc.re = fma(k.re, v.re, acc.re);  acc.re = fma(-k.im, v.im, acc.re)
//           acc.im = fma(k.re, v.im, acc.im);  acc.im = fma(k.im, v.re, acc.im)
//                 with v = t[m - e_j]
//         t[x] = (acc.re * r[n_p], acc.im * r[n_p])            one product per part
// s[k] = sqrt(k) (correctly rounded) and r[k] = 1.0 / s[k] (one IEEE division)
// are two host-made tables (lhaf_roots), handed to both paths.  Row p of A is read
// up to column p.  An entry is a pure function of earlier entries: the launch
// shape, the tiles and the thread count cannot change its bits, and a
// non-finite value reaches exactly the entries whose recurrence reads it.
//
// Slabs: slab (p, c), c = 1 .. d_p - 1, holds the S_p = prod_{i<p} d_i entries
// with n_q = 0 above p and n_p = c, at x = c S_p + y, y in [0, S_p).  It reads
// slabs (p, c-1) and (p, c-2) only (slab (p, 0) is the whole table of the modes
// below p), so its entries are independent of one another.  A mode with
// d_p = 1 has no slab.
//
// The digits of y come off by multiply and shift: for y < 2^27 and d <= 65,
// y / d = (y * ceil(2^35 / d)) >> 35 exactly (the error term y e / (d 2^35) with
// e < d stays below 2^-8 < 1/65, and the product below 2^63).
#pragma once
#include <stdint.h>

#include <cmath>

#include "cx.hpp"

namespace sup {

constexpr int kLhafTabMaxM = 64;                  // modes (include/superman.h SUP_MAX_N)
constexpr int kLhafTabMaxDim = 65;                // d_i <= 65: photon numbers 0 .. 64
constexpr uint64_t kLhafTabMaxEntries = 1ull << 27;  // include/superman.h SUP_LHAF_TABLE_MAX_ENTRIES: 2 GiB of results
constexpr int kLhafMagicShift = 35;
// The low kernel's compiled tile: entries of one work-group's LDS (64 KiB of
// complex values).  SUP_LHAF_TABLE_LOW=E forces a smaller prefix per call.
constexpr uint32_t kLhafLowTile = 4096;

// The per-mode integers both kernels take by value: kernel arguments, so every
// read of them is a scalar operand.
struct LhafModes {
  uint64_t magic[kLhafTabMaxM];  // ceil(2^35 / d_i)
  uint32_t d[kLhafTabMaxM];
  uint32_t stride[kLhafTabMaxM];  // S_i = prod_{k<i} d_k
};

// dims checked by the caller: each in [1, 65], their product at most the cap.
inline LhafModes lhaf_modes(const int32_t* dims, int M) {
  LhafModes md{};
  uint64_t S = 1;
  for (int i = 0; i < M; ++i) {
    const uint64_t d = (uint64_t)dims[i];
    md.d[i] = (uint32_t)d;
    md.magic[i] = ((1ull << kLhafMagicShift) + d - 1) / d;
    md.stride[i] = (uint32_t)S;
    S *= d;
  }
  return md;
}

// Row p of A up to column p, by value for the slab kernel.
struct LhafRow {
  double a[2 * kLhafTabMaxM];
};

SUP_CX_FN cx lhaf_tab_acc(cx acc, double sk, double are, double aim, cx v) {
  const double kre = sk * are, kim = sk * aim;
  acc.re = __builtin_fma(kre, v.re, acc.re);
  acc.re = __builtin_fma(-kim, v.im, acc.re);
  acc.im = __builtin_fma(kre, v.im, acc.im);
  acc.im = __builtin_fma(kim, v.re, acc.im);
  return acc;
}

// Entry y of slab (p, c).  Tab::load(x) gives t[x]; arow is row p of A as
// (re, im) pairs; rc = r[c].  Reads t below x = c S + y only.
template <class Tab>
SUP_CX_FN cx lhaf_tab_entry(const Tab& tab, const LhafModes& md, const double* arow, cx zeta_p, const double* s, double rc,
                            int p, uint32_t c, uint32_t S, uint32_t y) {
  const uint32_t xm = (c - 1u) * S + y;  // m = n - e_p
  cx acc = cx_mul(zeta_p, tab.load(xm));
  uint32_t rem = y;
  for (int j = 0; j < p; ++j) {
    const uint32_t q = (uint32_t)(((uint64_t)rem * md.magic[j]) >> kLhafMagicShift);
    const uint32_t dig = rem - q * md.d[j];
    rem = q;
    if (dig) acc = lhaf_tab_acc(acc, s[dig], arow[2 * j], arow[2 * j + 1], tab.load(xm - md.stride[j]));
  }
  if (c > 1u) acc = lhaf_tab_acc(acc, s[c - 1u], arow[2 * p], arow[2 * p + 1], tab.load(xm - S));
  return cx{acc.re * rc, acc.im * rc};
}

// s[k] and r[k] for k = 0 .. 64 (r[0] is never read: 0).
inline void lhaf_roots(double* s, double* r) {
  s[0] = 0.0, r[0] = 0.0;
  for (int k = 1; k < kLhafTabMaxDim; ++k) s[k] = std::sqrt((double)k), r[k] = 1.0 / s[k];
}

// How many leading modes the low kernel takes for a tile of `low` entries: the
// modes p with prod_{i<=p} d_i <= low; *count is that product (>= 1: entry 0).
inline int lhaf_low_modes(const int32_t* dims, int M, uint32_t low, uint32_t* count) {
  uint64_t prod = 1;
  int p = 0;
  while (p < M && prod * (uint64_t)dims[p] <= (uint64_t)low) prod *= (uint64_t)dims[p++];
  *count = (uint32_t)prod;
  return p;
}

}  // namespace sup
