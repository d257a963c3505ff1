// tortab.hpp — what the torontonian tables' kernels (walk_tor.hip's and
// walk_ltor.hip's table forms, mobius.hip), their host twin
// (torontonian_table.cpp) and their device runner (engine.cpp
// run_torontonian_table) share: the definition of the table and the order of
// the transform.  DESIGN.md §8m.
//
// For one list of n distinct modes (tor.hpp's positions and subsets z):
//   raw[z] = f(z), unsigned, z in [0, 2^n): tor.hpp's chains (ltor.hpp's with
//            a border), so raw[z] has the bits of the one-subset range entry
//            up to its sign (-1)^(n - |z|).
// f(z) depends on the selected positions only, so for every sub-list S
//   tor(O, S) = sum_{Z in S} (-1)^(|S| - |Z|) f(Z)
// is the subset Moebius transform of raw, in place, BITS ASCENDING:
//   for b = 0 .. n-1:  for every z with bit b set:  t[z] = t[z] - t[z ^ (1 << b)]
// One IEEE subtraction per stage and element (mobius_sub: no fma can form).
// Stage b reads only values stages < b left, so a group of elements closed
// under a set of bits may run those stages back to back: passes and tiles do
// not change the bits, the order of the stages does.  A NaN f(Z) reaches
// exactly the supersets of Z.
//
// The device's passes (mobius.hip), for tile bits L and pass bits K:
//   low pass    stages 0 .. min(L, n) - 1 on contiguous tiles of 2^L doubles;
//   high passes stages [b0, b0 + kb), kb <= K, b0 = L, L + K, ..: a thread owns
//               the 2^kb values of one column at stride 2^b0.
#pragma once
#include <stdint.h>

#include "cx.hpp"

namespace sup {

constexpr int kTorTabMaxN = 28;  // include/superman.h SUP_TORONTONIAN_TABLE_MAX_N: 2 GiB of results

// The shapes mobius.hip is compiled for, and the defaults (SUP_MOBIUS_BITS=L,K
// forces smaller ones per call).
constexpr int kMobiusTileMin = 6, kMobiusTileMax = 12;  // 2^12 doubles: 16 per thread, 32 KiB of LDS per work-group
constexpr int kMobiusPassMin = 1, kMobiusPassMax = 6;   // 2^6 doubles per thread
#ifndef SUP_MOBIUS_TILE_BITS
#define SUP_MOBIUS_TILE_BITS 12
#endif
#ifndef SUP_MOBIUS_PASS_BITS
#define SUP_MOBIUS_PASS_BITS 6
#endif
constexpr int kMobiusTileBits = SUP_MOBIUS_TILE_BITS, kMobiusPassBits = SUP_MOBIUS_PASS_BITS;
static_assert(kMobiusTileBits >= kMobiusTileMin && kMobiusTileBits <= kMobiusTileMax, "mobius.hip has no such tile");
static_assert(kMobiusPassBits >= kMobiusPassMin && kMobiusPassBits <= kMobiusPassMax, "mobius.hip has no such pass");

SUP_CX_FN double mobius_sub(double hi, double lo) { return hi - lo; }

// Passes over the table for n bits: the low pass and the high ones.
inline int mobius_passes(int n, int L, int K) { return n <= L ? 1 : 1 + (n - L + K - 1) / K; }

}  // namespace sup
