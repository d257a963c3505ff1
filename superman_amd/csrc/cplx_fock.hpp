// cplx_fock.hpp — what the collision-aware complex walk (walk_cplxf.hip), its
// host twin and slab builder (cplx_fock.cpp) and its device runner
// (engine.cpp run_cplx_fock) share: the descriptors of a slab of matrices and
// the fold of one matrix's chunk partials.  DESIGN.md §8c states the sum.
//
// A slab is a set of pools plus one descriptor per matrix and per wave-chunk:
//   tabs   per matrix the signed table of its K distinct columns b_0..b_K-1
//          (Re plane, then Im plane, each 2K x NP doubles: +b_k at row 2k,
//          -b_k at row 2k + 1, padding zero)
//   x0s    per matrix 2 NP doubles (re block, im block): x at v = 0
//   prog   step programs (one per distinct walk-digit list of the slab): entry
//          t in [1, Tw) = the byte offset of the signed column step t adds
//          and the signed weight of the state it reaches; entry 0 is the
//          start state (weight +1, no column); one padding entry follows
//   dig    per matrix its high digits, lowest first
//   grp    per matrix the K (index value, multiplicity) pairs of its collapsed
//          side (the device writes tabs and x0s from U and these:
//          cplx_fock_prepare; the host twin writes them itself)
//   wts    (-1)^v C(t, v) for t in [0, 64), v in [0, t], row t at t (t + 1) / 2
//   mats   FockMat per matrix; chunks: FockChunk per wave-chunk of the queue
#pragma once
#include <stdint.h>

#include "cx.hpp"

namespace sup {

constexpr uint32_t kFockWalkMax = 1024;      // Tw at most: the default layout's longest walk (2^10 steps)
constexpr uint32_t kFockMaxChunks = 1u << 24;  // wave-chunks of one matrix at most
constexpr int kFockFoldStack = 25;           // levels of the fold over kFockMaxChunks partials

struct FockStep {
  uint32_t off;  // byte offset of the signed column in the Re plane
  uint32_t pad_;
  double w;      // (-1)^(sum of walk digits) x prod C(t'_k, v_k) over the walk digits, after the step
};

struct FockDigit {
  uint32_t radix;    // t'_k + 1
  uint32_t col_off;  // byte offset of +b_k in the Re plane
  uint32_t wt_off;   // wts index of (-1)^0 C(t'_k, 0)
  uint32_t pad_;
};

struct FockMat {
  uint64_t tab;     // tabs index of the table
  uint64_t x0;      // x0s index of the start vector
  uint32_t prog;    // prog index of entry 0
  uint32_t dig;     // dig index of the first high digit
  uint32_t Tw;      // states each lane walks
  uint32_t ndig;    // high digits
  uint32_t H;       // valid values of h = 64 chunk + lane
  uint32_t im_off;  // bytes from the Re plane to the Im plane
  uint32_t chunk0;  // the matrix's first wave-chunk in the slab's queue and partials
  uint32_t chunks;  // ceil(H / 64)
  // what cplx_fock_prepare needs to write the table and x(0) from U
  uint32_t K;       // distinct columns
  uint32_t side;    // 0: the columns are collapsed, 1: the rows (transposed gather)
  uint32_t grp;     // grp index of the K (index value, multiplicity) pairs
  uint32_t pad_;
};

struct FockChunk {
  uint32_t mat;    // slab index of the matrix
  uint32_t local;  // chunk of that matrix
};

struct FockParams {
  const double* tabs;
  const double* x0s;
  const FockStep* prog;
  const FockDigit* dig;
  const double* wts;
  const FockMat* mats;
  const FockChunk* chunks;
  unsigned long long chunk_count;
  double* chunk_out;      // 2 doubles (re, im) per wave-chunk
  unsigned int* counter;  // queue head (zeroed before launch)
  unsigned int group;     // chunks per ticket (1..64)
  unsigned int pad_;
};

// The project's pairwise tree over `count` (re, im) partials at src (lower
// index first in every add, an odd last element moves up as it is), as a
// binary counter of finished subtrees: st[l] holds a subtree of 2^l partials
// waiting for its right sibling; at the end the waiting subtrees are joined
// from the smallest up, which is where the level-by-level tree joins them.
// count in [1, 2^24].
SUP_CX_FN cx fock_fold(const double* src, uint32_t count) {
  cx st[kFockFoldStack];
#pragma unroll
  for (int l = 0; l < kFockFoldStack; ++l) st[l] = cx{0.0, 0.0};
  for (uint32_t i = 0; i < count; ++i) {
    cx c{src[2 * (uint64_t)i], src[2 * (uint64_t)i + 1]};
    bool placed = false;
#pragma unroll
    for (int l = 0; l < kFockFoldStack; ++l) {
      if (!placed) {
        if ((i >> l) & 1u) {
          c = cx_add(st[l], c);
        } else {
          st[l] = c;
          placed = true;
        }
      }
    }
  }
  cx r{0.0, 0.0};
  bool have = false;
#pragma unroll
  for (int l = 0; l < kFockFoldStack; ++l) {
    if ((count >> l) & 1u) {
      r = have ? cx_add(st[l], r) : st[l];
      have = true;
    }
  }
  return r;
}

}  // namespace sup
