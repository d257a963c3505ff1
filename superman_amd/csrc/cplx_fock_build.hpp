// cplx_fock_build.hpp — the host-side grouping, layout and slab building of the
// collision-aware complex walks, shared by cplx_fock.cpp (square matrices,
// either side collapsed) and cplx_fock_minors.cpp (n x (n-1) matrices, the
// column side collapsed).  DESIGN.md §8c states the layout rule; it is a pure
// function of the collapsed side's multiplicity vector.
#pragma once
#include <algorithm>
#include <map>
#include <thread>
#include <vector>

#include "engine.hpp"

namespace sup {

// Fixed-size (n <= 64) so that planning a matrix allocates nothing: a call
// plans 10^4..10^7 of them.
struct FockGroups {
  int K = 0;
  int32_t val[SUP_MAX_N];  // distinct indices, order of first appearance
  int mult[SUP_MAX_N];
};

struct FockLayout {
  int nd = 0;                  // digits: the groups with t' >= 1, lowest first
  uint32_t radix[SUP_MAX_N];
  int col[SUP_MAX_N];          // the group of each digit
  int nwalk = 0;               // walk digits: digits [0, nwalk)
  uint32_t Tw = 1;
  uint64_t H = 1, T = 1;
};

// The distinct values of idx[0..n) with their multiplicities.
FockGroups fock_group_of(const int32_t* idx, int n);
// The digits, walk digits, Tw, H and T of a multiplicity vector (one copy of
// the group with the smallest multiplicity held, the first on a tie).
FockLayout fock_layout(const FockGroups& g);

using FockProgs = std::map<std::vector<uint32_t>, uint32_t>;

// Completes M (step program, high digits, H, its wave-chunks in the queue) for
// a matrix whose tables have NP = pad8(n) doubles per row, and appends it to
// S.  progs: the slab's step programs by walk-digit list.
void fock_append_desc(FockSlab& S, FockMat M, int n, const FockLayout& l, FockProgs& progs);

// Appends a matrix with collapsed groups g (layout l) over n expanded entries
// to S; at(k, j) = the (re, im) pair of b_k[j].  host_tables: write the signed
// table and x(0) here (the host twin); the device path leaves that to
// cplx_fock_prepare, which reads the groups recorded in S.grp.
template <class At>
void fock_append_mat(FockSlab& S, int n, const FockGroups& g, const FockLayout& l, int side, FockProgs& progs,
                     bool host_tables, const At& at) {
  const int NP = pad8(n), K = g.K;
  FockMat M{};
  M.tab = S.tab_doubles;
  M.x0 = S.x0_doubles;
  M.im_off = (uint32_t)(2 * K * NP * 8);
  M.K = (uint32_t)K;
  M.side = (uint32_t)side;
  M.grp = (uint32_t)S.grp.size();
  for (int kk = 0; kk < K; ++kk) S.grp.push_back(g.val[kk]), S.grp.push_back(g.mult[kk]);
  const size_t plane = (size_t)2 * K * NP;
  S.tab_doubles += 2 * plane;
  S.x0_doubles += 2 * (size_t)NP;
  if (host_tables) {
    S.tabs.resize(S.tab_doubles, 0.0);
    S.x0s.resize(S.x0_doubles, 0.0);
    double* t = S.tabs.data() + M.tab;
    double* x0 = S.x0s.data() + M.x0;
    for (int kk = 0; kk < K; ++kk)
      for (int j = 0; j < n; ++j) {
        const double* v = at(kk, j);
        t[(size_t)(2 * kk) * NP + j] = v[0];
        t[(size_t)(2 * kk + 1) * NP + j] = -v[0];
        t[plane + (size_t)(2 * kk) * NP + j] = v[1];
        t[plane + (size_t)(2 * kk + 1) * NP + j] = -v[1];
      }
    // x(0)_j = 1/2 sum_k t_k b_k[j]: s = fma(t_k, b, s) for k ascending, then s / 2
    for (int j = 0; j < n; ++j) {
      double sr = 0.0, si = 0.0;
      for (int kk = 0; kk < K; ++kk) {
        const double* v = at(kk, j);
        sr = __builtin_fma((double)g.mult[kk], v[0], sr);
        si = __builtin_fma((double)g.mult[kk], v[1], si);
      }
      x0[j] = 0.5 * sr;
      x0[NP + j] = 0.5 * si;
    }
  }
  fock_append_desc(S, M, n, l, progs);
}

// fn(a, b) on `threads` contiguous parts of [0, count).
template <class F>
void fock_parallel(uint64_t count, int threads, F fn) {
  const int nt = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)std::max(threads, 1), count / 256 + 1));
  std::vector<std::thread> th;
  for (int w = 1; w < nt; ++w)
    th.emplace_back([&, w]() { fn(count * (uint64_t)w / (uint64_t)nt, count * (uint64_t)(w + 1) / (uint64_t)nt); });
  fn(0, count / (uint64_t)nt);
  for (auto& t : th) t.join();
}

}  // namespace sup
