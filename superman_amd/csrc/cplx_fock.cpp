// cplx_fock.cpp — collision-aware complex permanents: sup_perman_complex_fock
// and sup_perman_complex_fock_plan.
//
// Matrix k is A[j][c] = U[rows[j]][cols[c]].  Equal indices on one side make
// equal columns (or rows) of A; with the distinct columns b_0..b_K-1 of
// multiplicities t_k (order of first appearance) and one copy of the group
// with the smallest multiplicity held (the first on a tie; t'_k = t_k - 1
// there, t_k elsewhere)
//   per(A) = 2 sum_{0 <= v_k <= t'_k} (-1)^(sum v) prod_k C(t'_k, v_k) prod_j x_j(v)
//   x_j(v) = 1/2 sum_k (t_k - 2 v_k) b_k[j]
// has T = prod (t'_k + 1) terms.  per(A) = per(A^T), so the side with the
// smaller T is collapsed (columns on a tie; for the rows the gather
// transposes); the other side stays expanded.
//
// Layout — a pure function of the collapsed side's multiplicity vector: the
// digits are the groups with t'_k >= 1 in order of first appearance, radix
// t'_k + 1.  Walk digits: the longest prefix of them whose radix product Tw
// stays <= 2^10 while the other digits still number H = T / Tw >= 64 values
// (a full wave of lanes).  The remaining digits form the mixed-radix number
// h = 64 chunk + lane < H, lowest digit first.
//
// Per matrix the builder below writes what walk_cplxf.hip reads (cplx_fock.hpp)
// and the host twin reads the same arrays, running the same cx.hpp operations
// in the same order: chunk partials, fock_fold per matrix, times 2.  The result
// is a function of (U, rows[k], cols[k]) only.
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <map>
#include <new>
#include <string>
#include <thread>

#include "cplx_fock_build.hpp"
#include "cx.hpp"
#include "engine.hpp"

namespace sup {

namespace {

constexpr size_t kFockSlabCapBytes = (size_t)256 << 20;

// The side collapsed for one matrix and that side's groups and layout.
struct FockChoice {
  int side = 0;
  FockGroups g;
  FockLayout lay;
};

FockChoice fock_choose(const int32_t* rows, const int32_t* cols, int n) {
  FockChoice c, r;
  c.g = fock_group_of(cols, n);
  c.lay = fock_layout(c.g);
  r.side = 1;
  r.g = fock_group_of(rows, n);
  r.lay = fock_layout(r.g);
  return r.lay.T < c.lay.T ? r : c;
}

inline uint32_t wt_row(int t) { return (uint32_t)(t * (t + 1) / 2); }

// cx_prod4 (walk_cplxf.hip cxf_prod4): strided partials p_{j mod 4}, then (p0 p1)(p2 p3).
cx fock_prod(const cx* x, int n) {
  const cx one{1.0, 0.0};
  cx p[4] = {x[0], n > 1 ? x[1] : one, n > 2 ? x[2] : one, n > 3 ? x[3] : one};
  for (int j = 4; j < n; ++j) p[j & 3] = cx_mul(p[j & 3], x[j]);
  if (n == 1) return p[0];
  if (n == 2) return cx_mul(p[0], p[1]);
  if (n == 3) return cx_mul(cx_mul(p[0], p[1]), p[2]);
  return cx_mul(cx_mul(p[0], p[1]), cx_mul(p[2], p[3]));
}

// Bytes matrix k adds to a slab (tables, start vector, partials, descriptors).
size_t fock_bytes(int n, const FockChoice& c) {
  const size_t NP = (size_t)pad8(n), K = (size_t)c.g.K;
  const size_t chunks = (size_t)((c.lay.H + 63) / 64);
  return (4 * K * NP + 2 * NP) * sizeof(double) + chunks * (sizeof(FockChunk) + 2 * sizeof(double)) +
         (size_t)c.lay.nd * sizeof(FockDigit) + sizeof(FockMat) + 16;
}

// Appends matrix k (already chosen: c) to S.  progs: the slab's step programs
// by walk-digit list.  host_tables: write the table and x(0) here (the host
// twin); the device path leaves that to cplx_fock_prepare, which reads the
// groups recorded in S.grp.
void fock_append(FockSlab& S, const CplxBatchIn& in, int n, uint64_t k, const FockChoice& c, FockProgs& progs,
                 bool host_tables) {
  const int32_t* rows = in.rows + k * n;
  const int32_t* cols = in.cols + k * n;
  // b_k[j] as its (re, im) pair: columns collapsed, b_k[j] = U[rows[j]][val_k];
  // rows collapsed (the transposed gather), b_k[j] = U[val_k][cols[j]]
  auto at = [&](int kk, int j) {
    return c.side == 0 ? in.U + 2 * ((size_t)rows[j] * in.C + (size_t)c.g.val[kk])
                       : in.U + 2 * ((size_t)c.g.val[kk] * in.C + (size_t)cols[j]);
  };
  fock_append_mat(S, n, c.g, c.lay, c.side, progs, host_tables, at);
}

// One wave-chunk of the slab's queue, every lane, then the 64-lane xor
// butterfly (walk_cplxf.hip's order).
cx fock_chunk(const FockSlab& S, uint64_t a) {
  const FockChunk ck = S.chunks[a];
  const FockMat& M = S.mats[ck.mat];
  const int n = S.n, NP = pad8(n);
  const std::vector<double>& wts = fock_weights();
  const double* re = S.tabs.data() + M.tab;
  const double* im = re + M.im_off / 8;
  const double* x0 = S.x0s.data() + M.x0;
  const FockStep* prog = S.prog.data() + M.prog;
  cx v[64];
  std::vector<cx> x(n);
  for (uint32_t lane = 0; lane < 64; ++lane) {
    const uint32_t h = 64u * ck.local + lane;
    if (h >= M.H) {  // the device walks such a lane at h = 0 and drops its value
      v[lane] = cx{0.0, 0.0};
      continue;
    }
    for (int r = 0; r < n; ++r) x[r] = cx{x0[r], x0[NP + r]};
    uint32_t rem = h;
    double hw = 1.0;
    for (uint32_t d = 0; d < M.ndig; ++d) {
      const FockDigit& D = S.dig[M.dig + d];
      const uint32_t q = rem / D.radix, vd = rem - q * D.radix;
      rem = q;
      hw = hw * wts[D.wt_off + vd];
      const double nv = -(double)vd;
      const size_t off = D.col_off / 8;
      for (int r = 0; r < n; ++r)
        x[r] = cx{__builtin_fma(nv, re[off + r], x[r].re), __builtin_fma(nv, im[off + r], x[r].im)};
    }
    cx acc = fock_prod(x.data(), n);
    for (uint32_t t = 1; t < M.Tw; ++t) {
      const size_t off = prog[t].off / 8;
      for (int r = 0; r < n; ++r) x[r] = cx_add_d2(x[r], re[off + r], im[off + r]);
      const cx term = fock_prod(x.data(), n);
      const double mr = prog[t].w * term.re, mi = prog[t].w * term.im;
      acc = cx{acc.re + mr, acc.im + mi};
    }
    v[lane] = cx{acc.re * hw, acc.im * hw};
  }
  for (int off = 1; off <= 32; off <<= 1) {
    cx w[64];
    for (int l = 0; l < 64; ++l) w[l] = cx_add(v[l], v[l ^ off]);
    std::copy(w, w + 64, v);
  }
  return v[0];
}

// The host twin on a slab: `threads` threads share the queue's chunks, then
// each matrix's partials are folded.
void fock_cpu(const FockSlab& S, int threads, double* out) {
  const uint64_t count = S.chunks.size();
  std::vector<double> parts(2 * (size_t)count, 0.0);
  const int nt = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)std::max(threads, 1), count));
  auto work = [&](int w) {
    for (uint64_t a = (uint64_t)w; a < count; a += (uint64_t)nt) {
      const cx v = fock_chunk(S, a);
      parts[2 * a] = v.re, parts[2 * a + 1] = v.im;
    }
  };
  std::vector<std::thread> th;
  for (int w = 1; w < nt; ++w) th.emplace_back(work, w);
  work(0);
  for (auto& t : th) t.join();
  for (size_t k = 0; k < S.mats.size(); ++k) {
    const cx v = fock_fold(parts.data() + 2 * (size_t)S.mats[k].chunk0, S.mats[k].chunks);
    out[2 * k] = 2.0 * v.re;
    out[2 * k + 1] = 2.0 * v.im;
  }
}

int check_lists(const char* who, int R, int C, const int32_t* rows, const int32_t* cols, int n, uint64_t count) {
  for (uint64_t k = 0; k < count; ++k)
    for (int j = 0; j < n; ++j) {
      const int32_t r = rows[k * n + j], c = cols[k * n + j];
      if (r < 0 || r >= R || c < 0 || c >= C) {
        const bool row_bad = r < 0 || r >= R;
        set_error(std::string(who) + ": " + (row_bad ? "rows" : "cols") + "[k = " + std::to_string(k) +
                  "][position " + std::to_string(j) + "] = " + std::to_string(row_bad ? r : c) + " outside [0, " +
                  std::to_string(row_bad ? R : C) + ")");
        return SUP_EINVAL;
      }
    }
  return SUP_OK;
}

}  // namespace

FockGroups fock_group_of(const int32_t* idx, int n) {
  FockGroups g;
  for (int j = 0; j < n; ++j) {
    int k = 0;
    while (k < g.K && g.val[k] != idx[j]) ++k;
    if (k == g.K) {
      g.val[k] = idx[j];
      g.mult[k] = 0;
      ++g.K;
    }
    ++g.mult[k];
  }
  return g;
}

FockLayout fock_layout(const FockGroups& g) {
  FockLayout l;
  int held = 0;
  for (int k = 1; k < g.K; ++k)
    if (g.mult[k] < g.mult[held]) held = k;
  for (int k = 0; k < g.K; ++k) {
    const int tp = g.mult[k] - (k == held ? 1 : 0);
    if (tp < 1) continue;
    l.radix[l.nd] = (uint32_t)tp + 1u;
    l.col[l.nd] = k;
    ++l.nd;
    l.T *= (uint64_t)tp + 1u;  // <= 2^(n-1) <= 2^63
  }
  l.H = l.T;
  for (int d = 0; d < l.nd; ++d) {
    const uint32_t r = l.radix[d];
    if ((uint64_t)l.Tw * r > kFockWalkMax || l.H / r < 64) break;
    l.Tw *= r;
    l.H /= r;
    l.nwalk = d + 1;
  }
  return l;
}

void fock_append_desc(FockSlab& S, FockMat M, int n, const FockLayout& l, FockProgs& progs) {
  const int NP = pad8(n);
  const std::vector<double>& wts = fock_weights();
  // the step program of the walk digits (shared by every matrix of the slab with this list)
  static thread_local std::vector<uint32_t> key;  // reused: no allocation per matrix
  key.clear();
  for (int d = 0; d < l.nwalk; ++d) key.push_back(l.radix[d]), key.push_back((uint32_t)l.col[d]);
  auto it = progs.find(key);
  if (it == progs.end()) {
    const uint32_t base = (uint32_t)S.prog.size();
    // reflected mixed-radix Gray code of tt: a = the digits of tt, digit i
    // runs down (g = radix - 1 - a) where the number formed by the digits
    // above it is odd.  tt is counted up digit by digit (a slab of sampler
    // stages builds hundreds of programs: no division per digit and step).
    uint32_t a[SUP_MAX_N] = {0}, g[SUP_MAX_N] = {0};
    bool odd[SUP_MAX_N] = {false};
    for (uint32_t tt = 0; tt < l.Tw; ++tt) {
      FockStep s{0u, 0u, 1.0};
      if (tt > 0) {
        // digits below c wrap (the number above each of them grows by one, and
        // their reflected value stays), digit c steps: the one g that changes
        int c = 0;
        while (a[c] == l.radix[c] - 1u) a[c] = 0, odd[c] = !odd[c], ++c;
        ++a[c];
        for (int i = 0; i <= c; ++i) {
          const uint32_t v = odd[i] ? l.radix[i] - 1u - a[i] : a[i];
          if (v != g[i])  // v up: x -= b (the -b row), v down: x += b
            s.off = (uint32_t)((2 * l.col[i] + (v > g[i] ? 1 : 0)) * NP * 8);
          g[i] = v;
        }
      }
      for (int i = 0; i < l.nwalk; ++i) s.w = s.w * wts[wt_row((int)l.radix[i] - 1) + g[i]];
      S.prog.push_back(s);
    }
    S.prog.push_back(FockStep{0u, 0u, 0.0});  // padding: the walk asks for entry t + 1 ahead
    it = progs.emplace(key, base).first;
  }
  M.prog = it->second;
  M.Tw = l.Tw;
  M.dig = (uint32_t)S.dig.size();
  M.ndig = (uint32_t)(l.nd - l.nwalk);
  for (int d = l.nwalk; d < l.nd; ++d)
    S.dig.push_back(FockDigit{l.radix[d], (uint32_t)(2 * l.col[d] * NP * 8), wt_row((int)l.radix[d] - 1), 0u});
  M.H = (uint32_t)l.H;
  M.chunk0 = (uint32_t)S.chunks.size();
  M.chunks = (uint32_t)((l.H + 63) / 64);
  const uint32_t mi = (uint32_t)S.mats.size();
  for (uint32_t cidx = 0; cidx < M.chunks; ++cidx) S.chunks.push_back(FockChunk{mi, cidx});
  S.mats.push_back(M);
}

const std::vector<double>& fock_weights() {
  static const std::vector<double> w = [] {
    std::vector<double> t(wt_row(64), 0.0);
    std::vector<uint64_t> row{1};  // Pascal's triangle: C(63, 31) < 2^63
    for (int n = 0; n < 64; ++n) {
      for (int v = 0; v <= n; ++v) t[wt_row(n) + v] = (v & 1) ? -(double)row[v] : (double)row[v];
      std::vector<uint64_t> next(n + 2, 1);
      for (int v = 1; v <= n; ++v) next[v] = row[v - 1] + row[v];
      row.swap(next);
    }
    return t;
  }();
  return w;
}

int cplx_fock_plan(const int32_t* rows, const int32_t* cols, int n, uint64_t count, uint64_t* terms, int* side) {
  if (!rows || !cols) {
    set_error("sup_perman_complex_fock_plan: null index list");
    return SUP_EINVAL;
  }
  if (n < 1 || n > SUP_MAX_N) {
    set_error("n = " + std::to_string(n) + " outside [1, 64] (64-bit Gray index)");
    return SUP_EINVAL;
  }
  for (uint64_t k = 0; k < count; ++k) {
    const FockChoice c = fock_choose(rows + k * n, cols + k * n, n);
    if (terms) terms[k] = c.lay.T;
    if (side) side[k] = c.side;
  }
  return SUP_OK;
}

int cplx_perman_fock(const CplxBatchIn& in, int n, uint64_t count, const sup_opts& o, bool on_cpu, double* out,
                     FockInfo* info) {
  const char* who = "sup_perman_complex_fock";
  if (!out || !in.U || !in.rows || !in.cols) {
    set_error(std::string(who) + ": null pointer");
    return SUP_EINVAL;
  }
  if (n < 1 || n > SUP_MAX_N) {
    set_error("n = " + std::to_string(n) + " outside [1, 64] (64-bit Gray index)");
    return SUP_EINVAL;
  }
  if (o.walk_log2 < 0 || o.walk_log2 > 31) {
    set_error("walk_log2 = " + std::to_string(o.walk_log2) + " outside [0, 31] (0 = default layout)");
    return SUP_EINVAL;
  }
  if (in.R < 1 || in.C < 1) {
    set_error(std::string(who) + ": U must have at least one row and one column (R = " + std::to_string(in.R) +
              ", C = " + std::to_string(in.C) + ")");
    return SUP_EINVAL;
  }
  if (int rc = check_lists(who, in.R, in.C, in.rows, in.cols, n, count)) return rc;
  FockInfo fi;
  if (info) *info = fi;
  if (count == 0) return SUP_OK;
  // every matrix's terms before any work (planned on o.threads host threads):
  // the sum for the stats, and the cap
  const int T = std::max(o.threads, 1);
  {
    std::vector<uint64_t> sum(T, 0), bad(T, ~0ull);
    std::atomic<int> next{0};
    fock_parallel(count, T, [&](uint64_t a, uint64_t b) {
      const int w = next.fetch_add(1);
      for (uint64_t k = a; k < b; ++k) {
        const FockChoice c = fock_choose(in.rows + k * n, in.cols + k * n, n);
        if ((c.lay.H + 63) / 64 > kFockMaxChunks) bad[w] = std::min(bad[w], k);
        sum[w] += c.lay.T;
      }
    });
    const uint64_t k = *std::min_element(bad.begin(), bad.end());
    if (k != ~0ull) {
      const FockChoice c = fock_choose(in.rows + k * n, in.cols + k * n, n);
      set_error(std::string(who) + ": matrix k = " + std::to_string(k) + " has " + std::to_string(c.lay.T) +
                " terms, more than 2^40 (2^24 wave-chunks of 64 lanes x 2^10 steps)");
      return SUP_EUNSUPPORTED;
    }
    for (uint64_t v : sum) fi.terms += v;
  }
  uint64_t slab_max = ~0ull;
  if (const char* e = std::getenv("SUP_CPLX_FOCK_SLAB")) {
    const long long v = std::atoll(e);
    if (v > 0) slab_max = (uint64_t)v;
  }
  int G = 1;
  if (!on_cpu) {
    int ndev = 0;
    int rc = device_count(&ndev);
    if (rc) return rc;
    if (ndev == 0) {
      set_error(std::string("no HIP device available (") + who + " has no CPU fallback; on_cpu = 1 runs host threads)");
      return SUP_ENODEV;
    }
    if (o.device_id < 0 || o.device_id >= ndev) {
      set_error(std::string(who) + ": device_id out of range");
      return SUP_EINVAL;
    }
    G = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)std::max(1, std::min(o.gpu_num, ndev - o.device_id)), count));
  }
  std::vector<int> drc(G, SUP_OK), dgrid(G, 0);
  std::vector<double> dms(G, 0.0);
  std::vector<std::string> derr(G);  // g_err is thread_local: carry worker messages back
  // matrices [a, b) in slabs: as many as keep a slab under kFockSlabCapBytes
  // and 2^31 chunks (at least one), or SUP_CPLX_FOCK_SLAB
  auto work = [&](int g) {
    const uint64_t a = count * (uint64_t)g / (uint64_t)G, b = count * (uint64_t)(g + 1) / (uint64_t)G;
    try {
      // the matrices of a window are planned on this device's share of the
      // host threads, then appended in order until the slab is full
      const int pt = std::max(1, T / G);
      std::vector<FockChoice> win;
      for (uint64_t k = a; k < b && !drc[g];) {
        FockSlab S;
        S.n = n;
        S.first = k;
        FockProgs progs;
        size_t bytes = 0;
        const uint64_t k0 = k;
        bool full = false;
        while (k < b && k - k0 < slab_max && !full) {
          const uint64_t w0 = k, wn = std::min<uint64_t>({b - k, slab_max - (k - k0), (uint64_t)1 << 13});
          win.resize((size_t)wn);
          fock_parallel(wn, pt, [&](uint64_t x, uint64_t y) {
            for (uint64_t i = x; i < y; ++i) win[i] = fock_choose(in.rows + (w0 + i) * n, in.cols + (w0 + i) * n, n);
          });
          for (; k < w0 + wn; ++k) {
            const FockChoice& c = win[k - w0];
            const size_t add = fock_bytes(n, c);
            const uint64_t chunks = (c.lay.H + 63) / 64;
            if (k > k0 && (bytes + add > kFockSlabCapBytes || S.chunks.size() + chunks > 0x7fffffffull)) {
              full = true;
              break;
            }
            fock_append(S, in, n, k, c, progs, on_cpu);
            bytes += add;
          }
        }
        if (on_cpu) {
          fock_cpu(S, std::max(o.threads, 1), out + 2 * k0);
        } else {
          double ms = 0.0;
          drc[g] = run_cplx_fock(o.device_id + g, S, in, out + 2 * k0, &ms, &dgrid[g]);
          if (drc[g]) derr[g] = last_error();
          dms[g] += ms;
        }
      }
    } catch (const std::bad_alloc&) {
      derr[g] = "out of host memory for a slab's tables and partials";
      drc[g] = SUP_ENOMEM;
    }
  };
  std::vector<std::thread> th;
  for (int g = 1; g < G; ++g) th.emplace_back(work, g);
  work(0);
  for (auto& t : th) t.join();
  for (int g = 0; g < G; ++g)
    if (drc[g]) {
      set_error(derr[g]);
      return drc[g];
    }
  if (!on_cpu) {
    fi.kernel_ms = *std::max_element(dms.begin(), dms.end());
    fi.grid = dgrid[0];
    fi.devices = G;
  }
  if (info) *info = fi;
  return SUP_OK;
}

}  // namespace sup
