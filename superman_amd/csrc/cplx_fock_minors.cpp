// cplx_fock_minors.cpp — collision-aware one-walk permanent minors:
// sup_perman_complex_fock_minors and sup_perman_complex_fock_minors_plan
// (DESIGN.md §8e).
//
// Matrix k is B[i][c] = U[rows[i]][cols[c]], n rows and q = n - 1 columns;
// minor j is B without row j.  Equal `cols` values make equal columns of B:
// with the distinct columns b_0..b_K-1 (vectors over all n rows) of
// multiplicities t_k (order of first appearance, sum q) and one copy of the
// group with the smallest multiplicity held (the first on a tie; t'_k = t_k - 1
// there, t_k elsewhere)
//   x_i(v) = 1/2 sum_k (t_k - 2 v_k) b_k[i]                                 (i < n)
//   per(minor j) = 2 sum_{0 <= v_k <= t'_k} (-1)^(sum v) prod_k C(t'_k, v_k) prod_{i != j} x_i(v)
// has T = prod (t'_k + 1) terms, and x_i(v) depends on row i only, so one walk
// serves all n minors (cxfm.hpp).  Only the column side is ever collapsed;
// repeated `rows` are only gathered.
//
// The layout is §8c's rule on the column multiplicity vector, through
// cplx_fock.cpp's own grouping, layout and step-program code
// (cplx_fock_build.hpp); the slab is a FockSlab whose tables have n rows.  The
// partials of output j of a matrix with `chunks` wave-chunks, the first at
// queue index chunk0, lie at 2 (n chunk0 + j chunks): contiguous per output,
// folded by fock_fold and scaled by 2.  The host twin below reads the same
// arrays and runs walk_cplxfm.hip's operations in its order, its threads
// sharing the slab's chunk queue: result (k, j) is a function of
// (U, rows[k], cols[k]) only.
#include <algorithm>
#include <cstdlib>
#include <new>
#include <string>
#include <thread>

#include "cplx_fock_build.hpp"
#include "cxfm.hpp"
#include "engine.hpp"

namespace sup {

namespace {

constexpr size_t kFockMinorsSlabCapBytes = (size_t)256 << 20;

struct MinorsChoice {
  FockGroups g;
  FockLayout lay;
};

MinorsChoice minors_choose(const int32_t* cols, int q) {
  MinorsChoice c;
  c.g = fock_group_of(cols, q);
  c.lay = fock_layout(c.g);
  return c;
}

// Bytes a matrix adds to a slab (tables, start vector, n partials per chunk, descriptors).
size_t minors_bytes(int n, const MinorsChoice& c) {
  const size_t NP = (size_t)pad8(n), K = (size_t)c.g.K;
  const size_t chunks = (size_t)((c.lay.H + 63) / 64);
  return (4 * K * NP + 2 * NP) * sizeof(double) + chunks * (sizeof(FockChunk) + 2 * sizeof(double) * (size_t)n) +
         (size_t)c.lay.nd * sizeof(FockDigit) + sizeof(FockMat) + 16 * (size_t)n;
}

// One wave-chunk of the slab's queue: every lane's walk, then per output the
// 64-lane xor butterfly's value (a pairwise tree, lower lane first).
template <int N>
void minors_chunk(const FockSlab& S, uint64_t a, cx* out) {
  constexpr int NP = pad8(N);
  const FockChunk ck = S.chunks[a];
  const FockMat& M = S.mats[ck.mat];
  const std::vector<double>& wts = fock_weights();
  const double* re = S.tabs.data() + M.tab;
  const double* im = re + M.im_off / 8;
  const double* x0 = S.x0s.data() + M.x0;
  const FockStep* prog = S.prog.data() + M.prog;
  static thread_local cx v[N][64];
  for (uint32_t lane = 0; lane < 64; ++lane) {
    const uint32_t h = 64u * ck.local + lane;
    if (h >= M.H) {  // the device walks such a lane at h = 0 and drops its values
      for (int r = 0; r < N; ++r) v[r][lane] = cx{0.0, 0.0};
      continue;
    }
    cx x[N], acc[N];
    for (int r = 0; r < N; ++r) x[r] = cx{x0[r], x0[NP + r]}, acc[r] = cx{0.0, 0.0};
    uint32_t rem = h;
    double hw = 1.0;
    for (uint32_t d = 0; d < M.ndig; ++d) {
      const FockDigit& D = S.dig[M.dig + d];
      const uint32_t q = rem / D.radix, vd = rem - q * D.radix;
      rem = q;
      hw = hw * wts[D.wt_off + vd];
      const double nv = -(double)vd;
      const size_t off = D.col_off / 8;
      for (int r = 0; r < N; ++r)
        x[r] = cx{__builtin_fma(nv, re[off + r], x[r].re), __builtin_fma(nv, im[off + r], x[r].im)};
    }
    cxm_accumulate<N, false>(x, acc);  // t = 0, weight +1
    for (uint32_t t = 1; t < M.Tw; ++t) {
      const size_t off = prog[t].off / 8;
      for (int r = 0; r < N; ++r) x[r] = cx_add_d2(x[r], re[off + r], im[off + r]);
      cxfm_accumulate<N>(x, prog[t].w, acc);
    }
    for (int r = 0; r < N; ++r) v[r][lane] = cx{acc[r].re * hw, acc[r].im * hw};
  }
  for (int r = 0; r < N; ++r) {
    for (int off = 1; off <= 32; off <<= 1)
      for (int l = 0; l < 64; l += 2 * off) v[r][l] = cx_add(v[r][l], v[r][l + off]);
    out[r] = v[r][0];
  }
}

typedef void (*ChunkFn)(const FockSlab&, uint64_t, cx*);
template <int N>
ChunkFn chunk_fn_rec(int n) {
  if (n == N) return &minors_chunk<N>;
  if constexpr (N < 32) return chunk_fn_rec<N + 1>(n);
  return nullptr;
}

// The host twin on a slab: `threads` threads share the queue's chunks, then
// each output's partials are folded.
void minors_cpu(const FockSlab& S, int threads, double* out) {
  const int n = S.n;
  const uint64_t count = S.chunks.size();
  const ChunkFn fn = chunk_fn_rec<2>(n);
  std::vector<double> parts(2 * (size_t)count * n, 0.0);
  const int nt = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)std::max(threads, 1), count));
  auto work = [&](int w) {
    cx res[32];
    for (uint64_t a = (uint64_t)w; a < count; a += (uint64_t)nt) {
      fn(S, a, res);
      const FockMat& M = S.mats[S.chunks[a].mat];
      for (int j = 0; j < n; ++j) {
        const size_t o = (size_t)n * M.chunk0 + (size_t)j * M.chunks + S.chunks[a].local;
        parts[2 * o] = res[j].re, parts[2 * o + 1] = res[j].im;
      }
    }
  };
  std::vector<std::thread> th;
  for (int w = 1; w < nt; ++w) th.emplace_back(work, w);
  work(0);
  for (auto& t : th) t.join();
  for (size_t k = 0; k < S.mats.size(); ++k)
    for (int j = 0; j < n; ++j) {
      const FockMat& M = S.mats[k];
      const cx v = fock_fold(parts.data() + 2 * ((size_t)n * M.chunk0 + (size_t)j * M.chunks), M.chunks);
      out[2 * (k * n + j)] = 2.0 * v.re;
      out[2 * (k * n + j) + 1] = 2.0 * v.im;
    }
}

}  // namespace

int cplx_fock_minors_plan(const int32_t* cols, int n, uint64_t count, uint64_t* terms) {
  const char* who = "sup_perman_complex_fock_minors_plan";
  if (n < 1) {
    set_error(std::string(who) + ": n = " + std::to_string(n) + " (must be >= 1)");
    return SUP_EINVAL;
  }
  if (n > 32) {
    set_error(std::string(who) + ": n = " + std::to_string(n) + " rows: more than 32 are not provided");
    return SUP_EUNSUPPORTED;
  }
  if (!terms || (!cols && n != 1)) {
    set_error(std::string(who) + ": null index list or output pointer");
    return SUP_EINVAL;
  }
  const int q = n - 1;
  for (uint64_t k = 0; k < count; ++k) terms[k] = q == 0 ? 1 : minors_choose(cols + k * q, q).lay.T;
  return SUP_OK;
}

int cplx_fock_minors(const CplxBatchIn& in, int n, uint64_t count, const sup_opts& o, bool on_cpu, double* out,
                     FockInfo* info) {
  const char* who = "sup_perman_complex_fock_minors";
  if (!out || !in.U || !in.rows || (!in.cols && n != 1)) {
    set_error(std::string(who) + ": null pointer");
    return SUP_EINVAL;
  }
  if (n < 1) {
    set_error(std::string(who) + ": n = " + std::to_string(n) + " (must be >= 1)");
    return SUP_EINVAL;
  }
  if (n > 32) {
    set_error(std::string(who) + ": n = " + std::to_string(n) + " rows: more than 32 are not provided");
    return SUP_EUNSUPPORTED;
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
  const int q = n - 1;
  for (uint64_t k = 0; k < count; ++k)
    for (int j = 0; j < n; ++j) {
      const int32_t r = in.rows[k * n + j];
      const bool row_bad = r < 0 || r >= in.R;
      const int32_t c = j < q ? in.cols[k * q + j] : 0;
      if (row_bad || c < 0 || c >= in.C) {
        set_error(std::string(who) + ": " + (row_bad ? "rows" : "cols") + "[k = " + std::to_string(k) +
                  "][position " + std::to_string(j) + "] = " + std::to_string(row_bad ? r : c) + " outside [0, " +
                  std::to_string(row_bad ? in.R : in.C) + ")");
        return SUP_EINVAL;
      }
    }
  FockInfo fi;
  if (info) *info = fi;
  if (count == 0) return SUP_OK;
  if (n == 1) {  // the one minor is the empty matrix: no walk, no device work
    for (uint64_t k = 0; k < count; ++k) out[2 * k] = 1.0, out[2 * k + 1] = 0.0;
    return SUP_OK;
  }
  uint64_t slab_max = ~0ull;
  if (const char* e = std::getenv("SUP_CPLX_FOCK_MINORS_SLAB")) {
    const long long v = std::atoll(e);
    if (v > 0) slab_max = (uint64_t)v;
  }
  const int T = std::max(o.threads, 1);
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
  std::vector<uint64_t> dterms(G, 0);
  std::vector<std::string> derr(G);  // g_err is thread_local: carry worker messages back
  // matrices [a, b) in slabs: as many as keep a slab under the byte cap and
  // 2^31 chunks (at least one), or SUP_CPLX_FOCK_MINORS_SLAB
  auto work = [&](int g) {
    const uint64_t a = count * (uint64_t)g / (uint64_t)G, b = count * (uint64_t)(g + 1) / (uint64_t)G;
    try {
      // the matrices of a window are planned on this device's share of the
      // host threads, then appended in order until the slab is full
      const int pt = std::max(1, T / G);
      std::vector<MinorsChoice> win;
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
            for (uint64_t i = x; i < y; ++i) win[i] = minors_choose(in.cols + (w0 + i) * q, q);
          });
          for (; k < w0 + wn; ++k) {
            const MinorsChoice& c = win[k - w0];
            const size_t add = minors_bytes(n, c);
            const uint64_t chunks = (c.lay.H + 63) / 64;
            if (k > k0 && (bytes + add > kFockMinorsSlabCapBytes ||
                           (S.chunks.size() + chunks) * (uint64_t)n > 0x7fffffffull)) {
              full = true;
              break;
            }
            const int32_t* rows = in.rows + k * n;
            // b_kk[i] = U[rows[i]][val_kk] as its (re, im) pair
            auto at = [&](int kk, int i) { return in.U + 2 * ((size_t)rows[i] * in.C + (size_t)c.g.val[kk]); };
            fock_append_mat(S, n, c.g, c.lay, 0, progs, on_cpu, at);
            bytes += add;
            dterms[g] += c.lay.T;
          }
        }
        if (on_cpu) {
          minors_cpu(S, T, out + 2 * k0 * n);
        } else {
          double ms = 0.0;
          drc[g] = run_cplx_fock_minors(o.device_id + g, S, in, out + 2 * k0 * n, &ms, &dgrid[g]);
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
  for (uint64_t v : dterms) fi.terms += v;
  if (!on_cpu) {
    fi.kernel_ms = *std::max_element(dms.begin(), dms.end());
    fi.grid = dgrid[0];
    fi.devices = G;
  }
  if (info) *info = fi;
  return SUP_OK;
}

}  // namespace sup
