// cplx_minors.cpp — the permanents of all n minors (B without row j) of
// n x (n-1) complex matrices B from one Gray walk per matrix:
// sup_perman_complex_minors and sup_perman_complex_minors_range.  The boson
// sampler (boson.cpp) asks for exactly this per stage, and it is the gradient
// of a permanent with respect to a row.
//
// The sum, q = n - 1: the layout and enumeration of order q
// (layout_with_walk(q, o.walk_log2), engine bit e = column e, column q - 1
// held), the Nijenhuis-Wilf vector over all n rows,
//   x_i(S) = b_i,q-1 - 1/2 sum_c b_ic + sum_{e in S} b_ie
//   per(minor j) = (4(q&1) - 2) sum_S (-1)^|S| prod_{i != j} x_i(S),
// every state's n products formed by cxm.hpp's prefix/suffix chain.  The host
// twin below runs walk_cplxm.hip's operations in its order (chunk start, lane
// layout, sign pattern, 64-lane butterfly, pairwise tree over the chunk
// index), so result (k, j) is a function of (gathered B, walk bits) only:
// bit-identical on the GPU for any device count and slab size and on any
// number of host threads.  It does not have sup_perman_complex's bits on the
// materialised minor (the product order differs).
// n = 1: the one minor is the empty matrix, 1 + 0i.  n in 33..64: every minor
// materialised and run through cplx_perman (sup_perman_complex's bits).
#include <algorithm>
#include <chrono>
#include <new>
#include <string>
#include <thread>

#include "cxm.hpp"
#include "engine.hpp"

namespace sup {

namespace {

// The signed column table (Re plane, then Im plane, each 2 max(q-1, 1) x NP)
// and x0 (re block, im block) of one matrix; at(j, c) = its entry's (re, im).
template <class At>
void minors_tables(const At& at, int n, std::vector<double>& tab, std::vector<double>& x0) {
  const int q = n - 1, NP = pad8(n), E = q > 1 ? q - 1 : 1;
  const size_t plane = (size_t)2 * E * NP;
  tab.assign(2 * plane, 0.0);
  x0.assign(2 * (size_t)NP, 0.0);
  for (int j = 0; j < n; ++j) {
    for (int e = 0; e < q - 1; ++e) {
      const double* v = at(j, e);
      tab[(size_t)(2 * e) * NP + j] = v[0];
      tab[(size_t)(2 * e + 1) * NP + j] = -v[0];
      tab[plane + (size_t)(2 * e) * NP + j] = v[1];
      tab[plane + (size_t)(2 * e + 1) * NP + j] = -v[1];
    }
    double rs = 0.0, is = 0.0;
    for (int c = 0; c < q; ++c) {
      const double* v = at(j, c);
      rs += v[0];
      is += v[1];
    }
    const double* last = at(j, q - 1);
    x0[j] = last[0] - rs / 2;
    x0[NP + j] = last[1] - is / 2;
  }
}

// One wave-chunk of one matrix: every lane's walk, then per output the
// 64-lane xor butterfly's lane 0 (a pairwise tree, lower lane first).
template <int N>
void minors_chunk(const double* tab, const double* x0c, const Layout& lay, uint64_t ga, cx* out) {
  constexpr int NP = pad8(N);
  const int L = lay.L, q = N - 1;
  const size_t plane = (size_t)2 * (q > 1 ? q - 1 : 1) * NP;
  const double* re = tab;
  const double* im = tab + plane;
  const double* reL = re + (size_t)(2 * L) * NP;  // walk bit 0, + and - columns follow
  const double* imL = reL + plane;
  const uint32_t T = 1u << lay.m;
  static thread_local cx v[N][64];
  for (uint32_t lane = 0; lane < 64; ++lane) {
    if (lane >= (1u << L)) {
      for (int r = 0; r < N; ++r) v[r][lane] = cx{0.0, 0.0};
      continue;
    }
    cx x[N], acc[N];
    for (int r = 0; r < N; ++r) x[r] = cx{x0c[r], x0c[NP + r]}, acc[r] = cx{0.0, 0.0};
    uint64_t h = ga ^ (ga >> 1);
    const int hb = L + lay.m;
    while (h) {
      const int b = __builtin_ctzll(h);
      h &= h - 1;
      const size_t off = (size_t)(2 * (hb + b)) * NP;
      for (int r = 0; r < N; ++r) x[r] = cx_add_d2(x[r], re[off + r], im[off + r]);
    }
    for (int e = 0; e < L; ++e) {
      const size_t off = (size_t)(2 * e) * NP;
      const bool on = (lane >> e) & 1u;
      for (int r = 0; r < N; ++r) x[r] = cx_add_d2(x[r], on ? re[off + r] : 0.0, on ? im[off + r] : 0.0);
    }
    auto step = [&](size_t off) {
      for (int r = 0; r < N; ++r) x[r] = cx_add_d2(x[r], reL[off + r], imL[off + r]);
    };
    cxm_accumulate<N, false>(x, acc);  // t = 0
    uint32_t t = 1;
    for (; t + 1 < T; t += 2) {
      step((size_t)((t >> 1) & 1u) * NP);
      cxm_accumulate<N, true>(x, acc);
      const uint32_t u = t + 1;
      const uint32_t k = (uint32_t)__builtin_ctz(u);
      const uint32_t neg = (u >> (k + 1)) & 1u;
      step((size_t)(2u * k + neg) * NP);
      cxm_accumulate<N, false>(x, acc);
    }
    if (t < T) {
      step((size_t)((t >> 1) & 1u) * NP);
      cxm_accumulate<N, true>(x, acc);
    }
    const uint32_t lane_par = __builtin_popcount(lane) & 1u;
    const bool flip = (((uint32_t)ga ^ lane_par) & 1u) != 0;
    for (int r = 0; r < N; ++r) v[r][lane] = flip ? cx_neg(acc[r]) : acc[r];
  }
  for (int r = 0; r < N; ++r) {
    for (int off = 1; off <= 32; off <<= 1)
      for (int l = 0; l < 64; l += 2 * off) v[r][l] = cx_add(v[r][l], v[r][l + off]);
    out[r] = v[r][0];
  }
}

typedef void (*ChunkFn)(const double*, const double*, const Layout&, uint64_t, cx*);
template <int N>
ChunkFn chunk_fn_rec(int n) {
  if (n == N) return &minors_chunk<N>;
  if constexpr (N < 32) return chunk_fn_rec<N + 1>(n);
  return nullptr;
}

// cx_pairwise (cplx.cpp): the pairwise tree over `count` (re, im) pairs, an
// odd last element moves up as it is.
cx fold_pairwise(const double* parts, uint64_t count) {
  if (count == 0) return cx{0.0, 0.0};
  std::vector<cx> v(count);
  for (uint64_t a = 0; a < count; ++a) v[a] = cx{parts[2 * a], parts[2 * a + 1]};
  while (v.size() > 1) {
    std::vector<cx> w((v.size() + 1) / 2);
    for (size_t i = 0; i < w.size(); ++i) w[i] = 2 * i + 1 < v.size() ? cx_add(v[2 * i], v[2 * i + 1]) : v[2 * i];
    v.swap(w);
  }
  return v[0];
}

// Chunks [c0, c1) of one matrix on `threads` host threads: output j's partials
// at parts[2 (j (c1 - c0) + c - c0)].
void cpu_minors_range(const std::vector<double>& tab, const std::vector<double>& x0, int n, const Layout& lay,
                      uint64_t c0, uint64_t c1, int threads, double* parts) {
  if (c1 <= c0) return;
  const uint64_t count = c1 - c0;
  const ChunkFn fn = chunk_fn_rec<2>(n);
  const int nt = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)std::max(threads, 1), count));
  auto work = [&](int w) {
    cx res[32];
    for (uint64_t a = (uint64_t)w; a < count; a += (uint64_t)nt) {
      fn(tab.data(), x0.data(), lay, c0 + a, res);
      for (int j = 0; j < n; ++j) parts[2 * (j * count + a)] = res[j].re, parts[2 * (j * count + a) + 1] = res[j].im;
    }
  };
  std::vector<std::thread> th;
  for (int w = 1; w < nt; ++w) th.emplace_back(work, w);
  work(0);
  for (auto& t : th) t.join();
}

int need_device(const sup_opts& o, const char* who, int* ndev) {
  int rc = device_count(ndev);
  if (rc) return rc;
  if (*ndev == 0) {
    set_error(std::string("no HIP device available (") + who + " has no CPU fallback; on_cpu = 1 runs host threads)");
    return SUP_ENODEV;
  }
  if (o.device_id < 0 || o.device_id >= *ndev) {
    set_error(std::string(who) + ": device_id out of range");
    return SUP_EINVAL;
  }
  return SUP_OK;
}

// fn(worker, k) for k < count on up to T host threads (k strided over the
// workers); the first failure wins, with its message.
template <class Fn>
int for_matrices(uint64_t count, int T, const Fn& fn) {
  T = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)std::max(T, 1), count));
  std::vector<int> wrc(T, SUP_OK);
  std::vector<std::string> werr(T);  // g_err is thread_local: carry worker messages back
  auto work = [&](int w) {
    for (uint64_t k = (uint64_t)w; k < count && !wrc[w]; k += (uint64_t)T)
      if ((wrc[w] = fn(w, k))) werr[w] = last_error();
  };
  std::vector<std::thread> th;
  for (int w = 1; w < T; ++w) th.emplace_back(work, w);
  work(0);
  for (auto& t : th) t.join();
  for (int w = 0; w < T; ++w)
    if (wrc[w]) {
      set_error(werr[w]);
      return wrc[w];
    }
  return SUP_OK;
}

}  // namespace

int cplx_minors(const CplxBatchIn& in, int n, uint64_t count, const sup_opts& o, bool on_cpu, double* out,
                CplxInfo* info) {
  const char* who = "sup_perman_complex_minors";
  if (!out || !in.U || !in.rows || (!in.cols && n != 1)) {
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
  CplxInfo ci;
  ci.lay = layout_with_walk(std::max(q, 1), o.walk_log2);
  if (info) *info = ci;
  if (count == 0) return SUP_OK;
  if (n == 1) {
    for (uint64_t k = 0; k < count; ++k) out[2 * k] = 1.0, out[2 * k + 1] = 0.0;
    return SUP_OK;
  }
  auto entry = [&](uint64_t k, int j, int c) {
    return in.U + 2 * ((size_t)in.rows[k * n + j] * in.C + (size_t)in.cols[k * q + c]);
  };
  int ndev = 0;
  if (!on_cpu)
    if (int rc = need_device(o, who, &ndev)) return rc;
  try {
    if (n > 32) {
      // every minor materialised (q x q) and run through cplx_perman
      std::vector<double> buf(2 * (size_t)q * q);
      for (uint64_t k = 0; k < count; ++k)
        for (int j = 0; j < n; ++j) {
          for (int r = 0, i = 0; i < n; ++i) {
            if (i == j) continue;
            for (int c = 0; c < q; ++c) {
              const double* v = entry(k, i, c);
              buf[2 * ((size_t)r * q + c)] = v[0], buf[2 * ((size_t)r * q + c) + 1] = v[1];
            }
            ++r;
          }
          CplxInfo one;
          double* dst = out + 2 * (k * n + j);
          if (int rc = cplx_perman(buf.data(), q, o, on_cpu, dst, dst + 1, &one)) return rc;
          ci.kernel_ms += one.kernel_ms;
          ci.grid = one.grid;
          ci.devices = one.devices;
        }
      if (info) *info = ci;
      return SUP_OK;
    }
    if (on_cpu) {
      const int T = std::max(o.threads, 1);
      const uint64_t C = ci.lay.chunks();
      const double f = 4.0 * (q & 1) - 2.0;  // a power-of-two scale, exact
      auto one = [&](uint64_t k, int threads) -> int {
        try {
          std::vector<double> tab, x0, parts(2 * (size_t)C * n);
          minors_tables([&](int j, int c) { return entry(k, j, c); }, n, tab, x0);
          cpu_minors_range(tab, x0, n, ci.lay, 0, C, threads, parts.data());
          for (int j = 0; j < n; ++j) {
            const cx total = fold_pairwise(parts.data() + 2 * (size_t)j * C, C);
            out[2 * (k * n + j)] = f * total.re;
            out[2 * (k * n + j) + 1] = f * total.im;
          }
          return SUP_OK;
        } catch (const std::bad_alloc&) {
          set_error("out of host memory for the wave-chunk partials of matrix " + std::to_string(k));
          return SUP_ENOMEM;
        }
      };
      if (count < (uint64_t)T) {  // few matrices: the threads share each matrix's chunks
        for (uint64_t k = 0; k < count; ++k)
          if (int rc = one(k, T)) return rc;
      } else if (int rc = for_matrices(count, T, [&](int, uint64_t k) { return one(k, 1); })) {
        return rc;
      }
      if (info) *info = ci;
      return SUP_OK;
    }
  } catch (const std::bad_alloc&) {
    set_error(std::string(who) + ": out of host memory");
    return SUP_ENOMEM;
  }
  const int G =
      (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)std::max(1, std::min(o.gpu_num, ndev - o.device_id)), count));
  std::vector<int> drc(G, SUP_OK), dgrid(G, 0);
  std::vector<double> dms(G, 0.0);
  std::vector<std::string> derr(G);
  auto work = [&](int g) {
    const uint64_t a = count * (uint64_t)g / (uint64_t)G, b = count * (uint64_t)(g + 1) / (uint64_t)G;
    drc[g] = run_cplx_minors(o.device_id + g, n, ci.lay, in, a, b, out + 2 * a * n, &dms[g], &dgrid[g]);
    if (drc[g]) derr[g] = last_error();
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
  ci.kernel_ms = *std::max_element(dms.begin(), dms.end());
  ci.grid = dgrid[0];
  ci.devices = G;
  if (info) *info = ci;
  return SUP_OK;
}

int cplx_minors_range(const double* mat, int n, uint64_t c0, uint64_t c1, const sup_opts& o, bool on_cpu, double* out,
                      CplxInfo* info) {
  const char* who = "sup_perman_complex_minors_range";
  if (!mat || !out) {
    set_error(std::string(who) + ": null matrix or output pointer");
    return SUP_EINVAL;
  }
  if (n < 2 || n > 32) {
    set_error(std::string(who) + ": n = " + std::to_string(n) + " outside [2, 32] (the one-walk minors)");
    return SUP_EUNSUPPORTED;
  }
  if (o.walk_log2 < 0 || o.walk_log2 > 31) {
    set_error("walk_log2 = " + std::to_string(o.walk_log2) + " outside [0, 31] (0 = default layout)");
    return SUP_EINVAL;
  }
  const int q = n - 1;
  CplxInfo ci;
  ci.lay = layout_with_walk(q, o.walk_log2);
  if (c0 > c1 || c1 > ci.lay.chunks()) {
    set_error("wave-chunk range [c0, c1) must satisfy c0 <= c1 <= " + std::to_string(ci.lay.chunks()) +
              " (the plan's chunks)");
    return SUP_EINVAL;
  }
  const uint64_t count = c1 - c0;
  std::vector<double> parts;
  try {
    parts.assign(2 * (size_t)count * n, 0.0);
    if (on_cpu) {
      std::vector<double> tab, x0;
      minors_tables([&](int j, int c) { return mat + 2 * ((size_t)j * q + c); }, n, tab, x0);
      cpu_minors_range(tab, x0, n, ci.lay, c0, c1, std::max(o.threads, 1), parts.data());
    } else {
      int ndev = 0;
      if (int rc = need_device(o, who, &ndev)) return rc;
      // the matrix as U with identity lists: the device gathers where it writes the tables
      std::vector<int32_t> idx(n);
      for (int j = 0; j < n; ++j) idx[j] = j;
      CplxBatchIn in;
      in.U = mat, in.R = n, in.C = q, in.rows = idx.data(), in.cols = idx.data();
      if (int rc = run_cplx_minors_range(o.device_id, n, ci.lay, in, c0, c1, parts.data(), &ci.kernel_ms, &ci.grid))
        return rc;
      ci.devices = 1;
    }
    for (int j = 0; j < n; ++j) {
      const cx total = fold_pairwise(parts.data() + 2 * (size_t)j * count, count);
      out[2 * j] = total.re;
      out[2 * j + 1] = total.im;
    }
  } catch (const std::bad_alloc&) {
    set_error("out of host memory for " + std::to_string(count) + " wave-chunk partials per output");
    return SUP_ENOMEM;
  }
  if (info) *info = ci;
  return SUP_OK;
}

}  // namespace sup
