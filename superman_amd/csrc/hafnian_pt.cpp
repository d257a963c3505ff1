// hafnian_pt.cpp — power-trace hafnians and loop hafnians of complex symmetric
// matrices gathered by index lists: sup_hafnian_complex_pt,
// sup_loop_hafnian_complex_pt, sup_hafnian_complex_pt_range and
// sup_hafnian_complex_pt_plan.
//
// The sum runs over the 2^(n/2) - 1 non-empty subsets z of the index pairs
// (hafpt.hpp); its cost does not depend on repeats.  The checks, the chunking
// and the host twin are here; the twin runs hafpt.hpp's operations in
// walk_hafpt.hip's order, so result k is a function of (A, mu, idx[k]) only
// and has the device's bits.
#include <algorithm>
#include <atomic>
#include <cstring>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "cx.hpp"
#include "engine.hpp"
#include "hafnian_pt.hpp"
#include "hafpt.hpp"

namespace sup {

namespace {

constexpr size_t kPtSlabCapBytes = (size_t)256 << 20;

// The 64-lane xor butterfly (walk_hafpt.hip pt_wave_sum) on v[0..63].
cx pt_butterfly(cx* v) {
  for (int off = 1; off <= 32; off <<= 1) {
    cx w[64];
    for (int l = 0; l < 64; ++l) w[l] = cx_add(v[l], v[l ^ off]);
    std::copy(w, w + 64, v);
  }
  return v[0];
}

struct PtWork {
  std::vector<cx> T, cur;  // 64 rows of np pairs
  cx xs[kPtMaxM + 1], jc[kPtMaxM + 1], gs[kPtMaxM + 1];
};

// f(z) of the matrix with table tab (hafpt.hpp's order).
cx pt_subset(const double* tab, int np, int m, bool loop, const double* coef, uint32_t z, PtWork& W) {
  const int NP = hafpt_pad8(np);
  auto C = [&](int l, int c) { return cx{tab[2 * ((size_t)l * NP + c)], tab[2 * ((size_t)l * NP + c) + 1]}; };
  auto D = [&](int i) { return C(np, i); };
  int r[64], R = 0;
  for (int b = 0; b < m; ++b)
    if ((z >> b) & 1u) r[R++] = 2 * b, r[R++] = 2 * b + 1;
  const cx zero{0.0, 0.0};
  cx v[64];
  if (loop) {
    cx y[64], yv[64];
    for (int i = 0; i < R; ++i) y[i] = D(r[i]);
    for (int j = 1; j <= m; ++j) {
      for (int i = 0; i < 64; ++i) v[i] = i < R ? cx_mul(D(r[i] ^ 1), y[i]) : zero;
      W.xs[j] = pt_butterfly(v);
      if (j < m) {
        for (int i = 0; i < R; ++i) yv[r[i]] = y[i];
        for (int i = 0; i < R; ++i) {
          cx acc = zero;
          for (int li = 0; li < R; ++li) acc = cx_fma(C(r[i], r[li]), yv[r[li]], acc);
          y[i] = acc;
        }
      }
    }
  }
  auto emit = [&](int j) {
    for (int i = R; i < 64; ++i) v[i] = zero;
    const cx t = pt_butterfly(v);
    const cx c = hafpt_cj(t, loop ? W.xs[j] : zero, coef[j], loop);
    W.jc[j] = hafpt_scale((double)j, c);
  };
  cx* T = W.T.data();
  cx* cur = W.cur.data();
  auto trace = [&]() {
    for (int i = 0; i < R; ++i) {
      cx s = zero;
      for (int li = 0; li < R; ++li) s = cx_fma(cur[(size_t)i * np + r[li]], T[(size_t)(i ^ 1) * np + (r[li] ^ 1)], s);
      v[i] = s;
    }
  };
  for (int i = 0; i < R; ++i)
    for (int li = 0; li < R; ++li) cur[(size_t)i * np + r[li]] = C(r[i], r[li]);
  for (int i = 0; i < R; ++i) v[i] = C(r[i], r[i]);
  emit(1);
  auto store = [&]() {
    for (int i = 0; i < R; ++i)
      for (int li = 0; li < R; ++li) T[(size_t)i * np + r[li]] = cur[(size_t)i * np + r[li]];
  };
  if (m >= 2) {
    store();
    trace();
    emit(2);
  }
  const int A = (m + 1) / 2;
  for (int a = 2; a <= A; ++a) {
    for (int i = 0; i < R; ++i) {
      cx* row = cur + (size_t)i * np;
      for (int ci = 0; ci < R; ++ci) row[r[ci]] = zero;
      for (int li = 0; li < R; ++li) {
        const int l = r[li];
        const cx p = T[(size_t)i * np + l];
        const double* crow = tab + 2 * (size_t)l * NP;
        for (int ci = 0; ci < R; ++ci) {
          const int c = r[ci];
          row[c] = cx_fma(p, cx{crow[2 * c], crow[2 * c + 1]}, row[c]);
        }
      }
    }
    trace();
    emit(2 * a - 1);
    if (2 * a <= m) {
      store();
      trace();
      emit(2 * a);
    }
  }
  const double* invs = coef + (kPtMaxM + 1);
  W.gs[0] = cx{1.0, 0.0};
  for (int s = 1; s <= m; ++s) {
    cx acc = zero;
    for (int j = 1; j <= s; ++j) acc = cx_fma(W.jc[j], W.gs[s - j], acc);
    W.gs[s] = hafpt_scale(invs[s], acc);
  }
  return W.gs[m];
}

inline cx pt_signed(cx f, int m, uint32_t z) { return ((m - __builtin_popcount(z)) & 1) ? cx_neg(f) : f; }

// The host twin on one matrix: the chunk partials of z in [z0, z1), then the
// fold.  threads > 1: blocks of subsets are evaluated in parallel and added
// to their chunks in ascending z.
cx pt_cpu_matrix(const double* tab, int np, bool loop, const double* coef, uint64_t z0, uint64_t z1, int threads) {
  const int m = np / 2, llog = hafpt_chunk_log(m);
  const uint64_t cfirst = z0 >> llog, cm = ((z1 + (1ull << llog) - 1) >> llog) - cfirst;
  std::vector<double> parts(2 * (size_t)cm, 0.0);
  auto add = [&](uint64_t z, cx f) {
    const size_t c = (size_t)((z >> llog) - cfirst);
    const cx s = cx_add(cx{parts[2 * c], parts[2 * c + 1]}, pt_signed(f, m, (uint32_t)z));
    parts[2 * c] = s.re, parts[2 * c + 1] = s.im;
  };
  const uint64_t zs = std::max<uint64_t>(1, z0);  // z = 0 is no subset: its chunk starts at z = 1
  const int nt = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)std::max(threads, 1), (z1 - zs + 3) / 4));
  if (nt == 1) {
    PtWork W;
    W.T.resize((size_t)64 * np), W.cur.resize((size_t)64 * np);
    for (uint64_t z = zs; z < z1; ++z) add(z, pt_subset(tab, np, m, loop, coef, (uint32_t)z, W));
  } else {
    const uint64_t block = (uint64_t)nt * 256;
    std::vector<cx> f((size_t)block);
    for (uint64_t b0 = zs; b0 < z1; b0 += block) {
      const uint64_t b1 = std::min(z1, b0 + block);
      std::atomic<uint64_t> next{b0};
      auto work = [&]() {
        PtWork W;
        W.T.resize((size_t)64 * np), W.cur.resize((size_t)64 * np);
        for (;;) {
          const uint64_t a = next.fetch_add(4);
          if (a >= b1) break;
          for (uint64_t z = a; z < std::min(b1, a + 4); ++z)
            f[(size_t)(z - b0)] = pt_subset(tab, np, m, loop, coef, (uint32_t)z, W);
        }
      };
      std::vector<std::thread> th;
      for (int w = 1; w < nt; ++w) th.emplace_back(work);
      work();
      for (auto& t : th) t.join();
      for (uint64_t z = b0; z < b1; ++z) add(z, f[(size_t)(z - b0)]);
    }
  }
  return fock_fold(parts.data(), (uint32_t)cm);
}

void pt_table(const HafIn& in, const int32_t* idx, int n, int np, std::vector<double>& tab) {
  const uint64_t pairs = hafpt_pairs(np);
  tab.resize(2 * (size_t)pairs);
  for (uint64_t e = 0; e < pairs; ++e) {
    const cx v = hafpt_entry(in.A, in.M, in.loop ? in.mu : nullptr, idx, n, np, e);
    tab[2 * (size_t)e] = v.re, tab[2 * (size_t)e + 1] = v.im;
  }
}

void pt_coef(double* coef) {
  std::fill(coef, coef + kPtCoef, 0.0);
  for (int j = 1; j <= kPtMaxM; ++j) coef[j] = 1.0 / (2.0 * j), coef[kPtMaxM + 1 + j] = 1.0 / (double)j;
}

}  // namespace

int hafnian_pt_plan(int n, int loop, uint64_t* subsets, double* est_ops) {
  if (n < 1 || n > SUP_MAX_N) {
    set_error("n = " + std::to_string(n) + " outside [1, 64] (64-bit Gray index)");
    return SUP_EINVAL;
  }
  const bool none = !loop && (n & 1);
  const int m = (n + 1) / 2;
  if (subsets) *subsets = none ? 0 : (1ull << m) - 1;
  if (est_ops) *est_ops = none ? 0.0 : hafpt_ops(m, loop != 0);
  return SUP_OK;
}

int hafnian_pt(const HafIn& in, int n, uint64_t count, bool range, uint64_t z_begin, uint64_t z_end,
               const sup_opts& o, bool on_cpu, double* out, PtInfo* info) {
  const std::string who = range ? "sup_hafnian_complex_pt_range"
                                : in.loop ? "sup_loop_hafnian_complex_pt" : "sup_hafnian_complex_pt";
  if (!out || !in.A || !in.idx || (in.loop && !in.mu)) {
    set_error(who + ": null pointer");
    return SUP_EINVAL;
  }
  if (n < 1 || n > SUP_MAX_N) {
    set_error("n = " + std::to_string(n) + " outside [1, 64] (64-bit Gray index)");
    return SUP_EINVAL;
  }
  if (in.M < 1) {
    set_error(who + ": A must have at least one row (M = " + std::to_string(in.M) + ")");
    return SUP_EINVAL;
  }
  for (int i = 0; i < in.M; ++i)
    for (int j = 0; j < i; ++j)
      if (std::memcmp(in.A + 2 * ((size_t)i * in.M + j), in.A + 2 * ((size_t)j * in.M + i), 2 * sizeof(double)) != 0) {
        set_error(who + ": A[" + std::to_string(j) + "][" + std::to_string(i) + "] and A[" + std::to_string(i) + "][" +
                  std::to_string(j) + "] differ: A must be symmetric bit for bit");
        return SUP_EINVAL;
      }
  for (uint64_t k = 0; k < count; ++k)
    for (int j = 0; j < n; ++j) {
      const int32_t v = in.idx[k * n + j];
      if (v < 0 || v >= in.M) {
        set_error(who + ": idx[k = " + std::to_string(k) + "][position " + std::to_string(j) + "] = " +
                  std::to_string(v) + " outside [0, " + std::to_string(in.M) + ")");
        return SUP_EINVAL;
      }
    }
  const int np = n + (n & 1), m = np / 2;
  if (range && (z_begin > z_end || z_end > (1ull << m))) {
    set_error(who + ": subsets [" + std::to_string(z_begin) + ", " + std::to_string(z_end) + ") outside 0 <= z_begin <= z_end <= 2^" +
              std::to_string(m));
    return SUP_EINVAL;
  }
  PtInfo pi;
  if (info) *info = pi;
  if (count == 0) return SUP_OK;
  if (!on_cpu && n > SUP_HAFNIAN_PT_MAX_DEVICE_N) {
    set_error(who + ": n = " + std::to_string(n) + " above the device cap SUP_HAFNIAN_PT_MAX_DEVICE_N = " +
              std::to_string(SUP_HAFNIAN_PT_MAX_DEVICE_N) + " (on_cpu = 1 serves n <= 64)");
    return SUP_EUNSUPPORTED;
  }
  int G = 1;
  if (!on_cpu) {
    int ndev = 0;
    int rc = device_count(&ndev);
    if (rc) return rc;
    if (ndev == 0) {
      set_error("no HIP device available (" + who + " has no CPU fallback; on_cpu = 1 runs host threads)");
      return SUP_ENODEV;
    }
    if (o.device_id < 0 || o.device_id >= ndev) {
      set_error(who + ": device_id out of range");
      return SUP_EINVAL;
    }
    G = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)std::max(1, std::min(o.gpu_num, ndev - o.device_id)), count));
  }
  const uint64_t z0 = range ? z_begin : 0, z1 = range ? z_end : (1ull << m);
  if ((!in.loop && (n & 1)) || std::max<uint64_t>(1, z0) >= z1) {  // no perfect matching, or no subset: exactly zero, nothing visited
    std::fill(out, out + 2 * count, 0.0);
    return SUP_OK;
  }
  pi.subsets = count * (z1 - std::max<uint64_t>(1, z0));
  pi.ops = hafpt_ops(m, in.loop);
  double coef[kPtCoef];
  pt_coef(coef);
  const int T = std::max(o.threads, 1);
  if (on_cpu) {
    try {
      if (count >= (uint64_t)T && T > 1) {  // one matrix per thread at a time
        std::atomic<uint64_t> next{0};
        auto work = [&]() {
          std::vector<double> tab;
          for (uint64_t k = next.fetch_add(1); k < count; k = next.fetch_add(1)) {
            pt_table(in, in.idx + k * n, n, np, tab);
            const cx v = pt_cpu_matrix(tab.data(), np, in.loop, coef, z0, z1, 1);
            out[2 * k] = v.re, out[2 * k + 1] = v.im;
          }
        };
        std::vector<std::thread> th;
        for (int w = 1; w < T; ++w) th.emplace_back(work);
        work();
        for (auto& t : th) t.join();
      } else {
        std::vector<double> tab;
        for (uint64_t k = 0; k < count; ++k) {
          pt_table(in, in.idx + k * n, n, np, tab);
          const cx v = pt_cpu_matrix(tab.data(), np, in.loop, coef, z0, z1, T);
          out[2 * k] = v.re, out[2 * k + 1] = v.im;
        }
      }
    } catch (const std::bad_alloc&) {
      set_error("out of host memory for the power-trace tables and partials");
      return SUP_ENOMEM;
    }
    if (info) *info = pi;
    return SUP_OK;
  }
  // matrices [a, b) of a device in slabs: as many as keep a slab under
  // kPtSlabCapBytes and 2^31 chunks (at least one)
  const int llog = hafpt_chunk_log(m);
  const uint64_t cm = ((z1 + (1ull << llog) - 1) >> llog) - (z0 >> llog);
  const uint64_t per = 16 * hafpt_pairs(np) + cm * 16 + (uint64_t)n * 4 + 16;
  const uint64_t slab = std::max<uint64_t>(1, std::min<uint64_t>(kPtSlabCapBytes / per, 0x7fffffffull / cm));
  std::vector<int> drc(G, SUP_OK), dgrid(G, 0);
  std::vector<double> dms(G, 0.0);
  std::vector<std::string> derr(G);  // g_err is thread_local: carry worker messages back
  auto work = [&](int g) {
    const uint64_t a = count * (uint64_t)g / (uint64_t)G, b = count * (uint64_t)(g + 1) / (uint64_t)G;
    for (uint64_t k = a; k < b && !drc[g]; k += slab) {
      double ms = 0.0;
      drc[g] = run_hafnian_pt(o.device_id + g, in, n, np, k, std::min(slab, b - k), z0, z1, coef, out + 2 * k, &ms,
                              &dgrid[g]);
      if (drc[g]) derr[g] = last_error();
      dms[g] += ms;
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
  pi.kernel_ms = *std::max_element(dms.begin(), dms.end());
  pi.grid = dgrid[0];
  pi.devices = G;
  if (info) *info = pi;
  return SUP_OK;
}

}  // namespace sup
