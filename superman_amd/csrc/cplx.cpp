// cplx.cpp — the permanent of a complex fp64 matrix: sup_perman_complex and
// sup_perman_complex_range, and many of them in one call:
// sup_perman_complex_batch and sup_perman_complex_submatrices
// (cplx_perman_batch at the end of this file).  The reference has no counterpart ("SUPerman does
// not support complex type", revised_perman/main.cpp:1557).
//
// Plan: the dense identity plan of Re A (default layout, or o.walk_log2 walk
// bits), its column table followed by the same table of Im A (two identity
// make_plan calls).  Start vector: x0_j = a_j,n-1 - rowsum_j / 2,
// componentwise in fp64 (nw_start on each part).
// Walk: walk_cplx.hip on o.gpu_num devices (static contiguous split of the
// wave-chunks, one host thread per device), or cpu_cplx_range below on host
// threads — the same cx.hpp operations in the same order, so the chunk
// partials are bit-identical.  They are combined on the host in one fixed
// pairwise tree over the chunk index (re and im each plain fp64 adds), so the
// result is a function of (matrix, walk bits) only: the device count, the
// split and the host thread count change no bit.
#include <algorithm>
#include <chrono>
#include <new>
#include <string>
#include <thread>

#include "cx.hpp"
#include "engine.hpp"

namespace sup {

namespace {

// Start state of wave-chunk ga, lane `lane` (walk_cplx.hip's chunk start).
void cx_start(const Plan& P, const std::vector<double>& x0c, uint64_t ga, uint32_t lane, cx* x) {
  const int n = P.n, NP = P.NP, L = P.lay.L;
  const double* re = P.cols.data();
  const double* im = re + P.cols.size() / 2;
  for (int r = 0; r < n; ++r) x[r] = cx{x0c[r], x0c[NP + r]};
  uint64_t h = ga ^ (ga >> 1);
  const int hb = L + P.lay.m;
  while (h) {
    const int b = __builtin_ctzll(h);
    h &= h - 1;
    const size_t off = (size_t)(2 * (hb + b)) * NP;
    for (int r = 0; r < n; ++r) x[r] = cx_add_d2(x[r], re[off + r], im[off + r]);
  }
  for (int e = 0; e < L; ++e) {
    const size_t off = (size_t)(2 * e) * NP;
    const bool on = (lane >> e) & 1u;
    for (int r = 0; r < n; ++r) x[r] = cx_add_d2(x[r], on ? re[off + r] : 0.0, on ? im[off + r] : 0.0);
  }
}

// cx_prod4 (walk_cplx.hip): strided partials p_{j mod 4}, then (p0 p1)(p2 p3).
cx cx_prod(const cx* x, int n) {
  const cx one{1.0, 0.0};
  cx p[4] = {x[0], n > 1 ? x[1] : one, n > 2 ? x[2] : one, n > 3 ? x[3] : one};
  for (int j = 4; j < n; ++j) p[j & 3] = cx_mul(p[j & 3], x[j]);
  if (n == 1) return p[0];
  if (n == 2) return cx_mul(p[0], p[1]);
  if (n == 3) return cx_mul(cx_mul(p[0], p[1]), p[2]);
  return cx_mul(cx_mul(p[0], p[1]), cx_mul(p[2], p[3]));
}

// One wave-chunk, every lane, then the 64-lane xor butterfly (cx_wave_sum).
cx cx_chunk(const Plan& P, const std::vector<double>& x0c, uint64_t ga) {
  const int n = P.n, NP = P.NP, L = P.lay.L;
  const uint32_t T = 1u << P.lay.m;
  const size_t plane = P.cols.size() / 2;
  const double* reL = P.cols.data() + (size_t)(2 * L) * NP;  // walk bit 0, + and - columns follow
  const double* imL = reL + plane;
  cx v[64];
  std::vector<cx> x(n);
  auto step = [&](size_t off) {
    for (int r = 0; r < n; ++r) x[r] = cx_add_d2(x[r], reL[off + r], imL[off + r]);
  };
  for (uint32_t lane = 0; lane < 64; ++lane) {
    if (lane >= (1u << L)) {
      v[lane] = cx{0.0, 0.0};
      continue;
    }
    cx_start(P, x0c, ga, lane, x.data());
    cx acc = cx_prod(x.data(), n);
    uint32_t t = 1;
    for (; t + 1 < T; t += 2) {
      step((size_t)((t >> 1) & 1u) * NP);
      acc = cx_sub(acc, cx_prod(x.data(), n));
      const uint32_t u = t + 1;
      const uint32_t k = (uint32_t)__builtin_ctz(u);
      const uint32_t neg = (u >> (k + 1)) & 1u;
      step((size_t)(2u * k + neg) * NP);
      acc = cx_add(acc, cx_prod(x.data(), n));
    }
    if (t < T) {
      step((size_t)((t >> 1) & 1u) * NP);
      acc = cx_sub(acc, cx_prod(x.data(), n));
    }
    const uint32_t lane_par = __builtin_popcount(lane) & 1u;
    if (((uint32_t)ga ^ lane_par) & 1u) acc = cx_neg(acc);
    v[lane] = acc;
  }
  for (int off = 1; off <= 32; off <<= 1) {
    cx w[64];
    for (int l = 0; l < 64; ++l) w[l] = cx_add(v[l], v[l ^ off]);
    std::copy(w, w + 64, v);
  }
  return v[0];
}

// Pairwise tree over the chunk index (an odd last element moves up as it is).
cx cx_pairwise(const double* parts, uint64_t count) {
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

// The layout of a complex walk of order n: the default layout, or o.walk_log2
// walk bits (n in [1, 64], o.walk_log2 in [0, 31]).
Layout cplx_layout(int n, const sup_opts& o) { return layout_with_walk(n, o.walk_log2); }

}  // namespace

// The plan (column planes Re, Im in P.cols) and start vector of A, n x n
// row-major interleaved (re, im); cplx_quad.cpp walks the same plan.
int cplx_plan(const double* A, int n, const sup_opts& o, Plan& P, std::vector<double>& x0c) {
  if (!A) {
    set_error("null matrix pointer");
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
  const Layout lay = cplx_layout(n, o);
  const size_t nn = (size_t)n * n;
  std::vector<double> Ar(nn), Ai(nn);
  for (size_t i = 0; i < nn; ++i) Ar[i] = A[2 * i], Ai[i] = A[2 * i + 1];
  Plan Pi;
  int rc = make_plan(Ar.data(), n, kWalkDense, true, lay, P);
  if (!rc) rc = make_plan(Ai.data(), n, kWalkDense, true, lay, Pi);
  if (rc) return rc;
  P.cols.insert(P.cols.end(), Pi.cols.begin(), Pi.cols.end());
  x0c = P.x0;
  x0c.insert(x0c.end(), Pi.x0.begin(), Pi.x0.end());
  P.chunk_ends = 0;  // the complex walk has no chunk-end check
  return SUP_OK;
}

namespace {

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

}  // namespace

void cpu_cplx_range(const Plan& P, const std::vector<double>& x0c, uint64_t c0, uint64_t c1, int threads,
                    double* parts) {
  if (c1 <= c0) return;
  const uint64_t count = c1 - c0;
  const int nt = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)std::max(threads, 1), count));
  std::vector<std::thread> th;
  for (int w = 0; w < nt; ++w)
    th.emplace_back([&, w]() {
      for (uint64_t a = (uint64_t)w; a < count; a += (uint64_t)nt) {
        const cx v = cx_chunk(P, x0c, c0 + a);
        parts[2 * a] = v.re, parts[2 * a + 1] = v.im;
      }
    });
  for (auto& t : th) t.join();
}

int cplx_perman_range(const double* A, int n, uint64_t c0, uint64_t c1, const sup_opts& o, bool on_cpu, double* re,
                      double* im, CplxInfo* info) {
  Plan P;
  std::vector<double> x0c;
  int rc = cplx_plan(A, n, o, P, x0c);
  if (rc) return rc;
  if (c0 > c1 || c1 > P.lay.chunks()) {
    set_error("wave-chunk range [c0, c1) must satisfy c0 <= c1 <= " + std::to_string(P.lay.chunks()) +
              " (the plan's chunks)");
    return SUP_EINVAL;
  }
  const uint64_t count = c1 - c0;
  std::vector<double> parts;
  try {
    parts.assign(2 * (size_t)count, 0.0);
  } catch (const std::bad_alloc&) {
    set_error("out of host memory for " + std::to_string(count) + " wave-chunk partials");
    return SUP_ENOMEM;
  }
  CplxInfo ci;
  ci.lay = P.lay;
  if (on_cpu) {
    cpu_cplx_range(P, x0c, c0, c1, std::max(o.threads, 1), parts.data());
  } else {
    int ndev = 0;
    if ((rc = need_device(o, "sup_perman_complex_range", &ndev))) return rc;
    if ((rc = run_range_cplx(o.device_id, P, x0c, c0, c1, parts.data(), &ci.kernel_ms, &ci.grid))) return rc;
    ci.devices = 1;
  }
  const cx total = cx_pairwise(parts.data(), count);
  *re = total.re;
  *im = total.im;
  if (info) *info = ci;
  return SUP_OK;
}

int cplx_perman(const double* A, int n, const sup_opts& o, bool on_cpu, double* re, double* im, CplxInfo* info) {
  Plan P;
  std::vector<double> x0c;
  int rc = cplx_plan(A, n, o, P, x0c);
  if (rc) return rc;
  const uint64_t C = P.lay.chunks();
  std::vector<double> parts;
  try {
    parts.assign(2 * (size_t)C, 0.0);
  } catch (const std::bad_alloc&) {
    set_error("out of host memory for " + std::to_string(C) + " wave-chunk partials");
    return SUP_ENOMEM;
  }
  CplxInfo ci;
  ci.lay = P.lay;
  if (on_cpu) {
    cpu_cplx_range(P, x0c, 0, C, std::max(o.threads, 1), parts.data());
  } else {
    int ndev = 0;
    if ((rc = need_device(o, "sup_perman_complex", &ndev))) return rc;
    const int G =
        (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)std::max(1, std::min(o.gpu_num, ndev - o.device_id)), C));
    std::vector<int> drc(G, SUP_OK), dgrid(G, 0);
    std::vector<double> dms(G, 0.0);
    std::vector<std::string> derr(G);  // g_err is thread_local: carry worker messages back
    auto work = [&](int g) {
      const uint64_t a = C * (uint64_t)g / (uint64_t)G, b = C * (uint64_t)(g + 1) / (uint64_t)G;
      drc[g] = run_range_cplx(o.device_id + g, P, x0c, a, b, parts.data() + 2 * a, &dms[g], &dgrid[g]);
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
  }
  const cx total = cx_pairwise(parts.data(), C);
  // perm = (4(n&1) - 2) * total: a power-of-two scale, exact
  const double f = 4.0 * (n & 1) - 2.0;
  *re = f * total.re;
  *im = f * total.im;
  if (info) *info = ci;
  return SUP_OK;
}

// ---- batched permanents: sup_perman_complex_batch, sup_perman_complex_submatrices ----
// Result k is cplx_perman's of matrix k alone (same walk bits), bit for bit:
// every matrix keeps its layout, chunk enumeration, cx.hpp operation order and
// the pairwise tree over its own chunk partials.  n <= 32 on the device: the
// batched walk (run_cplx_batch), o.gpu_num devices taking contiguous ranges of
// matrices, one host thread each.  n > 32 (one matrix already fills the chip):
// the matrices one after another through cplx_perman.  on_cpu: cplx_plan,
// cpu_cplx_range and cx_pairwise per matrix, o.threads host threads spread
// over the matrices, or over one matrix's chunks when there are fewer
// matrices than threads.
int cplx_perman_batch(const CplxBatchIn& in, int n, uint64_t count, const sup_opts& o, bool on_cpu, double* out,
                      CplxInfo* info) {
  const bool sub = in.U != nullptr;
  const char* who = sub ? "sup_perman_complex_submatrices" : "sup_perman_complex_batch";
  if (!out || (!sub && !in.mats) || (sub && (!in.rows || !in.cols))) {
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
  if (sub && (in.R < 1 || in.C < 1)) {
    set_error(std::string(who) + ": U must have at least one row and one column (R = " + std::to_string(in.R) +
              ", C = " + std::to_string(in.C) + ")");
    return SUP_EINVAL;
  }
  if (sub)
    for (uint64_t k = 0; k < count; ++k)
      for (int j = 0; j < n; ++j) {
        const int32_t r = in.rows[k * n + j], c = in.cols[k * n + j];
        if (r < 0 || r >= in.R || c < 0 || c >= in.C) {
          const bool row_bad = r < 0 || r >= in.R;
          set_error(std::string(who) + ": " + (row_bad ? "rows" : "cols") + "[k = " + std::to_string(k) +
                    "][position " + std::to_string(j) + "] = " + std::to_string(row_bad ? r : c) + " outside [0, " +
                    std::to_string(row_bad ? in.R : in.C) + ")");
          return SUP_EINVAL;
        }
      }
  CplxInfo ci;
  ci.lay = cplx_layout(n, o);
  if (info) *info = ci;
  if (count == 0) return SUP_OK;
  const size_t nn = (size_t)n * n;
  // matrix k, n x n interleaved: in place (raw form) or gathered into buf
  auto matrix = [&](uint64_t k, std::vector<double>& buf) -> const double* {
    if (!sub) return in.mats + k * 2 * nn;
    buf.resize(2 * nn);
    for (int j = 0; j < n; ++j) {
      const double* urow = in.U + 2 * (size_t)in.rows[k * n + j] * in.C;
      for (int c = 0; c < n; ++c) {
        const double* v = urow + 2 * (size_t)in.cols[k * n + c];
        buf[2 * ((size_t)j * n + c)] = v[0];
        buf[2 * ((size_t)j * n + c) + 1] = v[1];
      }
    }
    return buf.data();
  };
  if (on_cpu) {
    const int T = std::max(o.threads, 1);
    auto one = [&](uint64_t k, int threads, std::vector<double>& buf, std::vector<double>& parts) -> int {
      try {
        Plan P;
        std::vector<double> x0c;
        if (int rc = cplx_plan(matrix(k, buf), n, o, P, x0c)) return rc;
        const uint64_t C = P.lay.chunks();
        parts.assign(2 * (size_t)C, 0.0);
        cpu_cplx_range(P, x0c, 0, C, threads, parts.data());
        const cx total = cx_pairwise(parts.data(), C);
        const double f = 4.0 * (n & 1) - 2.0;
        out[2 * k] = f * total.re;
        out[2 * k + 1] = f * total.im;
        return SUP_OK;
      } catch (const std::bad_alloc&) {
        set_error("out of host memory for the wave-chunk partials of matrix " + std::to_string(k));
        return SUP_ENOMEM;
      }
    };
    if (count < (uint64_t)T) {  // few matrices: the threads share each matrix's chunks
      std::vector<double> buf, parts;
      for (uint64_t k = 0; k < count; ++k)
        if (int rc = one(k, T, buf, parts)) return rc;
    } else {
      std::vector<int> wrc(T, SUP_OK);
      std::vector<std::string> werr(T);  // g_err is thread_local: carry worker messages back
      auto work = [&](int w) {
        std::vector<double> buf, parts;
        for (uint64_t k = (uint64_t)w; k < count && !wrc[w]; k += (uint64_t)T)
          if ((wrc[w] = one(k, 1, buf, parts))) werr[w] = last_error();
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
    }
    if (info) *info = ci;
    return SUP_OK;
  }
  int ndev = 0;
  if (int rc = need_device(o, who, &ndev)) return rc;
  if (n > 32) {
    std::vector<double> buf;
    for (uint64_t k = 0; k < count; ++k) {
      CplxInfo one;
      if (int rc = cplx_perman(matrix(k, buf), n, o, false, &out[2 * k], &out[2 * k + 1], &one)) return rc;
      ci.kernel_ms += one.kernel_ms;
      ci.grid = one.grid;
      ci.devices = one.devices;
    }
    if (info) *info = ci;
    return SUP_OK;
  }
  const int G =
      (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)std::max(1, std::min(o.gpu_num, ndev - o.device_id)), count));
  std::vector<int> drc(G, SUP_OK), dgrid(G, 0);
  std::vector<double> dms(G, 0.0);
  std::vector<std::string> derr(G);
  auto work = [&](int g) {
    const uint64_t a = count * (uint64_t)g / (uint64_t)G, b = count * (uint64_t)(g + 1) / (uint64_t)G;
    drc[g] = run_cplx_batch(o.device_id + g, n, ci.lay, in, a, b, out + 2 * a, &dms[g], &dgrid[g]);
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

}  // namespace sup
