// cplx_quad.cpp — the permanent of a complex fp64 matrix in double-double
// (~100 bits per part): sup_perman_complex_quad and
// sup_perman_complex_quad_range, the higher-precision result the fp64 complex
// entries (cplx.cpp) are judged against, as quad.cpp is for the real walks.
//
// Plan: cplx_plan's (cplx.cpp: the dense identity plan of Re A, its column
// table followed by Im A's; default layout, or o.walk_log2 walk bits).  Start
// vector: x0_j = a_j,n-1 - rowsum_j / 2 on each part, the row sum accumulated
// in double-double as quad_setup forms it (quad.cpp), so a low word is live
// from the first state: 4 NP doubles in four blocks (re.hi, re.lo, im.hi,
// im.lo).
// Walk: walk_cplxdd.hip on o.gpu_num devices (static contiguous split of the
// wave-chunks, one host thread per device) for n <=
// SUP_CPLX_QUAD_MAX_DEVICE_N, or cpu_cplxdd_range below on host threads for
// every n <= 64 — the same cxdd.hpp operations in the same order, so the
// chunk partials are bit-identical.  They are combined on the host in one
// fixed pairwise tree over the chunk index (dd_add per part), so the result
// is a function of (matrix, walk bits) only: the device count, the split and
// the host thread count change no bit.
#include <algorithm>
#include <new>
#include <stdexcept>
#include <string>
#include <thread>

#include "cxdd.hpp"
#include "engine.hpp"

namespace sup {

namespace {

const cxdd kZero{dd{0.0, 0.0}, dd{0.0, 0.0}};

// Start state of wave-chunk ga, lane `lane` (walk_cplxdd.hip's chunk start).
void cxdd_start(const Plan& P, const std::vector<double>& x0q, uint64_t ga, uint32_t lane, cxdd* x) {
  const int n = P.n, NP = P.NP, L = P.lay.L;
  const double* re = P.cols.data();
  const double* im = re + P.cols.size() / 2;
  for (int r = 0; r < n; ++r) x[r] = cxdd{dd{x0q[r], x0q[NP + r]}, dd{x0q[2 * NP + r], x0q[3 * NP + r]}};
  uint64_t h = ga ^ (ga >> 1);
  const int hb = L + P.lay.m;
  while (h) {
    const int b = __builtin_ctzll(h);
    h &= h - 1;
    const size_t off = (size_t)(2 * (hb + b)) * NP;
    for (int r = 0; r < n; ++r) x[r] = cxdd_add_d2(x[r], re[off + r], im[off + r]);
  }
  for (int e = 0; e < L; ++e) {
    const size_t off = (size_t)(2 * e) * NP;
    const bool on = (lane >> e) & 1u;
    for (int r = 0; r < n; ++r) x[r] = cxdd_add_d2(x[r], on ? re[off + r] : 0.0, on ? im[off + r] : 0.0);
  }
}

// cxdd_prod4 (walk_cplxdd.hip): strided partials p_{j mod 4}, then (p0 p1)(p2 p3).
cxdd cxdd_prod(const cxdd* x, int n) {
  const cxdd one{dd{1.0, 0.0}, dd{0.0, 0.0}};
  cxdd p[4] = {x[0], n > 1 ? x[1] : one, n > 2 ? x[2] : one, n > 3 ? x[3] : one};
  for (int j = 4; j < n; ++j) p[j & 3] = cxdd_mul(p[j & 3], x[j]);
  if (n == 1) return p[0];
  if (n == 2) return cxdd_mul(p[0], p[1]);
  if (n == 3) return cxdd_mul(cxdd_mul(p[0], p[1]), p[2]);
  return cxdd_mul(cxdd_mul(p[0], p[1]), cxdd_mul(p[2], p[3]));
}

// One wave-chunk, every lane, then the 64-lane xor butterfly (cxdd_wave_sum).
cxdd cxdd_chunk(const Plan& P, const std::vector<double>& x0q, uint64_t ga) {
  const int n = P.n, NP = P.NP, L = P.lay.L;
  const uint32_t T = 1u << P.lay.m;
  const size_t plane = P.cols.size() / 2;
  const double* reL = P.cols.data() + (size_t)(2 * L) * NP;  // walk bit 0, + and - columns follow
  const double* imL = reL + plane;
  cxdd v[64];
  std::vector<cxdd> x(n);
  auto step = [&](size_t off) {
    for (int r = 0; r < n; ++r) x[r] = cxdd_add_d2(x[r], reL[off + r], imL[off + r]);
  };
  for (uint32_t lane = 0; lane < 64; ++lane) {
    if (lane >= (1u << L)) {
      v[lane] = kZero;
      continue;
    }
    cxdd_start(P, x0q, ga, lane, x.data());
    cxdd acc = cxdd_prod(x.data(), n);
    uint32_t t = 1;
    for (; t + 1 < T; t += 2) {
      step((size_t)((t >> 1) & 1u) * NP);
      acc = cxdd_add(acc, cxdd_neg(cxdd_prod(x.data(), n)));
      const uint32_t u = t + 1;
      const uint32_t k = (uint32_t)__builtin_ctz(u);
      const uint32_t neg = (u >> (k + 1)) & 1u;
      step((size_t)(2u * k + neg) * NP);
      acc = cxdd_add(acc, cxdd_prod(x.data(), n));
    }
    if (t < T) {
      step((size_t)((t >> 1) & 1u) * NP);
      acc = cxdd_add(acc, cxdd_neg(cxdd_prod(x.data(), n)));
    }
    const uint32_t lane_par = __builtin_popcount(lane) & 1u;
    if (((uint32_t)ga ^ lane_par) & 1u) acc = cxdd_neg(acc);
    v[lane] = acc;
  }
  for (int off = 1; off <= 32; off <<= 1) {
    cxdd w[64];
    for (int l = 0; l < 64; ++l) w[l] = cxdd_add(v[l], v[l ^ off]);
    std::copy(w, w + 64, v);
  }
  return v[0];
}

// Pairwise tree over the chunk index (an odd last element moves up as it is).
cxdd cxdd_pairwise(const double* parts, uint64_t count) {
  if (count == 0) return kZero;
  std::vector<cxdd> v(count);
  for (uint64_t a = 0; a < count; ++a)
    v[a] = cxdd{dd{parts[4 * a], parts[4 * a + 1]}, dd{parts[4 * a + 2], parts[4 * a + 3]}};
  while (v.size() > 1) {
    std::vector<cxdd> w((v.size() + 1) / 2);
    for (size_t i = 0; i < w.size(); ++i) w[i] = 2 * i + 1 < v.size() ? cxdd_add(v[2 * i], v[2 * i + 1]) : v[2 * i];
    v.swap(w);
  }
  return v[0];
}

// The plan (cplx_plan's) and the double-double start vector of A.
int cplx_quad_setup(const double* A, int n, const sup_opts& o, Plan& P, std::vector<double>& x0q) {
  std::vector<double> x0c;  // the fp64 start vector: not used by this walk
  if (int rc = cplx_plan(A, n, o, P, x0c)) return rc;
  const size_t NP = (size_t)P.NP;
  x0q.assign(4 * NP, 0.0);
  for (int j = 0; j < n; ++j) {
    const int i = P.rowperm[j];
    for (int part = 0; part < 2; ++part) {
      const double* row = A + 2 * (size_t)i * n + part;  // entry c of this part at row[2 c]
      dd rs{0.0, 0.0};
      for (int c = 0; c < n; ++c) rs = dd_add_d(rs, row[2 * c]);
      const dd x = dd_add_d(dd{-0.5 * rs.hi, -0.5 * rs.lo}, row[2 * (n - 1)]);
      x0q[2 * part * NP + j] = x.hi, x0q[(2 * part + 1) * NP + j] = x.lo;
    }
  }
  return SUP_OK;
}

// Argument checks that need no plan, then (device path) the cap before the
// device: n above SUP_CPLX_QUAD_MAX_DEVICE_N with on_cpu = 0 is
// SUP_EUNSUPPORTED on any machine, with or without a device.
int cplx_quad_request(const double* A, int n, const sup_opts& o, bool on_cpu, const double* out, const char* who) {
  if (!A || !out) {
    set_error(std::string(who) + ": null matrix or output pointer");
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
  if (!on_cpu && n > SUP_CPLX_QUAD_MAX_DEVICE_N) {
    set_error(std::string(who) + ": n = " + std::to_string(n) + " is above the device cap " +
              std::to_string(SUP_CPLX_QUAD_MAX_DEVICE_N) +
              " (SUP_CPLX_QUAD_MAX_DEVICE_N: 8n VGPRs of state; on_cpu = 1 runs host threads up to n = 64)");
    return SUP_EUNSUPPORTED;
  }
  return SUP_OK;
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

int alloc_parts(std::vector<double>& parts, uint64_t count) {
  try {
    parts.assign(4 * (size_t)count, 0.0);
  } catch (const std::bad_alloc&) {
    set_error("out of host memory for " + std::to_string(count) + " wave-chunk partials");
    return SUP_ENOMEM;
  } catch (const std::length_error&) {
    set_error("out of host memory for " + std::to_string(count) + " wave-chunk partials");
    return SUP_ENOMEM;
  }
  return SUP_OK;
}

}  // namespace

void cpu_cplxdd_range(const Plan& P, const std::vector<double>& x0q, uint64_t c0, uint64_t c1, int threads,
                      double* parts) {
  if (c1 <= c0) return;
  const uint64_t count = c1 - c0;
  const int nt = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)std::max(threads, 1), count));
  std::vector<std::thread> th;
  for (int w = 0; w < nt; ++w)
    th.emplace_back([&, w]() {
      for (uint64_t a = (uint64_t)w; a < count; a += (uint64_t)nt) {
        const cxdd v = cxdd_chunk(P, x0q, c0 + a);
        parts[4 * a] = v.re.hi, parts[4 * a + 1] = v.re.lo, parts[4 * a + 2] = v.im.hi, parts[4 * a + 3] = v.im.lo;
      }
    });
  for (auto& t : th) t.join();
}

int cplx_quad_perman_range(const double* A, int n, uint64_t c0, uint64_t c1, const sup_opts& o, bool on_cpu,
                           double* out, CplxInfo* info) {
  const char* who = "sup_perman_complex_quad_range";
  int rc = cplx_quad_request(A, n, o, on_cpu, out, who);
  if (rc) return rc;
  Plan P;
  std::vector<double> x0q;
  if ((rc = cplx_quad_setup(A, n, o, P, x0q))) return rc;
  if (c0 > c1 || c1 > P.lay.chunks()) {
    set_error("wave-chunk range [c0, c1) must satisfy c0 <= c1 <= " + std::to_string(P.lay.chunks()) +
              " (the plan's chunks)");
    return SUP_EINVAL;
  }
  const uint64_t count = c1 - c0;
  std::vector<double> parts;
  if ((rc = alloc_parts(parts, count))) return rc;
  CplxInfo ci;
  ci.lay = P.lay;
  if (on_cpu) {
    cpu_cplxdd_range(P, x0q, c0, c1, std::max(o.threads, 1), parts.data());
  } else {
    int ndev = 0;
    if ((rc = need_device(o, who, &ndev))) return rc;
    if ((rc = run_range_cplxdd(o.device_id, P, x0q, c0, c1, parts.data(), &ci.kernel_ms, &ci.grid))) return rc;
    ci.devices = 1;
  }
  const cxdd total = cxdd_pairwise(parts.data(), count);
  out[0] = total.re.hi, out[1] = total.re.lo, out[2] = total.im.hi, out[3] = total.im.lo;
  if (info) *info = ci;
  return SUP_OK;
}

int cplx_quad_perman(const double* A, int n, const sup_opts& o, bool on_cpu, double* out, CplxInfo* info) {
  const char* who = "sup_perman_complex_quad";
  int rc = cplx_quad_request(A, n, o, on_cpu, out, who);
  if (rc) return rc;
  Plan P;
  std::vector<double> x0q;
  if ((rc = cplx_quad_setup(A, n, o, P, x0q))) return rc;
  const uint64_t C = P.lay.chunks();
  std::vector<double> parts;
  if ((rc = alloc_parts(parts, C))) return rc;
  CplxInfo ci;
  ci.lay = P.lay;
  if (on_cpu) {
    cpu_cplxdd_range(P, x0q, 0, C, std::max(o.threads, 1), parts.data());
  } else {
    int ndev = 0;
    if ((rc = need_device(o, who, &ndev))) return rc;
    const int G =
        (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)std::max(1, std::min(o.gpu_num, ndev - o.device_id)), C));
    std::vector<int> drc(G, SUP_OK), dgrid(G, 0);
    std::vector<double> dms(G, 0.0);
    std::vector<std::string> derr(G);  // g_err is thread_local: carry worker messages back
    auto work = [&](int g) {
      const uint64_t a = C * (uint64_t)g / (uint64_t)G, b = C * (uint64_t)(g + 1) / (uint64_t)G;
      drc[g] = run_range_cplxdd(o.device_id + g, P, x0q, a, b, parts.data() + 4 * a, &dms[g], &dgrid[g]);
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
  const cxdd total = cxdd_pairwise(parts.data(), C);
  // perm = (4(n&1) - 2) * total: a power-of-two scale, exact on every word
  const double f = 4.0 * (n & 1) - 2.0;
  out[0] = f * total.re.hi, out[1] = f * total.re.lo, out[2] = f * total.im.hi, out[3] = f * total.im.lo;
  if (info) *info = ci;
  return SUP_OK;
}

}  // namespace sup
