// cplx_exact.cpp — the exact permanent of a matrix of Gaussian integers:
// sup_perman_complex_exact and sup_perman_complex_exact_range, the integer
// truth the floating complex entries (cplx.cpp, cplx_quad.cpp) are judged
// against, as exact.cpp is for the real ones.
//
// The sum (include/superman.h states it in full): the walk runs on 2A, so
// X_j(S) = 2 a_j,n-1 - sum_c a_jc + 2 sum_{e in S} a_je is a Gaussian integer
// with |Re X_j|, |Im X_j| <= R_j = sum_c (|Re a_jc| + |Im a_jc|) < 2^31, exact
// in two fp64 values; T = sum_S (-1)^|S| prod_j X_j(S) has |Re T|, |Im T| <=
// 2^(n-1) prod_j R_j, and perm = (4(n&1) - 2) T / 2^n.  Each product is formed
// in (Z/p)[i] (cxexact.hpp) for the largest primes below 2^pbits, taken until
// their product exceeds 8 times that bound; the residues of Re T and Im T are
// joined separately by exact.cpp's CRT, which also checks that each is
// divisible by 2^(n-1).
// Plan: cplx_plan's of 2A (default layout or o.walk_log2 walk bits, identity
// column map; no chunk-end skipping, no column-order search).
// Walk: walk_cplxexact.hip on o.gpu_num devices (static contiguous split of
// the wave-chunks, one host thread per device, kMaxCxPrimes primes per launch)
// for n <= SUP_CPLX_EXACT_MAX_DEVICE_N, or cpu_cplx_exact_range below on host
// threads for every n <= 64: the same residue operations, all exact, so the
// residues agree one for one whatever the split or the order of the sums.
#include <algorithm>
#include <cmath>
#include <string>
#include <thread>

#include "cxexact.hpp"
#include "engine.hpp"

namespace sup {

namespace {

// What both entries decide before they walk: G, the primes, the plan of 2A.
struct CxExactSetup {
  bool zero_row = false;  // a row of zeros (whole = true only): the permanent is 0, nothing else is filled
  int group = 0;
  std::vector<double> primes;
  Plan P;
  std::vector<double> x0c;
};

// Primes below 2^pbits for group products with parts below 2^ybits: a link
// needs 1.5 p Y < 2^52 (cxexact.hpp), and 1.5 2^pbits 2^ybits <= 1.5 2^51.
// p < 2^42 also bounds the 256-step accumulation (256 x 1.5 p < 2^51).
int cxe_pbits(int group, int xbits) { return std::min(42, 51 - (group == 2 ? 2 * xbits + 1 : xbits)); }

int cplx_exact_request(const double* A, int n, const sup_opts& o, const char* who) {
  if (!A) {
    set_error(std::string(who) + ": null matrix pointer");
    return SUP_EINVAL;
  }
  if (n < 1 || n > SUP_MAX_N) {
    set_error(std::string(who) + ": n = " + std::to_string(n) + " outside [1, 64] (64-bit Gray index)");
    return SUP_EINVAL;
  }
  if (o.walk_log2 < 0 || o.walk_log2 > 31) {
    set_error(std::string(who) + ": walk_log2 = " + std::to_string(o.walk_log2) +
              " outside [0, 31] (0 = default layout)");
    return SUP_EINVAL;
  }
  return SUP_OK;
}

// The front half of both entries (`who` in messages): the input limits, G, the
// primes and the plan, then (on_cpu false) the device cap.  whole: the whole
// entry, which stops at a zero row; the range entry walks such a matrix like
// any other (every term is zero).  want_group: 0 the cost model's G, or 1, 2.
int cplx_exact_setup(const double* A, int n, const sup_opts& o, bool on_cpu, bool whole, int want_group,
                     const char* who, CxExactSetup& S) {
  const std::string name(who);
  int rc = cplx_exact_request(A, n, o, who);
  if (rc) return rc;
  if (want_group != 0 && want_group != 1 && want_group != 2) {
    set_error(name + ": group = " + std::to_string(want_group) + " (0 = the cost model's choice, or 1, 2)");
    return SUP_EINVAL;
  }
  double maxrow = 0.0, logT = n - 1;
  bool zero_row = false;
  for (int j = 0; j < n; ++j) {
    double ra = 0.0;
    for (int c = 0; c < n; ++c)
      for (int part = 0; part < 2; ++part) {
        const double v = A[2 * ((size_t)j * n + c) + part];
        const std::string where =
            "entry (row " + std::to_string(j) + ", column " + std::to_string(c) + ", " + (part ? "Im" : "Re") + " part)";
        if (!std::isfinite(v) || v != std::floor(v)) {
          set_error(name + ": " + where + " is not an integer (parts must be integers with |part| < 2^31)");
          return SUP_EINVAL;
        }
        if (std::fabs(v) >= 2147483648.0) {
          set_error(name + ": " + where + " is out of range (parts must be integers with |part| < 2^31)");
          return SUP_EINVAL;
        }
        ra += std::fabs(v);  // exact: at most 128 integers below 2^31
      }
    if (ra >= 2147483648.0) {
      set_error(name + ": row " + std::to_string(j) +
                " has sum_c (|Re a| + |Im a|) >= 2^31 (the row bounds must stay below 2^31)");
      return SUP_EINVAL;
    }
    if (ra == 0.0) {
      zero_row = true;
      continue;
    }
    maxrow = std::max(maxrow, ra);
    logT += std::log2(ra);
  }
  if (!on_cpu && n > SUP_CPLX_EXACT_MAX_DEVICE_N) {
    set_error(name + ": n = " + std::to_string(n) + " is above the device cap " +
              std::to_string(SUP_CPLX_EXACT_MAX_DEVICE_N) +
              " (SUP_CPLX_EXACT_MAX_DEVICE_N: the largest order whose kernel needs no scratch memory; on_cpu = 1 "
              "runs host threads up to n = 64)");
    return SUP_EUNSUPPORTED;
  }
  if (whole && zero_row) {
    S.zero_row = true;
    return SUP_OK;
  }
  // |Re X_j|, |Im X_j| <= maxrow < 2^xbits.  The row bounds are below 2^31, so
  // xbits <= 31 and G = 1 always has pbits = min(42, 51 - xbits) >= 20; G = 2
  // needs 51 - (2 xbits + 1) >= 20, xbits <= 15.  G trades the shared pair
  // products (4 floor(n/2) per step) and smaller primes (more of them, more
  // launches of kMaxCxPrimes) against half the chain (10 per group and prime).
  const int xbits = (int)std::ceil(std::log2(maxrow + 1.0));
  int group = 0, pbits = 0;
  if (want_group) {
    group = want_group, pbits = cxe_pbits(want_group, xbits);
    if (pbits < 20) {
      set_error(name + ": group = " + std::to_string(want_group) + " with xbits = " + std::to_string(xbits) +
                " (row bounds below 2^xbits) leaves primes of " + std::to_string(pbits) +
                " bits; at least 20 are needed");
      return SUP_EINVAL;
    }
  } else {
    double best = 1e300;
    for (int G : {1, 2}) {
      const int pb = cxe_pbits(G, xbits);
      if (pb < 20) continue;
      const double need = std::ceil((logT + 3.0) / (pb - 0.5));
      const double launches = std::ceil(need / kMaxCxPrimes);
      const double ops = launches * cxe_ops_per_step(n, G, 0) + need * (10.0 * ((n + G - 1) / G) - 2.0);
      if (ops < best) best = ops, group = G, pbits = pb;
    }
    if (group == 0) {  // not reachable within the input limits (G = 1 above)
      set_error(name + ": xbits = " + std::to_string(xbits) + " leaves no group size with primes of 20 bits");
      return SUP_EINVAL;
    }
  }
  exact_take_primes(pbits, logT + 3.0, S.primes);  // product > 8 x the bound on |T|
  S.group = group;
  std::vector<double> A2(2 * (size_t)n * n);
  for (size_t i = 0; i < A2.size(); ++i) A2[i] = 2.0 * A[i];
  return cplx_plan(A2.data(), n, o, S.P, S.x0c);
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

// An exact integer-valued |v| < 2^53 as a residue in [0, p).
inline uint64_t to_res(double v, uint64_t p) {
  const int64_t i = (int64_t)v % (int64_t)p;
  return (uint64_t)(i < 0 ? i + (int64_t)p : i);
}

// Every prime of the walk on device `dev`, kMaxCxPrimes per launch.
int device_range(int dev, const CxExactSetup& S, uint64_t c0, uint64_t c1, std::vector<uint64_t>& re,
                 std::vector<uint64_t>& im, double* kernel_ms, int* grid) {
  const int np = (int)S.primes.size();
  re.assign(np, 0), im.assign(np, 0);
  for (int q0 = 0; q0 < np; q0 += kMaxCxPrimes) {
    const std::vector<double> pr(S.primes.begin() + q0, S.primes.begin() + std::min(np, q0 + kMaxCxPrimes));
    std::vector<uint64_t> r, i;
    double ms = 0.0;
    if (int rc = run_range_cplxexact(dev, S.P, S.x0c, S.group, c0, c1, pr, r, i, &ms, grid)) return rc;
    std::copy(r.begin(), r.end(), re.begin() + q0);
    std::copy(i.begin(), i.end(), im.begin() + q0);
    *kernel_ms += ms;
  }
  return SUP_OK;
}

void fill_info(CplxExactInfo* info, const CxExactSetup& S, const CplxInfo& ci) {
  if (!info) return;
  info->ci = ci;
  info->group = S.group;
  info->est_ops = cxe_ops_per_step(S.P.n, S.group, std::min((int)S.primes.size(), kMaxCxPrimes));
}

}  // namespace

// walk_cplxexact.hip on host threads: the states, the group products, the
// chains, the signed accumulate and a fold at least every 256 steps are the
// kernel's (the kernel starts a chunk one column back and makes step 0 an
// even step of its loop: the same integers); a lane's residues go straight
// into the thread's sums.
void cpu_cplx_exact_range(const Plan& P, const std::vector<double>& x0c, int group, uint64_t c0, uint64_t c1,
                          const std::vector<double>& primes, int threads, std::vector<uint64_t>& res_re,
                          std::vector<uint64_t>& res_im) {
  const int np = (int)primes.size(), n = P.n, NP = P.NP, L = P.lay.L;
  const int K = (n + group - 1) / group;
  res_re.assign(np, 0), res_im.assign(np, 0);
  if (c1 <= c0) return;
  const uint64_t count = c1 - c0;
  const uint32_t T = 1u << P.lay.m;
  const size_t plane = P.cols.size() / 2;
  const double* re = P.cols.data();
  const double* im = re + plane;
  const int TH = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)std::max(threads, 1), count));
  std::vector<std::vector<uint64_t>> part(TH, std::vector<uint64_t>(2 * (size_t)np, 0));
  std::vector<std::thread> th;
  for (int w = 0; w < TH; ++w)
    th.emplace_back([&, w]() {
      std::vector<double> pinv(np);
      for (int q = 0; q < np; ++q) pinv[q] = 1.0 / primes[q];
      std::vector<cx> x(n), y(K), acc(np);
      auto add_col = [&](size_t off, bool on) {
        for (int r = 0; r < n; ++r) x[r] = cx_add_d2(x[r], on ? re[off + r] : 0.0, on ? im[off + r] : 0.0);
      };
      // sign +1: acc += term, -1: acc -= term, 0: acc = term
      auto terms = [&](int sign) {
        for (int k = 0; k < K; ++k) y[k] = (group == 2 && 2 * k + 1 < n) ? cx_mul(x[2 * k], x[2 * k + 1]) : x[k * group];
        for (int q = 0; q < np; ++q) {
          cx r = cxe_red2(y[0], primes[q], pinv[q]);
          for (int k = 1; k < K; ++k) r = cxe_link(r, y[k], primes[q], pinv[q]);
          acc[q] = sign == 0 ? r : sign > 0 ? cx_add(acc[q], r) : cx_sub(acc[q], r);
        }
      };
      for (uint64_t a = (uint64_t)w; a < count; a += (uint64_t)TH) {
        const uint64_t ga = c0 + a;
        for (uint32_t lane = 0; lane < (1u << L); ++lane) {
          for (int r = 0; r < n; ++r) x[r] = cx{x0c[r], x0c[NP + r]};
          uint64_t h = ga ^ (ga >> 1);
          while (h) {
            const int b = __builtin_ctzll(h);
            h &= h - 1;
            add_col((size_t)(2 * (L + P.lay.m + b)) * NP, true);
          }
          for (int e = 0; e < L; ++e) add_col((size_t)(2 * e) * NP, (lane >> e) & 1u);
          terms(0);
          for (uint32_t t0 = 1; t0 < T; t0 += 256u) {
            const uint32_t lim = t0 + 256u < T ? t0 + 256u : T;
            for (uint32_t t = t0; t + 1 < lim; t += 2) {
              add_col((size_t)(2 * L + ((t >> 1) & 1u)) * NP, true);
              terms(-1);
              const uint32_t u = t + 1;
              const uint32_t k = (uint32_t)__builtin_ctz(u);
              const uint32_t neg = (u >> (k + 1)) & 1u;
              add_col((size_t)(2 * L + 2u * k + neg) * NP, true);
              terms(+1);
            }
            for (int q = 0; q < np; ++q) acc[q] = cxe_red2(acc[q], primes[q], pinv[q]);
          }
          if (T > 1u) {
            add_col((size_t)(2 * L + (((T - 1u) >> 1) & 1u)) * NP, true);
            terms(-1);
          }
          const bool flip = (((uint32_t)ga ^ (uint32_t)__builtin_popcount(lane)) & 1u) != 0;
          for (int q = 0; q < np; ++q) {
            const uint64_t pq = (uint64_t)primes[q];
            const cx v = cxe_red2(acc[q], primes[q], pinv[q]);
            const uint64_t vr = to_res(v.re, pq), vi = to_res(v.im, pq);
            part[w][2 * q] = (part[w][2 * q] + (flip ? (pq - vr) % pq : vr)) % pq;
            part[w][2 * q + 1] = (part[w][2 * q + 1] + (flip ? (pq - vi) % pq : vi)) % pq;
          }
        }
      }
    });
  for (auto& t : th) t.join();
  for (int q = 0; q < np; ++q) {
    const uint64_t pq = (uint64_t)primes[q];
    for (int w = 0; w < TH; ++w) {
      res_re[q] = (res_re[q] + part[w][2 * q]) % pq;
      res_im[q] = (res_im[q] + part[w][2 * q + 1]) % pq;
    }
  }
}

int cplx_exact_perman_range(const double* A, int n, uint64_t c0, uint64_t c1, const sup_opts& o, bool on_cpu,
                            int group, int cap, std::vector<uint64_t>& primes, std::vector<uint64_t>& res_re,
                            std::vector<uint64_t>& res_im, CplxExactInfo* info) {
  const char* who = "sup_perman_complex_exact_range";
  CxExactSetup S;
  int rc = cplx_exact_setup(A, n, o, on_cpu, false, group, who, S);
  if (rc) return rc;
  const Plan& P = S.P;
  if (c0 > c1 || c1 > P.lay.chunks()) {
    set_error("wave-chunk range [c0, c1) must satisfy c0 <= c1 <= " + std::to_string(P.lay.chunks()) +
              " (the plan's chunks)");
    return SUP_EINVAL;
  }
  const int np = (int)S.primes.size();
  if (cap < np) {  // before any walk
    set_error(std::string(who) + ": cap = " + std::to_string(cap) + " but this walk has " + std::to_string(np) +
              " primes");
    return SUP_EINVAL;
  }
  primes.resize(np);
  for (int q = 0; q < np; ++q) primes[q] = (uint64_t)S.primes[q];
  CplxInfo ci;
  ci.lay = P.lay;
  if (on_cpu) {
    cpu_cplx_exact_range(P, S.x0c, S.group, c0, c1, S.primes, std::max(o.threads, 1), res_re, res_im);
  } else {
    int ndev = 0;
    if ((rc = need_device(o, who, &ndev))) return rc;
    if ((rc = device_range(o.device_id, S, c0, c1, res_re, res_im, &ci.kernel_ms, &ci.grid))) return rc;
    ci.devices = 1;
  }
  fill_info(info, S, ci);
  return SUP_OK;
}

int cplx_exact_perman(const double* A, int n, const sup_opts& o, bool on_cpu, std::string& re, std::string& im,
                      CplxExactInfo* info) {
  const char* who = "sup_perman_complex_exact";
  CxExactSetup S;
  int rc = cplx_exact_setup(A, n, o, on_cpu, true, 0, who, S);
  if (rc) return rc;
  if (S.zero_row) {
    re = im = "0";
    if (info) *info = CplxExactInfo{};
    return SUP_OK;
  }
  const Plan& P = S.P;
  const uint64_t C = P.lay.chunks();
  const int np = (int)S.primes.size();
  std::vector<uint64_t> res_re(np, 0), res_im(np, 0);
  CplxInfo ci;
  ci.lay = P.lay;
  if (on_cpu) {
    cpu_cplx_exact_range(P, S.x0c, S.group, 0, C, S.primes, std::max(o.threads, 1), res_re, res_im);
  } else {
    int ndev = 0;
    if ((rc = need_device(o, who, &ndev))) return rc;
    const int G =
        (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)std::max(1, std::min(o.gpu_num, ndev - o.device_id)), C));
    std::vector<int> drc(G, SUP_OK), dgrid(G, 0);
    std::vector<double> dms(G, 0.0);
    std::vector<std::string> derr(G);  // g_err is thread_local: carry worker messages back
    std::vector<std::vector<uint64_t>> dre(G), dim(G);
    auto work = [&](int g) {
      const uint64_t a = C * (uint64_t)g / (uint64_t)G, b = C * (uint64_t)(g + 1) / (uint64_t)G;
      drc[g] = device_range(o.device_id + g, S, a, b, dre[g], dim[g], &dms[g], &dgrid[g]);
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
    for (int q = 0; q < np; ++q) {
      const uint64_t pq = (uint64_t)S.primes[q];
      for (int g = 0; g < G; ++g) {
        res_re[q] = (res_re[q] + dre[g][q]) % pq;
        res_im[q] = (res_im[q] + dim[g][q]) % pq;
      }
    }
    ci.kernel_ms = *std::max_element(dms.begin(), dms.end());
    ci.grid = dgrid[0];
    ci.devices = G;
  }
  if ((rc = exact_crt_perman(S.primes, res_re, n, "sup_perman_complex_exact (Re)", re))) return rc;
  if ((rc = exact_crt_perman(S.primes, res_im, n, "sup_perman_complex_exact (Im)", im))) return rc;
  fill_info(info, S, ci);
  return SUP_OK;
}

}  // namespace sup
