// gbs.cpp — a photon-number-resolving Gaussian boson sampler for pure states
// (sup_gbs_sample): the chain rule of Bulmer et al. 2022 ("The boundary for
// quantum advantage in Gaussian boson sampling", Sci. Adv. 8, eabl9236),
// batched over the samples, on the ragged loop-hafnian batch
// (loop_hafnian_each; hafnian.cpp, walk_lhafe.hip).  DESIGN.md §8n.
//
// The state is (B, zeta): B the M x M symmetric matrix of the pure state's
// amplitudes, zeta[s] the displacement of sample s (one row per sample, so a
// later mixed-state split can hand every sample its own).  het[s] holds the
// heterodyne outcomes alpha_0 .. alpha_{M-1} of sample s, drawn by the caller:
// this entry is deterministic.  Sample s, for mode k = 0 .. M-1, with the
// outcomes n_0 .. n_{k-1} drawn so far (N their sum):
//   z_i = zeta_i + sum_{j > k} B_ij conj(alpha_j),  i <= k
//         j ascending, one fma per part, in this order per j:
//         re = fma(Bre, are, re);  re = fma(Bim, aim, re);
//         im = fma(Bim, are, im);  im = fma(-Bre, aim, im)
//   w_c = |lhaf(B; n_i copies of i for i < k, then c copies of k; diagonal z)|^2 / c!
//         for c = 0 .. cutoff; an order N + c above 64 is not evaluated: w_c = 0
//   u   = (word64(seed, sample0 + s, k) >> 11) 2^-53
//   n_k = the first c whose running sum of w (ascending, from 0.0) exceeds
//         u tot, tot the sum of w ascending from 0.0; the running sum only
//         moves at w_c > 0, so no c with w_c = 0 is chosen; when rounding leaves
//         none, the last c with w_c > 0.
// tot zero or not finite: n_k and every later mode of the sample are -1.
// Renormalising over c <= cutoff is the only approximation of the law.
// Every mode step gathers the candidates (sample, c) of a batch of samples into
// one loop_hafnian_each call: cutoff + 1 items share the sample's one row z.
// The loop hafnians are bit-identical on the device and the host twin and
// everything else runs on the host for both, so both draw identical samples,
// and sample s depends on (B, zeta[s], het[s], cutoff, seed, sample0 + s) only.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "approx_core.hpp"
#include "engine.hpp"

namespace sup {

int gbs_sample(const double* B, int M, const double* zeta, const double* het, int cutoff, uint64_t nsamples,
               uint64_t sample0, uint64_t seed, const sup_opts& o, bool on_cpu, int32_t* out, GbsInfo* info) {
  const std::string who = "sup_gbs_sample";
  using clk = std::chrono::steady_clock;
  auto ms_since = [](clk::time_point t) { return std::chrono::duration<double, std::milli>(clk::now() - t).count(); };
  GbsInfo gi;
  if (info) *info = gi;
  if (!B) {
    set_error(who + ": null matrix");
    return SUP_EINVAL;
  }
  if (M < 1 || M > SUP_MAX_N) {
    set_error(who + ": M = " + std::to_string(M) + " outside [1, 64]");
    return SUP_EINVAL;
  }
  if (cutoff < 0 || cutoff > SUP_MAX_N) {
    set_error(who + ": cutoff = " + std::to_string(cutoff) + " outside [0, 64]");
    return SUP_EINVAL;
  }
  for (int i = 0; i < M; ++i)
    for (int j = 0; j < i; ++j)
      if (std::memcmp(B + 2 * ((size_t)i * M + j), B + 2 * ((size_t)j * M + i), 2 * sizeof(double)) != 0) {
        set_error(who + ": B[" + std::to_string(j) + "][" + std::to_string(i) + "] and B[" + std::to_string(i) + "][" +
                  std::to_string(j) + "] differ: B must be symmetric bit for bit");
        return SUP_EINVAL;
      }
  if (nsamples == 0) return SUP_OK;
  if (!zeta || !het || !out) {
    set_error(who + ": null pointer");
    return SUP_EINVAL;
  }
  if (!on_cpu) {
    int ndev = 0;
    if (int rc = device_count(&ndev)) return rc;
    if (ndev == 0) {
      set_error("no HIP device available (" + who + " has no CPU fallback; on_cpu = 1 runs host threads)");
      return SUP_ENODEV;
    }
  }
  try {
    const int C1 = cutoff + 1;
    double fact[SUP_MAX_N + 1];
    fact[0] = 1.0;
    for (int i = 1; i <= SUP_MAX_N; ++i) fact[i] = fact[i - 1] * (double)i;
    std::vector<int32_t> total(nsamples, 0);  // photons drawn so far; -1: the sample failed
    std::vector<double> z, vals, w(C1);
    std::vector<int32_t> idx, ns, mu_of;
    std::vector<uint64_t> who_s;  // the samples of the batch
    double ops_sum = 0.0;
    for (int k = 0; k < M; ++k) {
      for (uint64_t s = 0; s < nsamples;) {
        // ---- host stage: a batch of samples, their z rows and candidate lists ----
        auto t_host = clk::now();
        int32_t maxn = 0;
        for (uint64_t q = s; q < nsamples; ++q) maxn = std::max(maxn, total[q]);
        const int stride = std::min(SUP_MAX_N, (int)maxn + cutoff);
        z.clear(), idx.clear(), ns.clear(), mu_of.clear(), who_s.clear();
        size_t bytes = 0;
        std::vector<int32_t> list((size_t)std::max(stride, 1), 0);
        for (; s < nsamples; ++s) {
          if (total[s] < 0) continue;
          const int32_t N = total[s];
          int len = 0;
          for (int i = 0; i < k; ++i)
            for (int32_t c = 0; c < out[s * M + i]; ++c) list[len++] = i;
          for (int j = len; j < stride; ++j) list[j] = k;
          size_t add = 0;
          for (int c = 0; c < C1 && N + c <= SUP_MAX_N; ++c)
            if (N + c > 0) add += haf_item_bytes(list.data(), N + c);
          if (!who_s.empty() && bytes + add > haf_slab_cap_bytes()) break;
          bytes += add;
          const int32_t row = (int32_t)who_s.size();
          who_s.push_back(s);
          const double* zs = zeta + 2 * (size_t)M * s;
          const double* al = het + 2 * (size_t)M * s;
          const size_t z0 = z.size();
          z.resize(z0 + 2 * (size_t)M, 0.0);
          for (int i = 0; i <= k; ++i) {
            double re = zs[2 * i], im = zs[2 * i + 1];
            for (int j = k + 1; j < M; ++j) {
              const double br = B[2 * ((size_t)i * M + j)], bi = B[2 * ((size_t)i * M + j) + 1];
              const double ar = al[2 * j], ai = al[2 * j + 1];
              re = __builtin_fma(br, ar, re);
              re = __builtin_fma(bi, ai, re);
              im = __builtin_fma(bi, ar, im);
              im = __builtin_fma(-br, ai, im);
            }
            z[z0 + 2 * i] = re, z[z0 + 2 * i + 1] = im;
          }
          for (int c = 0; c < C1 && N + c <= SUP_MAX_N; ++c) {
            idx.insert(idx.end(), list.begin(), list.end());
            ns.push_back(N + c);
            mu_of.push_back(row);
          }
        }
        gi.host_ms += ms_since(t_host);
        if (who_s.empty()) continue;
        // ---- one ragged call for the batch ----
        auto t_each = clk::now();
        vals.assign(2 * ns.size(), 0.0);
        HafEachIn in;
        in.A = B, in.M = M, in.mu = z.data(), in.nmu = who_s.size(), in.mu_of = mu_of.data();
        in.idx = idx.data(), in.stride = (int)list.size(), in.n = ns.data();
        HafInfo hi;
        if (int rc = loop_hafnian_each(in, ns.size(), o, on_cpu, vals.data(), &hi)) return rc;
        gi.each_ms += ms_since(t_each);
        gi.kernel_ms += hi.kernel_ms;
        gi.visited += hi.terms;
        ops_sum += hi.ops * (double)hi.terms;
        gi.devices = std::max(gi.devices, hi.devices);
        // ---- host stage: the weights and the draw ----
        t_host = clk::now();
        size_t item = 0;
        for (const uint64_t q : who_s) {
          const int32_t N = total[q];
          double tot = 0.0;
          for (int c = 0; c < C1; ++c) {
            if (N + c <= SUP_MAX_N) {
              const double re = vals[2 * item], im = vals[2 * item + 1];
              ++item;
              const double rr = re * re, ii = im * im;
              w[c] = (rr + ii) / fact[c];
            } else {
              w[c] = 0.0;
            }
            tot += w[c];
          }
          if (!(tot > 0.0) || !std::isfinite(tot)) {
            for (int i = k; i < M; ++i) out[q * M + i] = -1;
            total[q] = -1;
            ++gi.failed;
            continue;
          }
          const double u = (double)(word64(seed, sample0 + q, (uint32_t)k) >> 11) * 0x1p-53;
          const double target = u * tot;
          double run = 0.0;
          int pick = -1;
          for (int c = 0; c < C1 && pick < 0; ++c) {
            run += w[c];
            if (run > target) pick = c;
          }
          if (pick < 0)  // rounding left no c: the last one with a positive weight
            for (int c = 0; c < C1; ++c)
              if (w[c] > 0.0) pick = c;
          out[q * M + k] = pick;
          total[q] = N + pick;
        }
        gi.host_ms += ms_since(t_host);
      }
    }
    gi.ops = gi.visited ? ops_sum / (double)gi.visited : 0.0;
  } catch (const std::bad_alloc&) {
    set_error(who + ": out of host memory for a step's lists");
    return SUP_ENOMEM;
  }
  if (info) *info = gi;
  return SUP_OK;
}

}  // namespace sup
