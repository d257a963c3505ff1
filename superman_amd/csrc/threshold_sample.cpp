// threshold_sample.cpp — a threshold-detector Gaussian boson sampler for pure
// states (sup_threshold_sample): gbs.cpp's chain rule with click / no-click
// outcomes, batched over the samples, on the ragged loop torontonian batch
// (loop_torontonian_each; loop_torontonian.cpp, walk_ltor.hip).  DESIGN.md §8p.
//
// The state is (B, zeta) as in gbs.cpp; het[s] holds the heterodyne outcomes
// alpha_0 .. alpha_{M-1} of sample s, drawn by the caller.  One matrix serves
// every step and every sample: O = [[0, B], [conj B, 0]] (2M x 2M; the state of
// modes 0 .. k given alpha_{k+1 ..} has the leading block of B, so its O is a
// principal submatrix of this one).  Sample s, for mode k = 0 .. M-1, with C
// the modes among 0 .. k-1 that clicked, ascending:
//   z_i = zeta_i + sum_{j > k} B_ij conj(alpha_j),  i <= k   (gbs.cpp's fma sequence)
//   gamma = (z, conj z): entry i is z_i, entry i + M its conjugate, zero above k
//   w_0 = ltor(O, gamma, C),  w_1 = ltor(O, gamma, C + [k])
//         a weight that is negative or -0 counts as +0 (the rounding of an
//         alternating sum); a NaN stays
//   u   = (word64(seed, sample0 + s, k) >> 11) 2^-53
//   click_k = the first c whose running sum of w (ascending, from 0.0) exceeds
//         u (w_0 + w_1); a zero weight is never chosen; when rounding leaves
//         none, the last c with w_c > 0.
// The prefactor of the conditional state cancels in w_1 / (w_0 + w_1).  A sum
// that is zero or not finite, or a step whose longer list would pass 32 modes:
// that mode and every later one of the sample are -1.
// Every mode step gathers two items per sample of a batch into one
// loop_torontonian_each call; both share the sample's one row gamma.  The loop
// torontonians are bit-identical on the device and the host twin and
// everything else runs on the host for both, so both draw identical samples,
// and sample s depends on (B, zeta[s], het[s], seed, sample0 + s) only.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "approx_core.hpp"
#include "engine.hpp"
#include "loop_torontonian.hpp"

namespace sup {

int threshold_sample(const double* B, int M, const double* zeta, const double* het, uint64_t nsamples, uint64_t sample0,
                     uint64_t seed, const sup_opts& o, bool on_cpu, int32_t* out, double* weights, ThrInfo* info) {
  const std::string who = "sup_threshold_sample";
  using clk = std::chrono::steady_clock;
  auto ms_since = [](clk::time_point t) { return std::chrono::duration<double, std::milli>(clk::now() - t).count(); };
  ThrInfo gi;
  if (info) *info = gi;
  if (!B) {
    set_error(who + ": null matrix");
    return SUP_EINVAL;
  }
  if (M < 1 || M > SUP_MAX_N) {
    set_error(who + ": M = " + std::to_string(M) + " outside [1, 64]");
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
    const size_t ld = 2 * (size_t)M;
    std::vector<double> O(2 * ld * ld, 0.0);
    for (int i = 0; i < M; ++i)
      for (int j = 0; j < M; ++j) {
        const double br = B[2 * ((size_t)i * M + j)], bi = B[2 * ((size_t)i * M + j) + 1];
        O[2 * ((size_t)i * ld + M + j)] = br, O[2 * ((size_t)i * ld + M + j) + 1] = bi;
        O[2 * ((size_t)(M + i) * ld + j)] = br, O[2 * ((size_t)(M + i) * ld + j) + 1] = -bi;
      }
    std::vector<int32_t> clicks(nsamples, 0);  // clicks so far; -1: the sample failed
    std::vector<double> gam, vals;
    std::vector<int32_t> lists, ns, gamma_of;
    std::vector<uint64_t> who_s;  // the samples of the batch
    double ops_sum = 0.0;
    auto fail = [&](uint64_t q, int k) {
      for (int i = k; i < M; ++i) out[q * M + i] = -1;
      if (weights)
        for (int i = k; i < M; ++i) weights[2 * (q * M + i)] = weights[2 * (q * M + i) + 1] = 0.0;
      clicks[q] = -1;
      ++gi.failed;
    };
    for (int k = 0; k < M; ++k) {
      for (uint64_t s = 0; s < nsamples;) {
        // ---- host stage: a batch of samples, their gamma rows and their two lists ----
        auto t_host = clk::now();
        int32_t maxc = 0;
        for (uint64_t q = s; q < nsamples; ++q) maxc = std::max(maxc, clicks[q]);
        const int stride = std::min(kTorMaxN, (int)maxc + 1);
        gam.clear(), lists.clear(), ns.clear(), gamma_of.clear(), who_s.clear();
        size_t bytes = 0;
        std::vector<int32_t> list((size_t)stride, 0);
        for (; s < nsamples; ++s) {
          if (clicks[s] < 0) continue;
          const int32_t c = clicks[s];
          if (c + 1 > kTorMaxN) {  // the list with mode k would pass 32 modes
            fail(s, k);
            continue;
          }
          const size_t add = (c > 0 ? ltor_item_bytes(c, stride) : 0) + ltor_item_bytes(c + 1, stride);
          if (!who_s.empty() && bytes + add > ltor_slab_cap_bytes()) break;
          bytes += add;
          int len = 0;
          for (int i = 0; i < k; ++i)
            if (out[s * M + i] == 1) list[len++] = i;
          list[len] = k;
          for (int j = len + 1; j < stride; ++j) list[j] = 0;
          const int32_t row = (int32_t)who_s.size();
          who_s.push_back(s);
          const double* zs = zeta + 2 * (size_t)M * s;
          const double* al = het + 2 * (size_t)M * s;
          const size_t g0 = gam.size();
          gam.resize(g0 + 4 * (size_t)M, 0.0);
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
            gam[g0 + 2 * i] = re, gam[g0 + 2 * i + 1] = im;
            gam[g0 + 2 * (M + i)] = re, gam[g0 + 2 * (M + i) + 1] = -im;
          }
          for (int t = 0; t < 2; ++t) {
            lists.insert(lists.end(), list.begin(), list.end());
            ns.push_back(c + t);
            gamma_of.push_back(row);
          }
        }
        gi.host_ms += ms_since(t_host);
        if (who_s.empty()) continue;
        // ---- one ragged call for the batch ----
        auto t_each = clk::now();
        vals.assign(ns.size(), 0.0);
        LtorEachIn in;
        in.O = O.data(), in.M = M, in.gamma = gam.data(), in.ngamma = who_s.size(), in.gamma_of = gamma_of.data();
        in.modes = lists.data(), in.stride = stride, in.n = ns.data();
        TorInfo ti;
        if (int rc = loop_torontonian_each(in, ns.size(), o, on_cpu, vals.data(), &ti)) return rc;
        gi.each_ms += ms_since(t_each);
        gi.kernel_ms += ti.kernel_ms;
        gi.visited += ti.subsets;
        ops_sum += ti.ops * (double)ti.subsets;
        gi.devices = std::max(gi.devices, ti.devices);
        // ---- host stage: the weights and the draw ----
        t_host = clk::now();
        size_t item = 0;
        for (const uint64_t q : who_s) {
          double w[2];
          for (int c = 0; c < 2; ++c) {
            w[c] = vals[item++];
            if (w[c] < 0.0 || w[c] == 0.0) w[c] = 0.0;  // negative or -0: +0; a NaN stays
          }
          if (weights) weights[2 * (q * M + k)] = w[0], weights[2 * (q * M + k) + 1] = w[1];
          double tot = 0.0;
          for (int c = 0; c < 2; ++c) tot += w[c];
          if (!(tot > 0.0) || !std::isfinite(tot)) {
            fail(q, k);
            if (weights) weights[2 * (q * M + k)] = w[0], weights[2 * (q * M + k) + 1] = w[1];
            continue;
          }
          const double u = (double)(word64(seed, sample0 + q, (uint32_t)k) >> 11) * 0x1p-53;
          const double target = u * tot;
          double run = 0.0;
          int pick = -1;
          for (int c = 0; c < 2 && pick < 0; ++c) {
            run += w[c];
            if (run > target) pick = c;
          }
          if (pick < 0)  // rounding left no c: the last one with a positive weight
            for (int c = 0; c < 2; ++c)
              if (w[c] > 0.0) pick = c;
          out[q * M + k] = pick;
          clicks[q] += pick;
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
