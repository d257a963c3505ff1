// boson.cpp — an exact boson sampler (sup_boson_sample): Clifford & Clifford
// 2018 ("The classical complexity of boson sampling", SODA'18), algorithm A,
// batched over the samples, on the one-walk permanent minors (cplx_minors.cpp).
//
// n photons enter the M x M unitary U in the distinct modes inputs[0..n).
// Sample s:
//   alpha = a uniform permutation of `inputs` (Fisher-Yates);
//   for k = 1..n the output mode r_k is drawn from
//     w_i = |per U[(r_1..r_{k-1}, i), (alpha_1..alpha_k)]|^2,  i < M,
//   which by Laplace expansion along the new row i is
//     w_i = |sum_l U[i][alpha_l] per(B without row l)|^2,
//     B[l][c] = U[r_c][alpha_l]   (k rows, k - 1 columns):
//   the k minors of one matrix, for all samples in one cplx_minors call of
//   order parameter k on U^T with rows = alpha_s[0..k), cols = r_s[0..k-1);
//   the output row is r sorted ascending.
// The marginal lemma behind the stage-wise pmf needs orthonormal columns: the
// inputs must be distinct and the n used columns of U orthonormal to 1e-8.
//
// Randomness (Philox4x32-10, approx_core.hpp draw(seed, s, step); w64 = v[0] |
// v[1] << 32 of that draw):
//   shuffle  t = 0 .. n-2, i = n-1-t: j = floor(w64(step t) (i + 1) / 2^64),
//            swap(alpha[i], alpha[j]); alpha starts as `inputs` in the caller's order
//   stage k  u = (w64(step 64 + k) >> 11) 2^-53, a 53-bit uniform in [0, 1)
// The pmf and the draw run on host threads for both on_cpu values, in one
// order: amp = cx_mul(U[i][alpha_0], minor_0), then amp = cx_add(amp,
// cx_mul(U[i][alpha_l], minor_l)) for l ascending; w_i = amp.re amp.re +
// amp.im amp.im (-ffp-contract=off); tot = sum of w ascending from 0.0; r_k =
// the first i whose running sum (ascending, from 0.0) exceeds u tot — the
// running sum only moves at w_i > 0, so no i with w_i = 0 is chosen; when
// rounding leaves none, the last i with w_i > 0.  The minors are bit-identical
// on the device and the host twin, so both draw identical samples, and sample
// s depends on (U, inputs, seed, s) only.
//
// sup_boson_sample_fock is the same function with one switch: every stage's
// minors come from cplx_fock_minors (cplx_fock_minors.cpp), whose
// walk collapses the repeated modes among the k - 1 drawn so far.  Its minors
// differ from cplx_minors' in their last bits, so a draw can differ where
// u tot lies within rounding of a running sum; everything else is shared.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <new>
#include <string>
#include <thread>

#include "approx_core.hpp"
#include "cx.hpp"
#include "engine.hpp"

namespace sup {

namespace {

// fn(first, last) over [0, count) split into contiguous ranges on up to T threads.
template <class Fn>
void parallel_ranges(uint64_t count, int T, const Fn& fn) {
  T = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)std::max(T, 1), count));
  std::vector<std::thread> th;
  for (int w = 1; w < T; ++w) th.emplace_back([&, w]() { fn(count * (uint64_t)w / T, count * (uint64_t)(w + 1) / T); });
  fn(0, count / (uint64_t)T);
  for (auto& t : th) t.join();
}

}  // namespace

int boson_sample(const double* U, int M, const int32_t* inputs, int n, uint64_t nsamples, uint64_t seed,
                 const sup_opts& o, bool on_cpu, int32_t* out, BosonInfo* info, bool collision_aware) {
  const char* who = collision_aware ? "sup_boson_sample_fock" : "sup_boson_sample";
  if (!U || !inputs || !out) {
    set_error(std::string(who) + ": null pointer");
    return SUP_EINVAL;
  }
  if (n > 32) {
    set_error(std::string(who) + ": n = " + std::to_string(n) + " photons: more than 32 are not provided");
    return SUP_EUNSUPPORTED;
  }
  if (n < 1 || M < 1) {
    set_error(std::string(who) + ": n = " + std::to_string(n) + ", M = " + std::to_string(M) + " (both must be >= 1)");
    return SUP_EINVAL;
  }
  if (o.walk_log2 < 0 || o.walk_log2 > 31) {
    set_error("walk_log2 = " + std::to_string(o.walk_log2) + " outside [0, 31] (0 = default layout)");
    return SUP_EINVAL;
  }
  for (int a = 0; a < n; ++a) {
    if (inputs[a] < 0 || inputs[a] >= M) {
      set_error(std::string(who) + ": inputs[position " + std::to_string(a) + "] = " + std::to_string(inputs[a]) +
                " outside [0, " + std::to_string(M) + ")");
      return SUP_EINVAL;
    }
    for (int b = 0; b < a; ++b)
      if (inputs[b] == inputs[a]) {
        set_error(std::string(who) + ": inputs[position " + std::to_string(a) + "] = " + std::to_string(inputs[a]) +
                  " repeats position " + std::to_string(b) + " (the input modes must be distinct)");
        return SUP_EINVAL;
      }
  }
  // the used columns must be orthonormal: |A^dagger A - I| <= 1e-8 entrywise
  for (int a = 0; a < n; ++a)
    for (int b = 0; b <= a; ++b) {
      double re = 0.0, im = 0.0;
      for (int i = 0; i < M; ++i) {
        const double* x = U + 2 * ((size_t)i * M + inputs[a]);
        const double* y = U + 2 * ((size_t)i * M + inputs[b]);
        re += x[0] * y[0] + x[1] * y[1];  // conj(x) y
        im += x[0] * y[1] - x[1] * y[0];
      }
      const double dr = re - (a == b ? 1.0 : 0.0);
      if (!(std::fabs(dr) <= 1e-8) || !(std::fabs(im) <= 1e-8)) {
        set_error(std::string(who) + ": columns inputs[" + std::to_string(a) + "] and inputs[" + std::to_string(b) +
                  "] of U are not orthonormal to 1e-8 (U must be unitary)");
        return SUP_EINVAL;
      }
    }
  BosonInfo bi;
  if (info) *info = bi;
  if (nsamples == 0) return SUP_OK;
  if (!on_cpu) {
    int ndev = 0;
    if (int rc = device_count(&ndev)) return rc;
    if (ndev == 0) {
      set_error(std::string("no HIP device available (") + who + " has no CPU fallback; on_cpu = 1 runs host threads)");
      return SUP_ENODEV;
    }
  }
  const int T = std::max(o.threads, 1);
  try {
    std::vector<double> Ut(2 * (size_t)M * M);
    for (int i = 0; i < M; ++i)
      for (int j = 0; j < M; ++j) {
        Ut[2 * ((size_t)j * M + i)] = U[2 * ((size_t)i * M + j)];
        Ut[2 * ((size_t)j * M + i) + 1] = U[2 * ((size_t)i * M + j) + 1];
      }
    std::vector<int32_t> alpha(nsamples * n), r(nsamples * n), rows, cols;
    parallel_ranges(nsamples, T, [&](uint64_t s0, uint64_t s1) {
      for (uint64_t s = s0; s < s1; ++s) {
        int32_t* al = &alpha[s * n];
        std::copy(inputs, inputs + n, al);
        for (int t = 0; t + 1 < n; ++t) {
          const int i = n - 1 - t;
          const int j = (int)(((unsigned __int128)word64(seed, s, (uint32_t)t) * (uint64_t)(i + 1)) >> 64);
          std::swap(al[i], al[j]);
        }
      }
    });
    std::vector<double> minors;
    std::atomic<int> bad{0};
    for (int k = 1; k <= n; ++k) {
      rows.assign(nsamples * k, 0);
      cols.assign(std::max<size_t>(1, nsamples * (k - 1)), 0);
      for (uint64_t s = 0; s < nsamples; ++s) {
        std::copy(&alpha[s * n], &alpha[s * n] + k, &rows[s * k]);
        std::copy(&r[s * n], &r[s * n] + (k - 1), &cols[s * (k - 1)]);
      }
      minors.assign(2 * (size_t)nsamples * k, 0.0);
      CplxBatchIn in;
      in.U = Ut.data(), in.R = M, in.C = M, in.rows = rows.data(), in.cols = cols.data();
      CplxInfo ci;
      FockInfo fi;
      const auto t0 = std::chrono::steady_clock::now();
      // the stage's minors: the one walk over all Gray states, or (collision_aware)
      // the walk over the multiplicities of the modes drawn so far
      if (int rc = collision_aware ? cplx_fock_minors(in, k, nsamples, o, on_cpu, minors.data(), &fi)
                                   : cplx_minors(in, k, nsamples, o, on_cpu, minors.data(), &ci))
        return rc;
      const auto t1 = std::chrono::steady_clock::now();
      bi.kernel_ms += collision_aware ? fi.kernel_ms : ci.kernel_ms;
      bi.devices = std::max(bi.devices, collision_aware ? fi.devices : ci.devices);
      if (k >= 2) bi.steps += nsamples << std::max(k - 2, 0);
      if (k >= 2) bi.visited += collision_aware ? fi.terms : nsamples << std::max(k - 2, 0);
      parallel_ranges(nsamples, T, [&](uint64_t s0, uint64_t s1) {
        std::vector<double> w(M);
        for (uint64_t s = s0; s < s1; ++s) {
          const int32_t* al = &alpha[s * n];
          const double* mn = &minors[2 * s * k];
          double tot = 0.0;
          for (int i = 0; i < M; ++i) {
            const double* urow = U + 2 * (size_t)i * M;
            cx amp = cx_mul(cx{urow[2 * al[0]], urow[2 * al[0] + 1]}, cx{mn[0], mn[1]});
            for (int l = 1; l < k; ++l)
              amp = cx_add(amp, cx_mul(cx{urow[2 * al[l]], urow[2 * al[l] + 1]}, cx{mn[2 * l], mn[2 * l + 1]}));
            w[i] = amp.re * amp.re + amp.im * amp.im;
            tot += w[i];
          }
          if (!(tot > 0.0) || !std::isfinite(tot)) {
            bad.store(1, std::memory_order_relaxed);
            r[s * n + k - 1] = 0;
            continue;
          }
          const double u = (double)(word64(seed, s, 64u + (uint32_t)k) >> 11) * 0x1p-53;
          const double target = u * tot;
          double run = 0.0;
          int pick = -1;
          for (int i = 0; i < M && pick < 0; ++i) {
            run += w[i];
            if (run > target) pick = i;
          }
          if (pick < 0)  // rounding left no i: the last one with a positive weight
            for (int i = 0; i < M; ++i)
              if (w[i] > 0.0) pick = i;
          r[s * n + k - 1] = pick;
        }
      });
      const auto t2 = std::chrono::steady_clock::now();
      bi.minors_ms += std::chrono::duration<double, std::milli>(t1 - t0).count();
      bi.pmf_ms += std::chrono::duration<double, std::milli>(t2 - t1).count();
      if (bad.load()) {
        set_error(std::string(who) + ": stage " + std::to_string(k) + " has a zero or non-finite total weight");
        return SUP_EINVAL;
      }
    }
    for (uint64_t s = 0; s < nsamples; ++s) {
      std::copy(&r[s * n], &r[s * n] + n, out + s * n);
      std::sort(out + s * n, out + (s + 1) * n);
    }
  } catch (const std::bad_alloc&) {
    set_error(std::string(who) + ": out of host memory");
    return SUP_ENOMEM;
  }
  if (info) *info = bi;
  return SUP_OK;
}

}  // namespace sup
