// torontonian_table.cpp — every click pattern's torontonian from one walk:
// sup_torontonian_table, sup_loop_torontonian_table and sup_mobius_subsets
// (DESIGN.md §8m).
//
// f(z) of tor.hpp (ltor.hpp) depends on the selected positions only, so the
// table raw[z] = f(z) of one list holds every term of every sub-list's sum, and
// the subset Moebius transform of tortab.hpp turns it into all 2^n
// torontonians.  The checks and the host twin are here: the twin takes f(z)
// from the per-entry twins' chains and runs the transform one stage at a time.
#include "torontonian_table.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "engine.hpp"

namespace sup {

namespace {

// Stage b over elements [i0, i1) of the half-size index space: pair i has its
// low element at insert-zero(i, b).
void mobius_stage(double* t, int b, uint64_t i0, uint64_t i1) {
  const uint64_t low = (1ull << b) - 1ull;
  for (uint64_t i = i0; i < i1; ++i) {
    const uint64_t lo = ((i & ~low) << 1) | (i & low);
    t[lo | (1ull << b)] = mobius_sub(t[lo | (1ull << b)], t[lo]);
  }
}

// The naive stage loop, every stage split over the threads.
void mobius_cpu(double* t, int n, int threads) {
  if (n < 1) return;
  const uint64_t pairs = 1ull << (n - 1);
  const int T = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)std::max(threads, 1), pairs >> 12));
  for (int b = 0; b < n; ++b) {
    std::vector<std::thread> th;
    for (int w = 1; w < T; ++w) th.emplace_back(mobius_stage, t, b, pairs * (uint64_t)w / T, pairs * (uint64_t)(w + 1) / T);
    mobius_stage(t, b, 0, pairs / T);
    for (auto& x : th) x.join();
  }
}

int need_device(const std::string& who, const sup_opts& o) {
  int ndev = 0;
  if (int rc = device_count(&ndev)) return rc;
  if (ndev == 0) {
    set_error("no HIP device available (" + who + " has no CPU fallback; on_cpu = 1 runs host threads)");
    return SUP_ENODEV;
  }
  if (o.device_id < 0 || o.device_id >= ndev) {
    set_error(who + ": device_id out of range");
    return SUP_EINVAL;
  }
  return SUP_OK;
}

}  // namespace

int mobius_shape(int* L, int* K) {
  *L = kMobiusTileBits, *K = kMobiusPassBits;
  const char* e = std::getenv("SUP_MOBIUS_BITS");  // tests, read per call: smaller tiles and passes (the bits do not change)
  if (!e || !*e) return SUP_OK;
  int l = 0, k = 0;
  char tail = 0;
  if (std::sscanf(e, "%d,%d%c", &l, &k, &tail) != 2 || l < kMobiusTileMin || l > kMobiusTileBits || k < kMobiusPassMin ||
      k > kMobiusPassBits) {
    set_error("SUP_MOBIUS_BITS=" + std::string(e) + ": expected L,K with L in [" + std::to_string(kMobiusTileMin) + ", " +
              std::to_string(kMobiusTileBits) + "] and K in [" + std::to_string(kMobiusPassMin) + ", " +
              std::to_string(kMobiusPassBits) + "], the shapes the transform is compiled for");
    return SUP_EINVAL;
  }
  *L = l, *K = k;
  return SUP_OK;
}

int torontonian_table(const LtorIn& in, bool loop, int n, bool transform, const sup_opts& o, bool on_cpu, double* out,
                      TorInfo* info) {
  const std::string who = loop ? "sup_loop_torontonian_table" : "sup_torontonian_table";
  if (!out || !in.O || !in.modes || (loop && !in.gamma)) {
    set_error(who + ": null pointer");
    return SUP_EINVAL;
  }
  if (n < 1 || n > kTorMaxN) {
    set_error(who + ": n = " + std::to_string(n) + " outside [1, 32]");
    return SUP_EINVAL;
  }
  if (in.M < 1) {
    set_error(who + ": O must have at least two rows (M = " + std::to_string(in.M) + ")");
    return SUP_EINVAL;
  }
  for (int j = 0; j < n; ++j) {
    const int32_t v = in.modes[j];
    if (v < 0 || v >= in.M) {
      set_error(who + ": modes[position " + std::to_string(j) + "] = " + std::to_string(v) + " outside [0, " +
                std::to_string(in.M) + ")");
      return SUP_EINVAL;
    }
    for (int i = 0; i < j; ++i)
      if (in.modes[i] == v) {
        set_error(who + ": modes names mode " + std::to_string(v) + " at positions " + std::to_string(i) + " and " +
                  std::to_string(j) + ": the modes of a list must be distinct");
        return SUP_EINVAL;
      }
  }
  if (o.gpu_num > 1) {
    set_error(who + ": gpu_num = " + std::to_string(o.gpu_num) + ": a table is one device's (o->device_id)");
    return SUP_EINVAL;
  }
  int L = 0, K = 0;
  if (int rc = mobius_shape(&L, &K)) return rc;
  if (n > SUP_TORONTONIAN_TABLE_MAX_N) {
    set_error(who + ": n = " + std::to_string(n) + " above SUP_TORONTONIAN_TABLE_MAX_N = " +
              std::to_string(SUP_TORONTONIAN_TABLE_MAX_N) + " (2^n results)");
    return SUP_EUNSUPPORTED;
  }
  TorInfo ti;
  ti.subsets = 1ull << n;
  ti.ops = (loop ? ltor_ops(n) : tor_ops(n)) + 0.5 * n;  // n 2^(n-1) subtractions over 2^n subsets
  if (on_cpu) {
    try {
      if (loop) {
        ltor_table_raw_cpu(in, n, o.threads, out);
      } else {
        TorIn ti_in;
        ti_in.O = in.O, ti_in.M = in.M, ti_in.modes = in.modes;
        tor_table_raw_cpu(ti_in, n, o.threads, out);
      }
      if (transform) mobius_cpu(out, n, o.threads);
    } catch (const std::bad_alloc&) {
      set_error("out of host memory for the torontonian table's matrices");
      return SUP_ENOMEM;
    }
    if (info) *info = ti;
    return SUP_OK;
  }
  if (int rc = need_device(who, o)) return rc;
  if (int rc = run_torontonian_table(o.device_id, in, loop, n, transform, L, K, out, &ti.kernel_ms, &ti.grid)) return rc;
  ti.devices = 1;
  if (info) *info = ti;
  return SUP_OK;
}

int mobius_subsets(double* t, int n, const sup_opts& o, bool on_cpu) {
  if (!t) {
    set_error("sup_mobius_subsets: null pointer");
    return SUP_EINVAL;
  }
  if (n < 0 || n > SUP_TORONTONIAN_TABLE_MAX_N) {
    set_error("sup_mobius_subsets: n = " + std::to_string(n) + " outside [0, " + std::to_string(SUP_TORONTONIAN_TABLE_MAX_N) + "]");
    return SUP_EINVAL;
  }
  int L = 0, K = 0;
  if (int rc = mobius_shape(&L, &K)) return rc;
  if (on_cpu) {
    mobius_cpu(t, n, o.threads);
    return SUP_OK;
  }
  if (int rc = need_device("sup_mobius_subsets", o)) return rc;
  return run_mobius(o.device_id, t, n, L, K);
}

}  // namespace sup
