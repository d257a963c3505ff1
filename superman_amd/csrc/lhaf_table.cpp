// lhaf_table.cpp — every Fock amplitude up to a cutoff from one recurrence:
// sup_loop_hafnian_table and sup_loop_hafnian_table_plan.
//
// lhaftab.hpp states the table and every floating operation of an entry.  The
// checks and the host twin are here: the twin runs that header slab by slab in
// the slabs' order, each slab split over the threads.
#include "lhaf_table.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "engine.hpp"

namespace sup {

namespace {

struct HostTab {
  const double* t;
  cx load(uint32_t x) const { return cx{t[2 * (size_t)x], t[2 * (size_t)x + 1]}; }
};

struct SlabJob {
  double* t;
  const LhafModes* md;
  const double* arow;
  cx zeta_p;
  const double* s;
  double rc;
  int p;
  uint32_t c, S;
};

void slab_range(SlabJob jb, uint32_t y0, uint32_t y1) {
  const HostTab tab{jb.t};
  for (uint32_t y = y0; y < y1; ++y) {
    const cx v = lhaf_tab_entry(tab, *jb.md, jb.arow, jb.zeta_p, jb.s, jb.rc, jb.p, jb.c, jb.S, y);
    const size_t x = (size_t)jb.c * jb.S + y;
    jb.t[2 * x] = v.re, jb.t[2 * x + 1] = v.im;
  }
}

void table_cpu(const double* A, int M, const double* zeta, const int32_t* dims, int threads, double* t) {
  double s[kLhafTabMaxDim], r[kLhafTabMaxDim];
  lhaf_roots(s, r);
  const LhafModes md = lhaf_modes(dims, M);
  t[0] = 1.0, t[1] = 0.0;
  for (int p = 0; p < M; ++p) {
    const uint32_t S = md.stride[p];
    const uint32_t T = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)std::max(threads, 1), S >> 12));
    for (uint32_t c = 1; c < (uint32_t)dims[p]; ++c) {
      const SlabJob jb{t, &md, A + 2 * (size_t)p * M, cx{zeta[2 * p], zeta[2 * p + 1]}, s, r[c], p, c, S};
      std::vector<std::thread> th;
      for (uint32_t w = 1; w < T; ++w)
        th.emplace_back(slab_range, jb, (uint32_t)((uint64_t)S * w / T), (uint32_t)((uint64_t)S * (w + 1) / T));
      slab_range(jb, 0, S / T);
      for (auto& x : th) x.join();
    }
  }
}

// prod dims, saturating at 2^64 - 1 (dims checked: each in [1, 65]).
uint64_t entries_of(const int32_t* dims, int M) {
  uint64_t e = 1;
  for (int i = 0; i < M; ++i) {
    const uint64_t d = (uint64_t)dims[i];
    if (e > ~0ull / d) return ~0ull;
    e *= d;
  }
  return e;
}

int check_dims(const std::string& who, const int32_t* dims, int M) {
  if (!dims) {
    set_error(who + ": null pointer");
    return SUP_EINVAL;
  }
  if (M < 1 || M > kLhafTabMaxM) {
    set_error(who + ": M = " + std::to_string(M) + " outside [1, 64]");
    return SUP_EINVAL;
  }
  for (int i = 0; i < M; ++i)
    if (dims[i] < 1 || dims[i] > kLhafTabMaxDim) {
      set_error(who + ": dims[" + std::to_string(i) + "] = " + std::to_string(dims[i]) + " outside [1, 65]");
      return SUP_EINVAL;
    }
  return SUP_OK;
}

// Operations of the whole table: per entry above 0, 4 for zeta_p t[m], 2 for
// the scale, and 6 per term of the sum (2 products, 4 fmas).  Slab (p, c) has
// S_p (d_j - 1) / d_j entries with m_j > 0 for every j < p, and all S_p with
// m_p > 0 when c > 1.  In long double: the counts are below 2^40.
long double table_ops(const int32_t* dims, int M, uint64_t entries) {
  long double terms = 0.0L, S = 1.0L;
  for (int p = 0; p < M; ++p) {
    const long double d = (long double)dims[p];
    long double below = 0.0L;
    for (int j = 0; j < p; ++j) below += S * (long double)(dims[j] - 1) / (long double)dims[j];
    terms += (d - 1.0L) * below + (d > 2.0L ? (d - 2.0L) * S : 0.0L);
    S *= d;
  }
  return 6.0L * (long double)(entries - 1) + 6.0L * terms;
}

// SUP_LHAF_TABLE_LOW=E or the compiled tile; E outside [1, kLhafLowTile]: SUP_EINVAL.
int lhaf_table_low(uint32_t* low) {
  *low = kLhafLowTile;
  const char* e = std::getenv("SUP_LHAF_TABLE_LOW");  // tests, read per call: a smaller prefix (the bits do not change)
  if (!e || !*e) return SUP_OK;
  long v = 0;
  char tail = 0;
  if (std::sscanf(e, "%ld%c", &v, &tail) != 1 || v < 1 || v > (long)kLhafLowTile) {
    set_error("SUP_LHAF_TABLE_LOW=" + std::string(e) + ": expected E with 1 <= E <= " + std::to_string(kLhafLowTile) +
              ", the entries of the low kernel's compiled tile");
    return SUP_EINVAL;
  }
  *low = (uint32_t)v;
  return SUP_OK;
}

}  // namespace

int loop_hafnian_table_plan(const int32_t* dims, int M, uint64_t* entries, uint64_t* launches, double* ops_per_entry) {
  const std::string who = "sup_loop_hafnian_table_plan";
  if (int rc = check_dims(who, dims, M)) return rc;
  uint32_t low = 0;
  if (int rc = lhaf_table_low(&low)) return rc;
  const uint64_t e = entries_of(dims, M);
  if (entries) *entries = e;
  uint32_t count = 1;
  const int plow = lhaf_low_modes(dims, M, low, &count);
  uint64_t n = 1;
  for (int p = plow; p < M; ++p) n += (uint64_t)(dims[p] - 1);
  if (launches) *launches = n;
  if (ops_per_entry) *ops_per_entry = e == ~0ull ? 0.0 : (double)(table_ops(dims, M, e) / (long double)e);
  return SUP_OK;
}

int loop_hafnian_table(const double* A, int M, const double* mu, const int32_t* dims, const sup_opts& o, bool on_cpu,
                       double* out, LhafTabInfo* info) {
  const std::string who = "sup_loop_hafnian_table";
  if (!A || !dims || !out) {
    set_error(who + ": null pointer");
    return SUP_EINVAL;
  }
  if (int rc = check_dims(who, dims, M)) return rc;
  for (int i = 0; i < M; ++i)
    for (int j = 0; j < i; ++j)
      if (std::memcmp(A + 2 * ((size_t)i * M + j), A + 2 * ((size_t)j * M + i), 2 * sizeof(double)) != 0) {
        set_error(who + ": A[" + std::to_string(j) + "][" + std::to_string(i) + "] and A[" + std::to_string(i) + "][" +
                  std::to_string(j) + "] differ: A must be symmetric bit for bit");
        return SUP_EINVAL;
      }
  if (o.gpu_num > 1) {
    set_error(who + ": gpu_num = " + std::to_string(o.gpu_num) + ": a table is one device's (o->device_id)");
    return SUP_EINVAL;
  }
  uint32_t low = 0;
  if (int rc = lhaf_table_low(&low)) return rc;
  LhafTabInfo ti;
  ti.entries = entries_of(dims, M);
  if (ti.entries > SUP_LHAF_TABLE_MAX_ENTRIES) {
    set_error(who + ": prod dims " + (ti.entries == ~0ull ? std::string("at least 2^64") : "= " + std::to_string(ti.entries)) +
              " above SUP_LHAF_TABLE_MAX_ENTRIES = " + std::to_string((uint64_t)SUP_LHAF_TABLE_MAX_ENTRIES) +
              " (16 bytes per entry)");
    return SUP_EUNSUPPORTED;
  }
  ti.ops = (double)(table_ops(dims, M, ti.entries) / (long double)ti.entries);
  const double zero[2 * kLhafTabMaxM] = {};
  const double* zeta = mu ? mu : zero;
  if (on_cpu) {
    try {
      table_cpu(A, M, zeta, dims, o.threads, out);
    } catch (const std::bad_alloc&) {
      set_error("out of host memory for the loop-hafnian table's threads");
      return SUP_ENOMEM;
    }
    if (info) *info = ti;
    return SUP_OK;
  }
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
  if (int rc = run_lhaf_table(o.device_id, A, M, zeta, dims, ti.entries, low, out, &ti.kernel_ms, &ti.grid, &ti.launches))
    return rc;
  ti.devices = 1;
  if (info) *info = ti;
  return SUP_OK;
}

}  // namespace sup
