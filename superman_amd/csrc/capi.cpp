// capi.cpp — extern "C" boundary (include/superman.h).
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <mutex>

#include "dd.hpp"
#include "engine.hpp"
#include "hafnian_exact.hpp"
#include "hafnian_pt.hpp"
#include "hafnian_quad.hpp"
#include "loop_torontonian.hpp"
#include "torontonian.hpp"
#include "lhaf_table.hpp"
#include "torontonian_table.hpp"

using namespace sup;

namespace {

int check_common(const void* mat, int n, double* out) {
  if (!mat || !out) {
    set_error("null matrix or output pointer");
    return SUP_EINVAL;
  }
  if (n < 1 || n > SUP_MAX_N) {
    set_error("n = " + std::to_string(n) + " outside [1, 64] (64-bit Gray index)");
    return SUP_EINVAL;
  }
  return SUP_OK;
}

// The kernels index the walk with 32 bits (T = 1u << m) and pack the walk
// bits' block counts into two 64-bit words (k < 32), as default_layout
// assumes; an item of the chunk queue is 2^chunk_log2 wave-chunks (< 2^64).
int check_walk_opts(const sup_opts& o) {
  if (o.walk_log2 < 0 || o.walk_log2 > 31) {
    set_error("walk_log2 = " + std::to_string(o.walk_log2) + " outside [0, 31] (0 = default layout)");
    return SUP_EINVAL;
  }
  if (o.chunk_log2 < 0 || o.chunk_log2 > 62) {
    set_error("chunk_log2 = " + std::to_string(o.chunk_log2) + " outside [0, 62] (0 = automatic item size)");
    return SUP_EINVAL;
  }
  return SUP_OK;
}

WalkKind kind_of(sup_kernel k) {
  switch (k) {
    case SUP_KERNEL_SPARYSER: return kWalkSparse;
    case SUP_KERNEL_SKIPPER: return kWalkSkip;
    case SUP_KERNEL_SEGMENTED: return kWalkSeg;
    default: return kWalkDense;
  }
}

void fill_stats(sup_stats* st, const Plan& P, const SchedResult& r, double wall_ms, uint64_t gray) {
  if (!st) return;
  std::memset(st, 0, sizeof(*st));
  st->kernel_ms = r.kernel_ms;
  st->wall_ms = wall_ms;
  st->gray_steps = gray;
  st->visited_steps = r.visited;
  st->devices_used = r.devices;
  st->lane_bits = P.lay.L;
  st->walk_bits = P.lay.m;
  st->grid = r.grid;
  st->chunks_done_cpu = r.cpu_items;
  for (size_t i = 0; i < r.dev_partials.size() && i < 16; ++i) st->partials[i] = r.dev_partials[i];
  st->walk_kind = P.lds ? 4 : (int)P.kind;
  st->leaves = 1;
  st->est_ops_per_step = walk_cost(P);
  st->jit_ms = r.compile_ms;
  st->items_resumed = r.items_resumed;
  if (P.kind == kWalkSeg) {
    st->seg_cached_bits = (int16_t)P.seg_cc;
    st->seg_pair_bits = (int16_t)P.seg_b;
  }
}

}  // namespace

extern "C" {

void sup_opts_init(sup_opts* o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  o->gpu_num = 1;
  o->device_id = 0;
  o->threads = 16;  // main.cu:333
  o->block_dim = 256;
  o->timing = 1;
}

int sup_abi_version(void) { return SUP_ABI_VERSION; }
const char* sup_last_error(void) { return last_error(); }
int sup_device_count(int* count) {
  if (!count) return SUP_EINVAL;
  return device_count(count);
}
uint64_t sup_device_checks(void) { return device_checks_passed(); }
int sup_device_warmup(int device_id, int gpu_num, int n) {
  if (device_id < 0 || gpu_num < 1) return SUP_EINVAL;
  return warm_devices(device_id, gpu_num, n);
}
int sup_kernel_time(int device_id, double* total_ms, uint64_t* launches) {
  if (device_id < 0) return SUP_EINVAL;
  return kernel_time(device_id, total_ms, launches);
}
int sup_rccl_devices(int ndev, int* phys) {
  if (ndev < 1 || ndev > 1024 || !phys) return SUP_EINVAL;
  std::vector<int> devs(ndev), p;
  for (int g = 0; g < ndev; ++g) devs[g] = g;
  if (int rc = rccl_physical_devices(devs, p)) return rc;
  std::copy(p.begin(), p.end(), phys);
  return SUP_OK;
}

int sup_nw_start(const void* mat, sup_dtype t, int n, double* x0, double* p0) {
  if (!x0 || !p0) {
    set_error("null output pointer");
    return SUP_EINVAL;
  }
  std::vector<double> A;
  int rc = to_double(mat, t, n, A);
  if (rc) return rc;
  nw_start(A.data(), n, x0, p0);
  return SUP_OK;
}

// The default layout, or the walk length (m walk bits) sup_opts::walk_log2 asks for.
static Layout layout_for(int n, const sup_opts& o) { return layout_with_walk(n, o.walk_log2); }

int sup_perman(const void* mat, sup_dtype t, int n, sup_kernel kernel, sup_sched sched, const sup_opts* o_in,
               double* out, sup_stats* st) {
  auto t0 = std::chrono::steady_clock::now();
  int rc = check_common(mat, n, out);
  if (rc) return rc;
  sup_opts o;
  if (o_in) o = *o_in;
  else sup_opts_init(&o);
  std::vector<double> A;
  if ((rc = to_double(mat, t, n, A))) return rc;
  if ((rc = check_walk_opts(o))) return rc;
  const Layout lay = layout_for(n, o);
  std::shared_ptr<const Plan> sp;
  if ((rc = plan_for_shared(A.data(), n, kernel, lay, sp, o.jit, sched == SUP_SCHED_SINGLE ? 1 : o.gpu_num,
                            o.device_id)))
    return rc;
  const Plan& P = *sp;
  SchedResult r;
  if ((rc = schedule(P, sched, o, 0, P.lay.chunks(), r))) return rc;
  *out = (double)(4 * (n & 1) - 2) * r.total;  // gpu_exact_dense.cu:698
  const double wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  fill_stats(st, P, r, wall, 1ull << (n - 1));
  return SUP_OK;
}

int sup_partial(const void* mat, sup_dtype t, int n, sup_kernel kernel, uint64_t start, uint64_t end,
                const sup_opts* o_in, double* out, sup_stats* st) {
  auto t0 = std::chrono::steady_clock::now();
  int rc = check_common(mat, n, out);
  if (rc) return rc;
  const uint64_t space = 1ull << (n - 1);
  if (start > end || end > space) {
    set_error("range [start, end) must satisfy start <= end <= 2^(n-1)");
    return SUP_EINVAL;
  }
  sup_opts o;
  if (o_in) o = *o_in;
  else sup_opts_init(&o);
  if ((rc = check_walk_opts(o))) return rc;
  // Largest layout whose wave-chunk (2^(L+m) Gray indices) divides both ends.
  Layout lay = default_layout(n);
  const int nb = n - 1;
  auto align_of = [&](uint64_t v) -> int { return v == 0 || v == space ? nb : __builtin_ctzll(v); };
  const int al = std::min(align_of(start), align_of(end));
  if (al < lay.L) {
    set_error("range ends must be multiples of 2^" + std::to_string(lay.L) + " (one wave of Gray indices)");
    return SUP_EINVAL;
  }
  if (lay.L + lay.m > al) {
    lay.m = al - lay.L;
    lay.h = nb - lay.L - lay.m;
  }
  if (o.walk_log2 > 0 && o.walk_log2 < lay.m) {
    lay.m = o.walk_log2;
    lay.h = nb - lay.L - lay.m;
  }
  std::vector<double> A;
  if ((rc = to_double(mat, t, n, A))) return rc;
  Plan P;
  if ((rc = make_plan(A.data(), n, kind_of(kernel), true, lay, P))) return rc;
  P.lds = kernel == SUP_KERNEL_DENSE_LDS;
  const int cb = lay.L + lay.m;
  SchedResult r;
  if ((rc = schedule(P, o.gpu_num > 1 ? SUP_SCHED_STATIC : SUP_SCHED_SINGLE, o, start >> cb, end >> cb, r)))
    return rc;
  *out = r.total;
  const double wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  fill_stats(st, P, r, wall, end - start);
  return SUP_OK;
}

int sup_perman_cpu(const void* mat, sup_dtype t, int n, sup_kernel kernel, int threads, double* out,
                   sup_stats* st) {
  auto t0 = std::chrono::steady_clock::now();
  int rc = check_common(mat, n, out);
  if (rc) return rc;
  std::vector<double> A;
  if ((rc = to_double(mat, t, n, A))) return rc;
  Plan P;
  if ((rc = plan_for(A.data(), n, kernel, default_layout(n), P))) return rc;
  SchedResult r;
  r.total = cpu_walk_range(P, 0, P.lay.chunks(), threads < 1 ? 1 : threads);
  r.visited = 1ull << (n - 1);
  *out = (double)(4 * (n & 1) - 2) * r.total;
  const double wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  fill_stats(st, P, r, wall, 1ull << (n - 1));
  return SUP_OK;
}

int sup_perman_shard(const void* mat, sup_dtype t, int n, sup_kernel kernel, int shard, int nshards,
                     const sup_opts* o_in, double* out, sup_stats* st) {
  auto t0 = std::chrono::steady_clock::now();
  int rc = check_common(mat, n, out);
  if (rc) return rc;
  if (nshards < 1 || shard < 0 || shard >= nshards) {
    set_error("shard index out of range");
    return SUP_EINVAL;
  }
  sup_opts o;
  if (o_in) o = *o_in;
  else sup_opts_init(&o);
  if ((rc = check_walk_opts(o))) return rc;
  std::vector<double> A;
  if ((rc = to_double(mat, t, n, A))) return rc;
  std::shared_ptr<const Plan> sp;
  if ((rc = plan_for_shared(A.data(), n, kernel, layout_for(n, o), sp, o.jit, nshards, o.device_id))) return rc;
  const Plan& P = *sp;
  const uint64_t C = P.lay.chunks();
  const uint64_t c0 = C * (uint64_t)shard / (uint64_t)nshards, c1 = C * (uint64_t)(shard + 1) / (uint64_t)nshards;
  SchedResult r;
  struct DeferTiming {  // sup_opts.timing = 0: this call's walk time is read by sup_kernel_time
    explicit DeferTiming(bool on) { set_defer_timing(on); }
    ~DeferTiming() { set_defer_timing(false); }
  } defer(o.timing == 0);
  if ((rc = schedule(P, SUP_SCHED_SINGLE, o, c0, c1, r))) return rc;
  *out = r.total;
  const double wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  fill_stats(st, P, r, wall, (c1 - c0) << (P.lay.L + P.lay.m));
  return SUP_OK;
}

int sup_perman_exact(const void* mat, sup_dtype t, int n, const sup_opts* o_in, int on_cpu, char* out,
                     size_t out_len, sup_stats* st) {
  auto t0 = std::chrono::steady_clock::now();
  if (!out || out_len < 2) {
    set_error("sup_perman_exact: output buffer missing or too small");
    return SUP_EINVAL;
  }
  std::vector<double> A;
  int rc = to_double(mat, t, n, A);
  if (rc) return rc;
  sup_opts o;
  if (o_in) o = *o_in;
  else sup_opts_init(&o);
  std::string s;
  double kms = 0.0;
  int used = 0, cpu_items = 0;
  RangeInfo ri;  // stays zero (dense, no walk bits) when a zero row ends the call early
  if ((rc = exact_perman(A.data(), n, o, on_cpu != 0, s, &kms, &used, &cpu_items, &ri))) return rc;
  if (s.size() + 1 > out_len) {
    set_error("sup_perman_exact: output buffer too small");
    return SUP_EINVAL;
  }
  std::memcpy(out, s.c_str(), s.size() + 1);
  if (st) {
    std::memset(st, 0, sizeof(*st));
    st->kernel_ms = kms;
    st->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    st->gray_steps = 1ull << (n - 1);
    st->visited_steps = st->gray_steps;
    st->devices_used = used;
    st->chunks_done_cpu = cpu_items;
    st->lane_bits = ri.lay.L;
    st->walk_bits = ri.lay.m;
    st->walk_kind = ri.walk_kind;
    st->seg_pair_bits = (int16_t)ri.group;
    st->leaves = 1;
  }
  return SUP_OK;
}

int sup_perman_exact_range(const void* mat, sup_dtype t, int n, uint64_t c0, uint64_t c1, const sup_opts* o_in,
                           int on_cpu, int form, int group, uint64_t* primes, uint64_t* residues, int cap,
                           int* nprimes, int* colmap, sup_stats* st) {
  auto t0 = std::chrono::steady_clock::now();
  if (!mat || !primes || !residues || !nprimes) {
    set_error("sup_perman_exact_range: null matrix or output pointer");
    return SUP_EINVAL;
  }
  sup_opts o;
  if (o_in) o = *o_in;
  else sup_opts_init(&o);
  int rc = check_range_request(n, o, form, "sup_perman_exact_range");
  if (rc) return rc;
  std::vector<double> A;
  if ((rc = to_double(mat, t, n, A))) return rc;
  std::vector<uint64_t> pr, res;
  RangeInfo ri;
  if ((rc = exact_perman_range(A.data(), n, c0, c1, o, on_cpu != 0, form, group, cap, pr, res, &ri))) return rc;
  std::copy(pr.begin(), pr.end(), primes);
  std::copy(res.begin(), res.end(), residues);
  *nprimes = (int)pr.size();
  if (colmap) std::copy(ri.colmap.begin(), ri.colmap.end(), colmap);
  if (st) {
    std::memset(st, 0, sizeof(*st));
    st->kernel_ms = ri.kernel_ms;
    st->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    st->gray_steps = (c1 - c0) << (ri.lay.L + ri.lay.m);
    st->visited_steps = st->gray_steps;
    st->devices_used = ri.devices;
    st->lane_bits = ri.lay.L;
    st->walk_bits = ri.lay.m;
    st->walk_kind = ri.walk_kind;
    st->seg_pair_bits = (int16_t)ri.group;
    st->leaves = 1;
    st->est_ops_per_step = ri.est_ops;
  }
  return SUP_OK;
}

int sup_perman_quad(const void* mat, sup_dtype t, int n, const sup_opts* o_in, int on_cpu, double* out_hi,
                    double* out_lo, sup_stats* st) {
  auto t0 = std::chrono::steady_clock::now();
  if (!out_hi) {
    set_error("sup_perman_quad: out_hi missing");
    return SUP_EINVAL;
  }
  std::vector<double> A;
  int rc = to_double(mat, t, n, A);
  if (rc) return rc;
  sup_opts o;
  if (o_in) o = *o_in;
  else sup_opts_init(&o);
  double hi = 0.0, lo = 0.0, kms = 0.0;
  int used = 0;
  RangeInfo ri;
  if ((rc = quad_perman(A.data(), n, o, on_cpu != 0, &hi, &lo, &kms, &used, &ri))) return rc;
  *out_hi = hi;
  if (out_lo) *out_lo = lo;
  if (st) {
    std::memset(st, 0, sizeof(*st));
    st->kernel_ms = kms;
    st->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    st->gray_steps = 1ull << (n - 1);
    st->visited_steps = st->gray_steps;
    st->devices_used = used;
    st->lane_bits = ri.lay.L;
    st->walk_bits = ri.lay.m;
    st->walk_kind = ri.walk_kind;
    st->leaves = 1;
    st->est_ops_per_step = ri.est_ops;
  }
  return SUP_OK;
}

int sup_perman_quad_range(const void* mat, sup_dtype t, int n, uint64_t c0, uint64_t c1, const sup_opts* o_in,
                          int on_cpu, int form, double* out_hi, double* out_lo, int* colmap, sup_stats* st) {
  auto t0 = std::chrono::steady_clock::now();
  if (!mat || !out_hi || !out_lo) {
    set_error("sup_perman_quad_range: null matrix or output pointer");
    return SUP_EINVAL;
  }
  sup_opts o;
  if (o_in) o = *o_in;
  else sup_opts_init(&o);
  int rc = check_range_request(n, o, form, "sup_perman_quad_range");
  if (rc) return rc;
  std::vector<double> A;
  if ((rc = to_double(mat, t, n, A))) return rc;
  double hi = 0.0, lo = 0.0;
  RangeInfo ri;
  if ((rc = quad_perman_range(A.data(), n, c0, c1, o, on_cpu != 0, form, &hi, &lo, &ri))) return rc;
  *out_hi = hi;
  *out_lo = lo;
  if (colmap) std::copy(ri.colmap.begin(), ri.colmap.end(), colmap);
  if (st) {
    std::memset(st, 0, sizeof(*st));
    st->kernel_ms = ri.kernel_ms;
    st->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    st->gray_steps = (c1 - c0) << (ri.lay.L + ri.lay.m);
    st->visited_steps = st->gray_steps;
    st->devices_used = ri.devices;
    st->lane_bits = ri.lay.L;
    st->walk_bits = ri.lay.m;
    st->walk_kind = ri.walk_kind;
    st->leaves = 1;
    st->est_ops_per_step = ri.est_ops;
  }
  return SUP_OK;
}

// sup_stats of a complex call over `steps` Gray steps (est_ops_per_step: 6n, the header's figure).
static void fill_cplx_stats(sup_stats* st, const CplxInfo& ci, int n, uint64_t steps, double wall_ms) {
  if (!st) return;
  std::memset(st, 0, sizeof(*st));
  st->kernel_ms = ci.kernel_ms;
  st->wall_ms = wall_ms;
  st->gray_steps = steps;
  st->visited_steps = steps;
  st->devices_used = ci.devices;
  st->lane_bits = ci.lay.L;
  st->walk_bits = ci.lay.m;
  st->grid = ci.grid;
  st->walk_kind = (int)kWalkDense;
  st->leaves = 1;
  st->est_ops_per_step = 6.0 * n;
}

int sup_perman_complex(const double* mat, int n, const sup_opts* o_in, int on_cpu, double* out_re, double* out_im,
                       sup_stats* st) {
  auto t0 = std::chrono::steady_clock::now();
  if (!mat || !out_re || !out_im) {
    set_error("sup_perman_complex: null matrix or output pointer");
    return SUP_EINVAL;
  }
  sup_opts o;
  if (o_in) o = *o_in;
  else sup_opts_init(&o);
  double re = 0.0, im = 0.0;
  CplxInfo ci;
  if (int rc = cplx_perman(mat, n, o, on_cpu != 0, &re, &im, &ci)) return rc;
  *out_re = re;
  *out_im = im;
  const double wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  fill_cplx_stats(st, ci, n, 1ull << (n - 1), wall);
  return SUP_OK;
}

int sup_perman_complex_range(const double* mat, int n, uint64_t c0, uint64_t c1, const sup_opts* o_in, int on_cpu,
                             double* out_re, double* out_im, sup_stats* st) {
  auto t0 = std::chrono::steady_clock::now();
  if (!mat || !out_re || !out_im) {
    set_error("sup_perman_complex_range: null matrix or output pointer");
    return SUP_EINVAL;
  }
  sup_opts o;
  if (o_in) o = *o_in;
  else sup_opts_init(&o);
  double re = 0.0, im = 0.0;
  CplxInfo ci;
  if (int rc = cplx_perman_range(mat, n, c0, c1, o, on_cpu != 0, &re, &im, &ci)) return rc;
  *out_re = re;
  *out_im = im;
  const double wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  fill_cplx_stats(st, ci, n, (c1 - c0) << (ci.lay.L + ci.lay.m), wall);
  return SUP_OK;
}

// The complex double-double entries (cplx_quad.cpp checks every argument).
int sup_perman_complex_quad(const double* mat, int n, const sup_opts* o_in, int on_cpu, double* out, sup_stats* st) {
  auto t0 = std::chrono::steady_clock::now();
  sup_opts o;
  if (o_in) o = *o_in;
  else sup_opts_init(&o);
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  CplxInfo ci;
  if (int rc = cplx_quad_perman(mat, n, o, on_cpu != 0, out ? v : nullptr, &ci)) return rc;
  std::copy(v, v + 4, out);
  const double wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  fill_cplx_stats(st, ci, n, 1ull << (n - 1), wall);
  if (st) st->est_ops_per_step = 86.0 * n - 28.0;
  return SUP_OK;
}

int sup_perman_complex_quad_range(const double* mat, int n, uint64_t c0, uint64_t c1, const sup_opts* o_in, int on_cpu,
                                  double* out, sup_stats* st) {
  auto t0 = std::chrono::steady_clock::now();
  sup_opts o;
  if (o_in) o = *o_in;
  else sup_opts_init(&o);
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  CplxInfo ci;
  if (int rc = cplx_quad_perman_range(mat, n, c0, c1, o, on_cpu != 0, out ? v : nullptr, &ci)) return rc;
  std::copy(v, v + 4, out);
  const double wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  fill_cplx_stats(st, ci, n, (c1 - c0) << (ci.lay.L + ci.lay.m), wall);
  if (st) st->est_ops_per_step = 86.0 * n - 28.0;
  return SUP_OK;
}

// The exact complex entries (cplx_exact.cpp checks the matrix and the options).
static void fill_cplx_exact_stats(sup_stats* st, const CplxExactInfo& xi, int n, uint64_t steps, double wall_ms) {
  fill_cplx_stats(st, xi.ci, n, steps, wall_ms);
  if (!st) return;
  st->seg_pair_bits = (int16_t)xi.group;
  st->est_ops_per_step = xi.est_ops;
}

int sup_perman_complex_exact(const double* mat, int n, const sup_opts* o_in, int on_cpu, char* out_re, char* out_im,
                             size_t out_len, sup_stats* st) {
  auto t0 = std::chrono::steady_clock::now();
  if (!mat || !out_re || !out_im) {
    set_error("sup_perman_complex_exact: null matrix or output pointer");
    return SUP_EINVAL;
  }
  sup_opts o;
  if (o_in) o = *o_in;
  else sup_opts_init(&o);
  std::string re, im;
  CplxExactInfo xi;
  if (int rc = cplx_exact_perman(mat, n, o, on_cpu != 0, re, im, &xi)) return rc;
  const size_t need = std::max(re.size(), im.size()) + 1;
  if (out_len < need) {
    set_error("sup_perman_complex_exact: out_len = " + std::to_string(out_len) + " but the result needs " +
              std::to_string(need) + " bytes per buffer (640 always suffice)");
    return SUP_EINVAL;
  }
  std::memcpy(out_re, re.c_str(), re.size() + 1);
  std::memcpy(out_im, im.c_str(), im.size() + 1);
  const double wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  fill_cplx_exact_stats(st, xi, n, xi.group ? 1ull << (n - 1) : 0, wall);  // group 0: a zero row, no walk
  return SUP_OK;
}

int sup_perman_complex_exact_range(const double* mat, int n, uint64_t c0, uint64_t c1, const sup_opts* o_in,
                                   int on_cpu, int group, uint64_t* primes, uint64_t* res_re, uint64_t* res_im,
                                   int cap, int* nprimes, sup_stats* st) {
  auto t0 = std::chrono::steady_clock::now();
  if (!mat || !primes || !res_re || !res_im || !nprimes) {
    set_error("sup_perman_complex_exact_range: null matrix or output pointer");
    return SUP_EINVAL;
  }
  sup_opts o;
  if (o_in) o = *o_in;
  else sup_opts_init(&o);
  std::vector<uint64_t> pr, rr, ri;
  CplxExactInfo xi;
  if (int rc = cplx_exact_perman_range(mat, n, c0, c1, o, on_cpu != 0, group, cap, pr, rr, ri, &xi)) return rc;
  std::copy(pr.begin(), pr.end(), primes);
  std::copy(rr.begin(), rr.end(), res_re);
  std::copy(ri.begin(), ri.end(), res_im);
  *nprimes = (int)pr.size();
  const double wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  fill_cplx_exact_stats(st, xi, n, (c1 - c0) << (xi.ci.lay.L + xi.ci.lay.m), wall);
  return SUP_OK;
}

// Both batched complex entries: `in` names the matrices (raw or U + index lists).
static int complex_batch(const CplxBatchIn& in, int n, uint64_t count, const sup_opts* o_in, int on_cpu, double* out,
                         sup_stats* st) {
  auto t0 = std::chrono::steady_clock::now();
  sup_opts o;
  if (o_in) o = *o_in;
  else sup_opts_init(&o);
  CplxInfo ci;
  if (int rc = cplx_perman_batch(in, n, count, o, on_cpu != 0, out, &ci)) return rc;
  const double wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  fill_cplx_stats(st, ci, n, count << (n - 1), wall);
  if (st) st->leaves = (int)std::min<uint64_t>(count, 0x7fffffffu);
  return SUP_OK;
}

int sup_perman_complex_batch(const double* mats, int n, uint64_t count, const sup_opts* o, int on_cpu, double* out,
                             sup_stats* st) {
  if (!mats || !out) {
    set_error("sup_perman_complex_batch: null matrix or output pointer");
    return SUP_EINVAL;
  }
  CplxBatchIn in;
  in.mats = mats;
  return complex_batch(in, n, count, o, on_cpu, out, st);
}

int sup_perman_complex_submatrices(const double* U, int R, int C, const int32_t* rows, const int32_t* cols, int n,
                                   uint64_t count, const sup_opts* o, int on_cpu, double* out, sup_stats* st) {
  if (!U || !rows || !cols || !out) {
    set_error("sup_perman_complex_submatrices: null matrix, index list or output pointer");
    return SUP_EINVAL;
  }
  CplxBatchIn in;
  in.U = U, in.R = R, in.C = C, in.rows = rows, in.cols = cols;
  return complex_batch(in, n, count, o, on_cpu, out, st);
}

int sup_perman_complex_fock(const double* U, int R, int C, const int32_t* rows, const int32_t* cols, int n,
                            uint64_t count, const sup_opts* o_in, int on_cpu, double* out, sup_stats* st) {
  auto t0 = std::chrono::steady_clock::now();
  if (!U || !rows || !cols || !out) {
    set_error("sup_perman_complex_fock: null matrix, index list or output pointer");
    return SUP_EINVAL;
  }
  sup_opts o;
  if (o_in) o = *o_in;
  else sup_opts_init(&o);
  CplxBatchIn in;
  in.U = U, in.R = R, in.C = C, in.rows = rows, in.cols = cols;
  FockInfo fi;
  if (int rc = cplx_perman_fock(in, n, count, o, on_cpu != 0, out, &fi)) return rc;
  if (st) {
    std::memset(st, 0, sizeof(*st));
    st->kernel_ms = fi.kernel_ms;
    st->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    st->gray_steps = count << (n - 1);  // nominal: the expanded matrices' walk
    st->visited_steps = fi.terms;
    st->devices_used = fi.devices;
    st->grid = fi.grid;
    st->walk_kind = (int)kWalkDense;
    st->leaves = (int)std::min<uint64_t>(count, 0x7fffffffu);
    st->est_ops_per_step = 6.0 * n;
  }
  return SUP_OK;
}

int sup_perman_complex_fock_plan(const int32_t* rows, const int32_t* cols, int n, uint64_t count, uint64_t* terms,
                                 int* side) {
  return cplx_fock_plan(rows, cols, n, count, terms, side);
}

static int hafnian_entry(const HafIn& in, int n, uint64_t count, const sup_opts* o_in, int on_cpu, double* out,
                         sup_stats* st) {
  auto t0 = std::chrono::steady_clock::now();
  sup_opts o;
  if (o_in) o = *o_in;
  else sup_opts_init(&o);
  HafInfo hi;
  if (int rc = hafnian_complex(in, n, count, o, on_cpu != 0, out, &hi)) return rc;
  if (st) {
    std::memset(st, 0, sizeof(*st));
    st->kernel_ms = hi.kernel_ms;
    st->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    st->gray_steps = count << (n - 1);  // nominal: the sum without repeats
    st->visited_steps = hi.terms;
    st->devices_used = hi.devices;
    st->grid = hi.grid;
    st->walk_kind = (int)kWalkDense;
    st->leaves = (int)std::min<uint64_t>(count, 0x7fffffffu);
    st->est_ops_per_step = hi.ops;
  }
  return SUP_OK;
}

int sup_hafnian_complex(const double* A, int M, const int32_t* idx, int n, uint64_t count, const sup_opts* o,
                        int on_cpu, double* out, sup_stats* st) {
  HafIn in;
  in.A = A, in.M = M, in.idx = idx;
  return hafnian_entry(in, n, count, o, on_cpu, out, st);
}

int sup_loop_hafnian_complex(const double* A, int M, const double* mu, const int32_t* idx, int n, uint64_t count,
                             const sup_opts* o, int on_cpu, double* out, sup_stats* st) {
  HafIn in;
  in.A = A, in.M = M, in.mu = mu, in.idx = idx, in.loop = true;
  return hafnian_entry(in, n, count, o, on_cpu, out, st);
}

static int hafnian_quad_entry(const HafIn& in, int n, uint64_t count, const sup_opts* o_in, int on_cpu, double* out,
                              sup_stats* st) {
  auto t0 = std::chrono::steady_clock::now();
  sup_opts o;
  if (o_in) o = *o_in;
  else sup_opts_init(&o);
  HafInfo hi;
  if (int rc = hafnian_quad(in, n, count, o, on_cpu != 0, out, &hi)) return rc;
  if (st) {
    std::memset(st, 0, sizeof(*st));
    st->kernel_ms = hi.kernel_ms;
    st->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    st->gray_steps = count << (n - 1);  // nominal: the sum without repeats
    st->visited_steps = hi.terms;
    st->devices_used = hi.devices;
    st->grid = hi.grid;
    st->walk_kind = (int)kWalkDense;
    st->leaves = (int)std::min<uint64_t>(count, 0x7fffffffu);
    st->est_ops_per_step = hi.ops;
  }
  return SUP_OK;
}

int sup_hafnian_complex_quad(const double* A, int M, const int32_t* idx, int n, uint64_t count, const sup_opts* o,
                             int on_cpu, double* out, sup_stats* st) {
  HafIn in;
  in.A = A, in.M = M, in.idx = idx;
  return hafnian_quad_entry(in, n, count, o, on_cpu, out, st);
}

int sup_loop_hafnian_complex_quad(const double* A, int M, const double* mu, const int32_t* idx, int n, uint64_t count,
                                  const sup_opts* o, int on_cpu, double* out, sup_stats* st) {
  HafIn in;
  in.A = A, in.M = M, in.mu = mu, in.idx = idx, in.loop = true;
  return hafnian_quad_entry(in, n, count, o, on_cpu, out, st);
}

int sup_hafnian_complex_plan(const int32_t* idx, int n, uint64_t count, uint64_t* terms) {
  return hafnian_plan(idx, n, count, terms);
}

int sup_loop_hafnian_complex_each(const double* A, int M, const double* mu, uint64_t nmu, const int32_t* mu_of,
                                  const int32_t* idx, int stride, const int32_t* n, uint64_t count,
                                  const sup_opts* o_in, int on_cpu, double* out, sup_stats* st) {
  auto t0 = std::chrono::steady_clock::now();
  sup_opts o;
  if (o_in) o = *o_in;
  else sup_opts_init(&o);
  HafEachIn in;
  in.A = A, in.M = M, in.mu = mu, in.nmu = nmu, in.mu_of = mu_of, in.idx = idx, in.stride = stride, in.n = n;
  HafInfo hi;
  if (int rc = loop_hafnian_each(in, count, o, on_cpu != 0, out, &hi)) return rc;
  if (st) {
    std::memset(st, 0, sizeof(*st));
    st->kernel_ms = hi.kernel_ms;
    st->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    uint64_t nominal = 0;  // the sums without repeats, saturating
    for (uint64_t k = 0; k < count; ++k)
      if (n[k] > 0) {
        const uint64_t add = 1ull << (n[k] - 1);
        nominal = nominal + add < nominal ? ~0ull : nominal + add;
      }
    st->gray_steps = nominal;
    st->visited_steps = hi.terms;
    st->devices_used = hi.devices;
    st->grid = hi.grid;
    st->walk_kind = (int)kWalkDense;
    st->leaves = (int)std::min<uint64_t>(count, 0x7fffffffu);
    st->est_ops_per_step = hi.ops;
  }
  return SUP_OK;
}

int sup_gbs_sample(const double* B, int M, const double* zeta, const double* het, int cutoff, uint64_t nsamples,
                   uint64_t sample0, uint64_t seed, const sup_opts* o_in, int on_cpu, int32_t* out, sup_stats* st) {
  auto t0 = std::chrono::steady_clock::now();
  sup_opts o;
  if (o_in) o = *o_in;
  else sup_opts_init(&o);
  GbsInfo gi;
  if (int rc = gbs_sample(B, M, zeta, het, cutoff, nsamples, sample0, seed, o, on_cpu != 0, out, &gi)) return rc;
  if (st) {
    std::memset(st, 0, sizeof(*st));
    st->kernel_ms = gi.kernel_ms;
    st->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    st->gray_steps = gi.visited;
    st->visited_steps = gi.visited;
    st->devices_used = gi.devices;
    st->walk_kind = (int)kWalkDense;
    st->leaves = (int)std::min<uint64_t>(nsamples, 0x7fffffffu);
    st->est_ops_per_step = gi.ops;
    st->partials[0] = gi.each_ms;         // wall time inside the ragged loop-hafnian calls
    st->partials[1] = gi.host_ms;         // wall time of the host stage: lists, z rows, weights and draws
    st->partials[2] = (double)gi.failed;  // samples whose weights summed to zero or to a non-finite value
  }
  return SUP_OK;
}

int sup_loop_hafnian_table(const double* A, int M, const double* mu, const int32_t* dims, const sup_opts* o_in,
                           int on_cpu, double* out, sup_stats* st) {
  auto t0 = std::chrono::steady_clock::now();
  sup_opts o;
  if (o_in) o = *o_in;
  else sup_opts_init(&o);
  LhafTabInfo ti;
  if (int rc = loop_hafnian_table(A, M, mu, dims, o, on_cpu != 0, out, &ti)) return rc;
  if (st) {
    std::memset(st, 0, sizeof(*st));
    st->kernel_ms = ti.kernel_ms;
    st->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    st->gray_steps = ti.entries;
    st->visited_steps = ti.entries;
    st->devices_used = ti.devices;
    st->grid = ti.grid;
    st->walk_kind = (int)kWalkDense;
    st->leaves = 1;
    st->est_ops_per_step = ti.ops;
    st->partials[0] = (double)ti.launches;  // kernel launches of the device path
  }
  return SUP_OK;
}

int sup_loop_hafnian_table_plan(const int32_t* dims, int M, uint64_t* entries, uint64_t* launches,
                                double* ops_per_entry) {
  return loop_hafnian_table_plan(dims, M, entries, launches, ops_per_entry);
}

int sup_hafnian_complex_exact(const double* A, int M, const double* mu, const int32_t* idx, int n, uint64_t count,
                              const sup_opts* o_in, int on_cpu, char* out_re, char* out_im, size_t out_len,
                              sup_stats* st) {
  auto t0 = std::chrono::steady_clock::now();
  if (!A || !idx || ((!out_re || !out_im) && count > 0)) {
    set_error("sup_hafnian_complex_exact: null pointer");
    return SUP_EINVAL;
  }
  sup_opts o;
  if (o_in) o = *o_in;
  else sup_opts_init(&o);
  HafIn in;
  in.A = A, in.M = M, in.mu = mu, in.idx = idx, in.loop = mu != nullptr;
  std::vector<std::string> re, im;
  HafxInfo hi;
  if (int rc = hafnian_exact(in, n, count, o, on_cpu != 0, re, im, &hi)) return rc;
  size_t need = 0;
  for (uint64_t k = 0; k < count; ++k) need = std::max(need, std::max(re[k].size(), im[k].size()) + 1);
  if (out_len < need) {
    set_error("sup_hafnian_complex_exact: out_len = " + std::to_string(out_len) + " but a result needs " +
              std::to_string(need) + " bytes per matrix and buffer (768 always suffice)");
    return SUP_EINVAL;
  }
  for (uint64_t k = 0; k < count; ++k) {
    std::memcpy(out_re + k * out_len, re[k].c_str(), re[k].size() + 1);
    std::memcpy(out_im + k * out_len, im[k].c_str(), im[k].size() + 1);
  }
  if (st) {
    std::memset(st, 0, sizeof(*st));
    st->kernel_ms = hi.kernel_ms;
    st->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    st->gray_steps = count << (n - 1);  // nominal: the sum without repeats
    st->visited_steps = hi.terms;
    st->devices_used = hi.devices;
    st->grid = hi.grid;
    st->walk_kind = (int)kWalkDense;
    st->leaves = (int)std::min<uint64_t>(count, 0x7fffffffu);
    st->est_ops_per_step = hi.ops;
    st->seg_cached_bits = (int16_t)hi.primes;
    st->seg_pair_bits = (int16_t)hi.launches;
  }
  return SUP_OK;
}

static int hafnian_pt_entry(const HafIn& in, int n, uint64_t count, bool range, uint64_t z0, uint64_t z1,
                            const sup_opts* o_in, int on_cpu, double* out, sup_stats* st) {
  auto t0 = std::chrono::steady_clock::now();
  sup_opts o;
  if (o_in) o = *o_in;
  else sup_opts_init(&o);
  if (range) o.gpu_num = 1;
  PtInfo pi;
  if (int rc = hafnian_pt(in, n, count, range, z0, z1, o, on_cpu != 0, out, &pi)) return rc;
  if (st) {
    std::memset(st, 0, sizeof(*st));
    st->kernel_ms = pi.kernel_ms;
    st->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    st->gray_steps = count << (n - 1);  // nominal: the Kan walk without repeats
    st->visited_steps = pi.subsets;
    st->devices_used = pi.devices;
    st->grid = pi.grid;
    st->walk_kind = (int)kWalkDense;
    st->leaves = (int)std::min<uint64_t>(count, 0x7fffffffu);
    st->est_ops_per_step = pi.ops;
  }
  return SUP_OK;
}

int sup_hafnian_complex_pt(const double* A, int M, const int32_t* idx, int n, uint64_t count, const sup_opts* o,
                           int on_cpu, double* out, sup_stats* st) {
  HafIn in;
  in.A = A, in.M = M, in.idx = idx;
  return hafnian_pt_entry(in, n, count, false, 0, 0, o, on_cpu, out, st);
}

int sup_loop_hafnian_complex_pt(const double* A, int M, const double* mu, const int32_t* idx, int n, uint64_t count,
                                const sup_opts* o, int on_cpu, double* out, sup_stats* st) {
  HafIn in;
  in.A = A, in.M = M, in.mu = mu, in.idx = idx, in.loop = true;
  return hafnian_pt_entry(in, n, count, false, 0, 0, o, on_cpu, out, st);
}

int sup_hafnian_complex_pt_range(const double* A, int M, const double* mu_or_null, const int32_t* idx, int n,
                                 uint64_t z_begin, uint64_t z_end, const sup_opts* o, int on_cpu, double* out,
                                 sup_stats* st) {
  HafIn in;
  in.A = A, in.M = M, in.mu = mu_or_null, in.idx = idx, in.loop = mu_or_null != nullptr;
  return hafnian_pt_entry(in, n, 1, true, z_begin, z_end, o, on_cpu, out, st);
}

int sup_hafnian_complex_pt_plan(int n, int loop, uint64_t* subsets, double* est_ops) {
  return hafnian_pt_plan(n, loop, subsets, est_ops);
}

static int torontonian_entry(const TorIn& in, int n, uint64_t count, bool range, uint64_t z0, uint64_t z1,
                             const sup_opts* o_in, int on_cpu, double* out, sup_stats* st) {
  auto t0 = std::chrono::steady_clock::now();
  sup_opts o;
  if (o_in) o = *o_in;
  else sup_opts_init(&o);
  if (range) o.gpu_num = 1;
  TorInfo ti;
  if (int rc = torontonian(in, n, count, range, z0, z1, o, on_cpu != 0, out, &ti)) return rc;
  if (st) {
    std::memset(st, 0, sizeof(*st));
    st->kernel_ms = ti.kernel_ms;
    st->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    st->gray_steps = count << n;
    st->visited_steps = ti.subsets;
    st->devices_used = ti.devices;
    st->grid = ti.grid;
    st->walk_kind = (int)kWalkDense;
    st->leaves = (int)std::min<uint64_t>(count, 0x7fffffffu);
    st->est_ops_per_step = ti.ops;
  }
  return SUP_OK;
}

int sup_torontonian(const double* O, int M, const int32_t* modes, int n, uint64_t count, const sup_opts* o, int on_cpu,
                    double* out, sup_stats* st) {
  TorIn in;
  in.O = O, in.M = M, in.modes = modes;
  return torontonian_entry(in, n, count, false, 0, 0, o, on_cpu, out, st);
}

int sup_torontonian_range(const double* O, int M, const int32_t* modes, int n, uint64_t z_begin, uint64_t z_end,
                          const sup_opts* o, int on_cpu, double* out, sup_stats* st) {
  TorIn in;
  in.O = O, in.M = M, in.modes = modes;
  return torontonian_entry(in, n, 1, true, z_begin, z_end, o, on_cpu, out, st);
}

int sup_torontonian_plan(int n, uint64_t* subsets, double* est_ops) { return torontonian_plan(n, subsets, est_ops); }

static int loop_torontonian_entry(const LtorIn& in, int n, uint64_t count, bool range, uint64_t z0, uint64_t z1,
                                  const sup_opts* o_in, int on_cpu, double* out, sup_stats* st) {
  auto t0 = std::chrono::steady_clock::now();
  sup_opts o;
  if (o_in) o = *o_in;
  else sup_opts_init(&o);
  if (range) o.gpu_num = 1;
  TorInfo ti;
  if (int rc = loop_torontonian(in, n, count, range, z0, z1, o, on_cpu != 0, out, &ti)) return rc;
  if (st) {
    std::memset(st, 0, sizeof(*st));
    st->kernel_ms = ti.kernel_ms;
    st->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    st->gray_steps = count << n;
    st->visited_steps = ti.subsets;
    st->devices_used = ti.devices;
    st->grid = ti.grid;
    st->walk_kind = (int)kWalkDense;
    st->leaves = (int)std::min<uint64_t>(count, 0x7fffffffu);
    st->est_ops_per_step = ti.ops;
  }
  return SUP_OK;
}

int sup_loop_torontonian(const double* O, int M, const double* gamma, const int32_t* modes, int n, uint64_t count,
                         const sup_opts* o, int on_cpu, double* out, sup_stats* st) {
  LtorIn in;
  in.O = O, in.M = M, in.gamma = gamma, in.modes = modes;
  return loop_torontonian_entry(in, n, count, false, 0, 0, o, on_cpu, out, st);
}

int sup_loop_torontonian_range(const double* O, int M, const double* gamma, const int32_t* modes, int n,
                               uint64_t z_begin, uint64_t z_end, const sup_opts* o, int on_cpu, double* out,
                               sup_stats* st) {
  LtorIn in;
  in.O = O, in.M = M, in.gamma = gamma, in.modes = modes;
  return loop_torontonian_entry(in, n, 1, true, z_begin, z_end, o, on_cpu, out, st);
}

int sup_loop_torontonian_plan(int n, uint64_t* subsets, double* est_ops) {
  return loop_torontonian_plan(n, subsets, est_ops);
}

int sup_loop_torontonian_each(const double* O, int M, const double* gamma, uint64_t ngamma, const int32_t* gamma_of,
                              const int32_t* modes, int stride, const int32_t* n, uint64_t count, const sup_opts* o_in,
                              int on_cpu, double* out, sup_stats* st) {
  auto t0 = std::chrono::steady_clock::now();
  sup_opts o;
  if (o_in) o = *o_in;
  else sup_opts_init(&o);
  LtorEachIn in;
  in.O = O, in.M = M, in.gamma = gamma, in.ngamma = ngamma, in.gamma_of = gamma_of, in.modes = modes, in.stride = stride;
  in.n = n;
  TorInfo ti;
  if (int rc = loop_torontonian_each(in, count, o, on_cpu != 0, out, &ti)) return rc;
  if (st) {
    std::memset(st, 0, sizeof(*st));
    st->kernel_ms = ti.kernel_ms;
    st->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    st->gray_steps = ti.subsets;
    st->visited_steps = ti.subsets;
    st->devices_used = ti.devices;
    st->grid = ti.grid;
    st->walk_kind = (int)kWalkDense;
    st->leaves = (int)std::min<uint64_t>(count, 0x7fffffffu);
    st->est_ops_per_step = ti.ops;
  }
  return SUP_OK;
}

int sup_threshold_sample(const double* B, int M, const double* zeta, const double* het, uint64_t nsamples, uint64_t sample0,
                         uint64_t seed, const sup_opts* o_in, int on_cpu, int32_t* out, double* weights, sup_stats* st) {
  auto t0 = std::chrono::steady_clock::now();
  sup_opts o;
  if (o_in) o = *o_in;
  else sup_opts_init(&o);
  ThrInfo gi;
  if (int rc = threshold_sample(B, M, zeta, het, nsamples, sample0, seed, o, on_cpu != 0, out, weights, &gi)) return rc;
  if (st) {
    std::memset(st, 0, sizeof(*st));
    st->kernel_ms = gi.kernel_ms;
    st->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    st->gray_steps = gi.visited;
    st->visited_steps = gi.visited;
    st->devices_used = gi.devices;
    st->walk_kind = (int)kWalkDense;
    st->leaves = (int)std::min<uint64_t>(nsamples, 0x7fffffffu);
    st->est_ops_per_step = gi.ops;
    st->partials[0] = gi.each_ms;         // wall time inside the ragged loop torontonian calls
    st->partials[1] = gi.host_ms;         // wall time of the host stage: lists, gamma rows, weights and draws
    st->partials[2] = (double)gi.failed;  // samples that ended in -1
  }
  return SUP_OK;
}

double sup_ltor_exp(double x) { return ltor_exp(x); }

int sup_ltor_exp_device(const double* x, uint64_t count, double* out, int device_id) {
  if (count == 0) return SUP_OK;
  if (!x || !out) {
    set_error("sup_ltor_exp_device: null pointer");
    return SUP_EINVAL;
  }
  int ndev = 0;
  if (int rc = device_count(&ndev)) return rc;
  if (ndev == 0) {
    set_error("no HIP device available (sup_ltor_exp_device; sup_ltor_exp is the host's)");
    return SUP_ENODEV;
  }
  if (device_id < 0 || device_id >= ndev) {
    set_error("sup_ltor_exp_device: device_id out of range");
    return SUP_EINVAL;
  }
  return run_ltor_exp(device_id, x, count, out);
}

static int torontonian_table_entry(const LtorIn& in, bool loop, int n, int transform, const sup_opts* o_in, int on_cpu,
                                   double* out, sup_stats* st) {
  auto t0 = std::chrono::steady_clock::now();
  sup_opts o;
  if (o_in) o = *o_in;
  else sup_opts_init(&o);
  TorInfo ti;
  if (int rc = torontonian_table(in, loop, n, transform != 0, o, on_cpu != 0, out, &ti)) return rc;
  if (st) {
    std::memset(st, 0, sizeof(*st));
    st->kernel_ms = ti.kernel_ms;
    st->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    st->gray_steps = ti.subsets;
    st->visited_steps = ti.subsets;
    st->devices_used = ti.devices;
    st->grid = ti.grid;
    st->walk_kind = (int)kWalkDense;
    st->leaves = 1;
    st->est_ops_per_step = ti.ops;
  }
  return SUP_OK;
}

int sup_torontonian_table(const double* O, int M, const int32_t* modes, int n, int transform, const sup_opts* o,
                          int on_cpu, double* out, sup_stats* st) {
  LtorIn in;
  in.O = O, in.M = M, in.modes = modes;
  return torontonian_table_entry(in, false, n, transform, o, on_cpu, out, st);
}

int sup_loop_torontonian_table(const double* O, int M, const double* gamma, const int32_t* modes, int n, int transform,
                               const sup_opts* o, int on_cpu, double* out, sup_stats* st) {
  LtorIn in;
  in.O = O, in.M = M, in.gamma = gamma, in.modes = modes;
  return torontonian_table_entry(in, true, n, transform, o, on_cpu, out, st);
}

int sup_mobius_subsets(double* t, int n, const sup_opts* o_in, int on_cpu) {
  sup_opts o;
  if (o_in) o = *o_in;
  else sup_opts_init(&o);
  return mobius_subsets(t, n, o, on_cpu != 0);
}

// sup_stats of a minors call: the batch entry's, with the one-walk step cost.
static void fill_minors_stats(sup_stats* st, const CplxInfo& ci, int n, uint64_t outputs, uint64_t steps,
                              double wall_ms) {
  fill_cplx_stats(st, ci, n, steps, wall_ms);
  if (!st) return;
  st->leaves = (int)std::min<uint64_t>(outputs, 0x7fffffffu);
  st->est_ops_per_step = n <= 32 ? std::max(16.0 * n - 24.0, 0.0) : 6.0 * (n - 1);
}

int sup_perman_complex_minors(const double* U, int R, int C, const int32_t* rows, const int32_t* cols, int n,
                              uint64_t count, const sup_opts* o_in, int on_cpu, double* out, sup_stats* st) {
  auto t0 = std::chrono::steady_clock::now();
  if (!U || !rows || (!cols && n != 1) || !out) {
    set_error("sup_perman_complex_minors: null matrix, index list or output pointer");
    return SUP_EINVAL;
  }
  sup_opts o;
  if (o_in) o = *o_in;
  else sup_opts_init(&o);
  CplxBatchIn in;
  in.U = U, in.R = R, in.C = C, in.rows = rows, in.cols = cols;
  CplxInfo ci;
  if (int rc = cplx_minors(in, n, count, o, on_cpu != 0, out, &ci)) return rc;
  const double wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  // n <= 32: one walk of 2^(q-1) states per matrix; above, n walks of order q
  const uint64_t per = n <= 1 ? 0 : n <= 32 ? 1ull << (n - 2) : (uint64_t)n << (n - 2);
  fill_minors_stats(st, ci, n, count * (uint64_t)n, count * per, wall);
  return SUP_OK;
}

int sup_perman_complex_minors_range(const double* mat, int n, uint64_t c0, uint64_t c1, const sup_opts* o_in,
                                    int on_cpu, double* out, sup_stats* st) {
  auto t0 = std::chrono::steady_clock::now();
  sup_opts o;
  if (o_in) o = *o_in;
  else sup_opts_init(&o);
  CplxInfo ci;
  if (int rc = cplx_minors_range(mat, n, c0, c1, o, on_cpu != 0, out, &ci)) return rc;
  const double wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  fill_minors_stats(st, ci, n, 1, (c1 - c0) << (ci.lay.L + ci.lay.m), wall);
  return SUP_OK;
}

int sup_perman_complex_fock_minors(const double* U, int R, int C, const int32_t* rows, const int32_t* cols, int n,
                                   uint64_t count, const sup_opts* o_in, int on_cpu, double* out, sup_stats* st) {
  auto t0 = std::chrono::steady_clock::now();
  if (!U || !rows || (!cols && n != 1) || !out) {
    set_error("sup_perman_complex_fock_minors: null matrix, index list or output pointer");
    return SUP_EINVAL;
  }
  sup_opts o;
  if (o_in) o = *o_in;
  else sup_opts_init(&o);
  CplxBatchIn in;
  in.U = U, in.R = R, in.C = C, in.rows = rows, in.cols = cols;
  FockInfo fi;
  if (int rc = cplx_fock_minors(in, n, count, o, on_cpu != 0, out, &fi)) return rc;
  if (st) {
    std::memset(st, 0, sizeof(*st));
    st->kernel_ms = fi.kernel_ms;
    st->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    st->gray_steps = n <= 1 ? 0 : count << (n - 2);  // nominal: the one walk over every Gray state
    st->visited_steps = fi.terms;
    st->devices_used = fi.devices;
    st->grid = fi.grid;
    st->walk_kind = (int)kWalkDense;
    st->leaves = (int)std::min<uint64_t>(count * (uint64_t)n, 0x7fffffffu);
    st->est_ops_per_step = std::max(16.0 * n - 20.0, 0.0);
  }
  return SUP_OK;
}

int sup_perman_complex_fock_minors_plan(const int32_t* cols, int n, uint64_t count, uint64_t* terms) {
  return cplx_fock_minors_plan(cols, n, count, terms);
}

// Both samplers: collision_aware picks the per-stage minors entry.
static int boson_sample_entry(const double* U, int M, const int32_t* inputs, int n, uint64_t nsamples, uint64_t seed,
                              const sup_opts* o_in, int on_cpu, int32_t* out, sup_stats* st, bool collision_aware) {
  auto t0 = std::chrono::steady_clock::now();
  sup_opts o;
  if (o_in) o = *o_in;
  else sup_opts_init(&o);
  BosonInfo bi;
  if (int rc = boson_sample(U, M, inputs, n, nsamples, seed, o, on_cpu != 0, out, &bi, collision_aware)) return rc;
  if (st) {
    std::memset(st, 0, sizeof(*st));
    st->kernel_ms = bi.kernel_ms;
    st->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    st->gray_steps = bi.steps;
    st->visited_steps = bi.visited;
    st->devices_used = bi.devices;
    st->walk_kind = (int)kWalkDense;
    st->leaves = (int)std::min<uint64_t>(nsamples, 0x7fffffffu);
    st->est_ops_per_step = std::max(16.0 * n - (collision_aware ? 20.0 : 24.0), 0.0);
    st->partials[0] = bi.minors_ms;  // wall time inside the minors calls
    st->partials[1] = bi.pmf_ms;     // wall time of the host pmf and draw stage
  }
  return SUP_OK;
}

int sup_boson_sample(const double* U, int M, const int32_t* inputs, int n, uint64_t nsamples, uint64_t seed,
                     const sup_opts* o_in, int on_cpu, int32_t* out, sup_stats* st) {
  return boson_sample_entry(U, M, inputs, n, nsamples, seed, o_in, on_cpu, out, st, false);
}

int sup_boson_sample_fock(const double* U, int M, const int32_t* inputs, int n, uint64_t nsamples, uint64_t seed,
                          const sup_opts* o_in, int on_cpu, int32_t* out, sup_stats* st) {
  return boson_sample_entry(U, M, inputs, n, nsamples, seed, o_in, on_cpu, out, st, true);
}

int sup_perman_reduced_exact(const void* mat, sup_dtype t, int n, const sup_opts* o_in, int on_cpu,
                             const sup_reduce_opts* r_in, char* out, size_t out_len, sup_stats* st) {
  auto t0 = std::chrono::steady_clock::now();
  if (!mat || !out || out_len < 2 || n < 1 || n > SUP_MAX_READ_N) {
    set_error("sup_perman_reduced_exact: bad argument");
    return SUP_EINVAL;
  }
  const size_t nn = (size_t)n * n;
  std::vector<double> A(nn);
  for (size_t i = 0; i < nn; ++i)
    A[i] = t == SUP_INT32 ? (double)((const int32_t*)mat)[i]
           : t == SUP_FLOAT32 ? (double)((const float*)mat)[i] : ((const double*)mat)[i];
  sup_opts o;
  if (o_in) o = *o_in;
  else sup_opts_init(&o);
  sup_reduce_opts r;
  if (r_in) r = *r_in;
  else sup_reduce_opts_init(&r);
  std::string s;
  double kms = 0.0;
  int leaves = 0, rc;
  if ((rc = exact_perman_reduced(A.data(), n, o, on_cpu != 0, r, s, &kms, &leaves))) return rc;
  if (s.size() + 1 > out_len) {
    set_error("sup_perman_reduced_exact: output buffer too small");
    return SUP_EINVAL;
  }
  std::memcpy(out, s.c_str(), s.size() + 1);
  if (st) {
    std::memset(st, 0, sizeof(*st));
    st->kernel_ms = kms;
    st->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    st->leaves = leaves;
    st->walk_kind = (int)kWalkDense;
  }
  return SUP_OK;
}

int sup_plan_info(const void* mat, sup_dtype t, int n, sup_kernel kernel, const sup_opts* o_in, int* walk_kind,
                  int* colmap, int* L, int* m, int* cached_bits, int* pair_bits, double* est_ops_per_step) {
  std::vector<double> A;
  int rc = to_double(mat, t, n, A);
  if (rc) return rc;
  sup_opts o;
  if (o_in) o = *o_in;
  else sup_opts_init(&o);
  Plan P;
  if ((rc = check_walk_opts(o))) return rc;
  if ((rc = plan_for(A.data(), n, kernel, layout_for(n, o), P, o.jit, o.gpu_num, o.device_id))) return rc;
  if (walk_kind) *walk_kind = P.lds ? 4 : (int)P.kind;
  if (cached_bits) *cached_bits = P.kind == kWalkSeg ? P.seg_cc : 0;
  if (pair_bits) *pair_bits = P.kind == kWalkSeg ? P.seg_b : 0;
  if (est_ops_per_step) *est_ops_per_step = walk_cost(P);
  if (colmap)
    for (int e = 0; e < n - 1; ++e) colmap[e] = P.colmap[e];
  if (L) *L = P.lay.L;
  if (m) *m = P.lay.m;
  return SUP_OK;
}

static_assert(SUP_CENSUS_CLASSES == kSegCensusN, "superman.h lists the census classes of engine.hpp");

int sup_plan_census(const void* mat, sup_dtype t, int n, sup_kernel kernel, const sup_opts* o_in, int* hi_bits,
                    double* census) {
  std::vector<double> A;
  int rc = to_double(mat, t, n, A);
  if (rc) return rc;
  sup_opts o;
  if (o_in) o = *o_in;
  else sup_opts_init(&o);
  Plan P;
  if ((rc = check_walk_opts(o))) return rc;
  if ((rc = plan_for(A.data(), n, kernel, layout_for(n, o), P, o.jit, o.gpu_num, o.device_id))) return rc;
  const bool seg = P.kind == kWalkSeg;
  if (hi_bits) *hi_bits = seg ? P.seg_hi : 0;
  if (census)
    for (int c = 0; c < kSegCensusN; ++c) census[c] = seg ? P.seg_census[c] : 0.0;
  return SUP_OK;
}

int sup_plan_key(const void* mat, sup_dtype t, int n, sup_kernel kernel, const sup_opts* o_in, uint64_t* key) {
  if (!key) {
    set_error("sup_plan_key: key pointer missing");
    return SUP_EINVAL;
  }
  std::vector<double> A;
  int rc = to_double(mat, t, n, A);
  if (rc) return rc;
  sup_opts o;
  if (o_in) o = *o_in;
  else sup_opts_init(&o);
  Plan P;
  if ((rc = check_walk_opts(o))) return rc;
  if ((rc = plan_for(A.data(), n, kernel, layout_for(n, o), P, o.jit, o.gpu_num, o.device_id))) return rc;
  *key = plan_fingerprint(P);
  return SUP_OK;
}

int sup_prepare(const void* mat, sup_dtype t, int n, sup_kernel kernel, const sup_opts* o_in, int* walk_kind,
                double* compile_ms) {
  std::vector<double> A;
  int rc = to_double(mat, t, n, A);
  if (rc) return rc;
  sup_opts o;
  if (o_in) o = *o_in;
  else sup_opts_init(&o);
  Plan P;
  if ((rc = check_walk_opts(o))) return rc;
  // compiles may already happen while planning (the live-value budget is
  // checked against the compiler), so the time is taken around both
  const double before = jit_compile_ms_thread();
  if ((rc = plan_for(A.data(), n, kernel, layout_for(n, o), P, o.jit, o.gpu_num, o.device_id))) return rc;
  if (walk_kind) *walk_kind = P.lds ? 4 : (int)P.kind;
  if (P.kind == kWalkSeg && (rc = jit_compile_only(P, nullptr))) return rc;
  if (compile_ms) *compile_ms = jit_compile_ms_thread() - before;
  return SUP_OK;
}

// ---- reference-signature wrappers ------------------------------------------
// The reference's sparse wrappers take the caller's CSC (cptrs, rows, cvals)
// and, for SkipPer, CSR (rptrs, cols) next to the dense matrix (built by
// matrix2compressed*, util.h:522-551).  The engine derives its own structure
// from `mat` (touched rows per column, SkipOrder masks), so these arrays must
// describe exactly mat's nonzeros: each column's rows ascending with their
// values, each row's columns ascending.  They are checked, never silently
// ignored: an array built with the reference's `> 0` test (util.h:537,542),
// which drops negative entries, is refused with SUP_EINVAL.
static double entry(const void* mat, sup_dtype t, size_t i) {
  return t == SUP_INT32 ? (double)((const int32_t*)mat)[i]
         : t == SUP_FLOAT32 ? (double)((const float*)mat)[i] : ((const double*)mat)[i];
}

static int check_compressed(const void* mat, sup_dtype t, int n, const int* cptrs, const int* rows,
                            const void* cvals, const int* rptrs, const int* cols) {
  if (!mat || n < 1 || n > SUP_MAX_N) {
    set_error("reference wrapper: null matrix or n outside [1, 64]");
    return SUP_EINVAL;
  }
  if (!cptrs || !rows || !cvals) {
    set_error("reference wrapper: CSC arrays (cptrs, rows, cvals) missing");
    return SUP_EINVAL;
  }
  auto bad = [](const std::string& m) {
    set_error("reference wrapper: " + m + " (build CSR/CSC with sup_compress: nonzero test != 0)");
    return SUP_EINVAL;
  };
  if (cptrs[0] != 0) return bad("cptrs[0] != 0");
  for (int c = 0; c < n; ++c) {
    if (cptrs[c + 1] < cptrs[c]) return bad("cptrs not ascending");
    int want = 0;
    for (int r = 0; r < n; ++r) want += entry(mat, t, (size_t)r * n + c) != 0.0;
    if (cptrs[c + 1] - cptrs[c] != want)
      return bad("column " + std::to_string(c) + " lists " + std::to_string(cptrs[c + 1] - cptrs[c]) +
                 " entries, the matrix has " + std::to_string(want) + " nonzeros");
    for (int k = cptrs[c]; k < cptrs[c + 1]; ++k) {
      const int r = rows[k];
      if (r < 0 || r >= n || (k > cptrs[c] && r <= rows[k - 1])) return bad("CSC rows out of range or order");
      const double v = entry(mat, t, (size_t)r * n + c);
      if (v == 0.0 || entry(cvals, t, (size_t)k) != v)
        return bad("CSC value at (" + std::to_string(r) + ", " + std::to_string(c) + ") differs from the matrix");
    }
  }
  if (rptrs || cols) {
    if (!rptrs || !cols) return bad("CSR arrays incomplete");
    if (rptrs[0] != 0) return bad("rptrs[0] != 0");
    for (int r = 0; r < n; ++r) {
      if (rptrs[r + 1] < rptrs[r]) return bad("rptrs not ascending");
      int want = 0;
      for (int c = 0; c < n; ++c) want += entry(mat, t, (size_t)r * n + c) != 0.0;
      if (rptrs[r + 1] - rptrs[r] != want) return bad("row " + std::to_string(r) + " nonzero count differs");
      for (int k = rptrs[r]; k < rptrs[r + 1]; ++k) {
        const int c = cols[k];
        if (c < 0 || c >= n || (k > rptrs[r] && c <= cols[k - 1]) || entry(mat, t, (size_t)r * n + c) == 0.0)
          return bad("CSR columns out of range, order or pattern");
      }
    }
  }
  return SUP_OK;
}

static int run_ref(const void* mat, sup_dtype t, int nov, sup_kernel k, sup_sched s, int gpu_num, int cpu,
                   int threads, double* out) {
  sup_opts o;
  sup_opts_init(&o);
  o.gpu_num = gpu_num < 1 ? 1 : gpu_num;
  o.cpu_worker = cpu;
  o.threads = threads;
  return sup_perman(mat, t, nov, k, s, &o, out, nullptr);
}

int sup_gpu_perman64_xshared_coalescing_mshared(const void* mat, sup_dtype t, int nov, int, int, double* out) {
  return run_ref(mat, t, nov, SUP_KERNEL_DENSE, SUP_SCHED_SINGLE, 1, 0, 16, out);
}
int sup_gpu_perman64_xshared_coalescing_mshared_multigpu(const void* mat, sup_dtype t, int nov, int gpu_num, int,
                                                         int, double* out) {
  return run_ref(mat, t, nov, SUP_KERNEL_DENSE, SUP_SCHED_STATIC, gpu_num, 0, 16, out);
}
int sup_gpu_perman64_xshared_coalescing_mshared_multigpucpu_chunks(const void* mat, sup_dtype t, int nov,
                                                                   int gpu_num, int cpu, int threads, int, int,
                                                                   double* out) {
  return run_ref(mat, t, nov, SUP_KERNEL_DENSE, SUP_SCHED_CHUNKS, gpu_num, cpu, threads, out);
}
int sup_gpu_perman64_xshared_coalescing_mshared_multigpu_manual_distribution(const void* mat, sup_dtype t, int nov,
                                                                             int gpu_num, int, int, double* out) {
  return run_ref(mat, t, nov, SUP_KERNEL_DENSE, SUP_SCHED_MANUAL, gpu_num, 0, 16, out);
}
int sup_gpu_perman64_xshared_coalescing_mshared_sparse(const void* mat, const int* cptrs, const int* rows,
                                                       const void* cvals, sup_dtype t, int nov, int, int,
                                                       double* out) {
  int rc = check_compressed(mat, t, nov, cptrs, rows, cvals, nullptr, nullptr);
  return rc ? rc : run_ref(mat, t, nov, SUP_KERNEL_SPARYSER, SUP_SCHED_SINGLE, 1, 0, 16, out);
}
int sup_gpu_perman64_xshared_coalescing_mshared_multigpu_sparse(const void* mat, const int* cptrs, const int* rows,
                                                                const void* cvals, sup_dtype t, int nov, int gpu_num,
                                                                int, int, double* out) {
  int rc = check_compressed(mat, t, nov, cptrs, rows, cvals, nullptr, nullptr);
  return rc ? rc : run_ref(mat, t, nov, SUP_KERNEL_SPARYSER, SUP_SCHED_STATIC, gpu_num, 0, 16, out);
}
int sup_gpu_perman64_xshared_coalescing_mshared_multigpucpu_chunks_sparse(const void* mat, const int* cptrs,
                                                                          const int* rows, const void* cvals,
                                                                          sup_dtype t, int nov, int gpu_num, int cpu,
                                                                          int threads, int, int, double* out) {
  int rc = check_compressed(mat, t, nov, cptrs, rows, cvals, nullptr, nullptr);
  return rc ? rc : run_ref(mat, t, nov, SUP_KERNEL_SPARYSER, SUP_SCHED_CHUNKS, gpu_num, cpu, threads, out);
}
int sup_gpu_perman64_xshared_coalescing_mshared_multigpu_sparse_manual_distribution(const void* mat, const int* cptrs,
                                                                                    const int* rows, const void* cvals,
                                                                                    sup_dtype t, int nov, int gpu_num,
                                                                                    int, int, double* out) {
  int rc = check_compressed(mat, t, nov, cptrs, rows, cvals, nullptr, nullptr);
  return rc ? rc : run_ref(mat, t, nov, SUP_KERNEL_SPARYSER, SUP_SCHED_MANUAL, gpu_num, 0, 16, out);
}
int sup_gpu_perman64_xshared_coalescing_mshared_skipper(const void* mat, const int* rptrs, const int* cols,
                                                        const int* cptrs, const int* rows, const void* cvals,
                                                        sup_dtype t, int nov, int, int, double* out) {
  int rc = check_compressed(mat, t, nov, cptrs, rows, cvals, rptrs, cols);
  return rc ? rc : run_ref(mat, t, nov, SUP_KERNEL_SKIPPER, SUP_SCHED_SINGLE, 1, 0, 16, out);
}
int sup_gpu_perman64_xshared_coalescing_mshared_multigpucpu_chunks_skipper(const void* mat, const int* rptrs,
                                                                           const int* cols, const int* cptrs,
                                                                           const int* rows, const void* cvals,
                                                                           sup_dtype t, int nov, int gpu_num, int cpu,
                                                                           int threads, int, int, double* out) {
  int rc = check_compressed(mat, t, nov, cptrs, rows, cvals, rptrs, cols);
  return rc ? rc : run_ref(mat, t, nov, SUP_KERNEL_SKIPPER, SUP_SCHED_CHUNKS, gpu_num, cpu, threads, out);
}


// ---- reductions + engine (sup_decompose with engine leaves) ----------------
namespace {
struct LeafCtx {
  sup_kernel kernel;
  sup_sched sched;
  sup_opts o;
  int on_cpu;
  int preprocessing;
  sup_stats acc;
  bool first = true;
};

int leaf_compute(const LeafCtx& c, const double* a, int n, double* out, sup_stats* st) {
  std::vector<double> m(a, a + (size_t)n * n);
  std::vector<int> rp(n), cp(n);
  int rc = SUP_OK;
  // main.cpp:983-988: every leaf's CSR/CSC is built with the -r order
  if (c.preprocessing == 1) rc = sup_sort_order(m.data(), SUP_FLOAT64, n, cp.data());
  else if (c.preprocessing == 2) rc = sup_skip_order(m.data(), SUP_FLOAT64, n, rp.data(), cp.data());
  if (rc) return rc;
  return c.on_cpu ? sup_perman_cpu(m.data(), SUP_FLOAT64, n, c.kernel, c.o.threads, out, st)
                  : sup_perman(m.data(), SUP_FLOAT64, n, c.kernel, c.sched, &c.o, out, st);
}

// Whether the leaves of this request may share launches (run_range_batch):
// one device, the single-device schedule, a kernel request the batch kernels
// serve, and no checkpoint.  Leaves whose plan turns out otherwise (a
// segmented or SkipPer plan) still go one at a time.
int leaf_workers();
int leaf_batch_max();
bool leaf_batching(const LeafCtx& c) {
  if (leaf_batch_max() <= 1) return false;
  return !c.on_cpu && c.sched == SUP_SCHED_SINGLE && c.o.use_rccl <= 0 && !(c.o.checkpoint && *c.o.checkpoint) &&
         (c.kernel == SUP_KERNEL_DENSE || c.kernel == SUP_KERNEL_SPARYSER || c.kernel == SUP_KERNEL_DENSE_PLAIN);
}
// Default: batches of 16.  Measured on dwt_59 (145,798 n = 30 leaves, one
// MI355X): round 4, one worker 65.2 s -> 46.7 s with batches of 16, but with 8
// workers the concurrent one-leaf launches filled the GPU (37.8 s against
// 39.6 s batched), so batches were for one worker only.  Since round 5 the
// prefix-blocked walk ends ~64 % of these leaves' chunks at their first state
// (walk_sparse.hip): the leaves are short, launches and host planning weigh
// more, and batches win at every worker count — 8 workers 17.9 s one leaf per
// launch, 12.7 s batched; one worker 48.1 s / 16.8 s
// (profiles/r5/probe_reduce_chunk_ends.log).
int leaf_batch_max() {
  const char* e = std::getenv("SUP_LEAF_BATCH");
  if (e) return std::max(1, std::min(kMaxBatchLeaves, std::atoi(e)));
  return 16;
}

// Several leaves of order n: each planned as sup_perman plans it (the same
// plan, so the same bits), the batchable ones walked in one launch, the rest
// one at a time through sup_perman.
// A batch of leaves planned on the host (leaf_plan_batch), walked later
// (leaf_walk_batch), so a worker can plan the next batch while this one walks
// (decompose_batched_staged).  Each leaf is planned as sup_perman plans it
// (the same plan, so the same bits); the batchable ones walk in one launch,
// the rest one at a time through sup_perman.
struct LeafBatchState {
  int n = 0;
  std::vector<std::vector<double>> ms;
  std::vector<std::shared_ptr<const Plan>> plans;
  std::vector<double*> outs;
  std::chrono::steady_clock::time_point t0;
};

int leaf_plan_batch(const LeafCtx& c, const std::vector<const double*>& mats, int n, const std::vector<double*>& outs,
                    LeafBatchState& b) {
  b.t0 = std::chrono::steady_clock::now();
  const size_t K = mats.size();
  b.n = n;
  b.outs = outs;
  b.ms.assign(K, {});
  b.plans.assign(K, nullptr);
  const Layout lay = layout_for(n, c.o);
  int rc = check_walk_opts(c.o);
  if (rc) return rc;
  for (size_t i = 0; i < K; ++i) {
    b.ms[i].assign(mats[i], mats[i] + (size_t)n * n);
    std::vector<int> rp(n), cp(n);
    if (c.preprocessing == 1) rc = sup_sort_order(b.ms[i].data(), SUP_FLOAT64, n, cp.data());
    else if (c.preprocessing == 2) rc = sup_skip_order(b.ms[i].data(), SUP_FLOAT64, n, rp.data(), cp.data());
    if (rc) return rc;
    // batch leaves stay out of the process plan cache (32 entries): two batches of 16 would evict the
    // caller's plans; a repeated leaf is served by the reduction's leaf memo
    if ((rc = plan_for_shared(b.ms[i].data(), n, c.kernel, lay, b.plans[i], c.o.jit, 1, c.o.device_id, false)))
      return rc;
  }
  return SUP_OK;
}

int leaf_walk_batch(const LeafCtx& c, const LeafBatchState& b, sup_stats* st) {
  const size_t K = b.ms.size();
  const int n = b.n;
  const auto& ms = b.ms;
  const auto& plans = b.plans;
  const auto& outs = b.outs;
  const auto t0 = b.t0;
  int rc = SUP_OK;
  std::memset(st, 0, sizeof(*st));
  const double sign = (double)(4 * (n & 1) - 2);  // gpu_exact_dense.cu:698
  std::vector<const Plan*> group;
  std::vector<size_t> gi;
  double kms = 0.0;
  uint64_t steps = 0;
  for (size_t i = 0; i < K; ++i) {
    if (K > 1 && batchable(*plans[i], *plans[i])) {
      if (group.empty() || batchable(*group[0], *plans[i])) {
        group.push_back(plans[i].get());
        gi.push_back(i);
        continue;
      }
    }
    sup_stats one;  // not batchable with the group: on its own, as before
    if ((rc = sup_perman(ms[i].data(), SUP_FLOAT64, n, c.kernel, c.sched, &c.o, outs[i], &one))) return rc;
    kms += one.kernel_ms;
    steps += one.gray_steps;
    st->walk_kind = one.walk_kind;
  }
  if (!group.empty()) {
    std::vector<double> part;
    double ms_b = 0.0;
    if ((rc = run_range_batch(c.o.device_id, group, part, &ms_b))) return rc;
    for (size_t q = 0; q < gi.size(); ++q) *outs[gi[q]] = sign * part[q];
    kms += ms_b;
    steps += (uint64_t)gi.size() << (n - 1);
    st->walk_kind = (int)group[0]->kind;
    st->lane_bits = group[0]->lay.L;
    st->walk_bits = group[0]->lay.m;
    st->est_ops_per_step = walk_cost(*group[0]);
  }
  st->kernel_ms = kms;
  st->gray_steps = steps;
  st->visited_steps = steps;
  st->devices_used = 1;
  st->leaves = (int)K;
  st->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return SUP_OK;
}


void leaf_accumulate(LeafCtx& c, const sup_stats& st) {
  if (c.first) {
    c.acc = st;
    c.first = false;
  } else {
    const sup_stats prev = c.acc;
    c.acc = st;
    c.acc.kernel_ms += prev.kernel_ms;
    c.acc.wall_ms += prev.wall_ms;
    c.acc.gray_steps += prev.gray_steps;
    c.acc.visited_steps += prev.visited_steps;
    c.acc.leaves += prev.leaves;
  }
}

// Concurrent GPU leaves of sup_perman_reduced: one per context lane (8; dwt_59's
// 145,798 n = 30 leaves: 85 s one at a time, 41 s with 4, 39 s with 8,
// profiles/r3/probe_reduce_memo.log).  SUP_LEAF_WORKERS overrides; 1 = one leaf
// at a time, as the reference's RunAlgo per leaf.
int leaf_workers() {
  const char* e = std::getenv("SUP_LEAF_WORKERS");
  return e ? std::max(1, std::min(kCtxLanes, std::atoi(e))) : kCtxLanes;
}

}  // namespace

int sup_perman_reduced_quad(const void* mat, sup_dtype t, int n, const sup_opts* o_in, int on_cpu,
                            const sup_reduce_opts* r_in, double* out_hi, double* out_lo, sup_stats* st) {
  auto t0 = std::chrono::steady_clock::now();
  if (!mat || !out_hi || n < 1 || n > SUP_MAX_READ_N) {
    set_error("sup_perman_reduced_quad: bad argument");
    return SUP_EINVAL;
  }
  std::vector<double> A((size_t)n * n);
  for (size_t i = 0; i < A.size(); ++i)
    A[i] = t == SUP_INT32 ? (double)((const int32_t*)mat)[i]
           : t == SUP_FLOAT32 ? (double)((const float*)mat)[i] : ((const double*)mat)[i];
  sup_opts o;
  if (o_in) o = *o_in;
  else sup_opts_init(&o);
  sup_reduce_opts r;
  if (r_in) r = *r_in;
  else sup_reduce_opts_init(&r);
  double kms = 0.0;
  int used = 0;
  std::mutex mu;
  // GPU leaves several at a time on their own context lanes (as sup_perman_reduced)
  auto leaf = [&](int w, const double* a, int k, dd* v) {
    set_ctx_lane(w);
    double ms = 0.0;
    int u = 0;
    const int rc = quad_perman(a, k, o, on_cpu != 0, &v->hi, &v->lo, &ms, &u);
    std::lock_guard<std::mutex> g(mu);
    kms += ms;
    used = std::max(used, u);
    return rc;
  };
  dd v{0.0, 0.0};
  int leaves = 0;
  const int rc = decompose_dd_batched(A.data(), n, r, on_cpu ? 1 : leaf_workers(), leaf, &v, &leaves);
  if (rc) return rc;
  *out_hi = v.hi;
  if (out_lo) *out_lo = v.lo;
  if (st) {
    std::memset(st, 0, sizeof(*st));
    st->kernel_ms = kms;
    st->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    st->devices_used = used;
    st->walk_kind = (int)kWalkDense;
    st->leaves = leaves;
  }
  return SUP_OK;
}

int sup_perman_reduced(const void* mat, sup_dtype t, int n, sup_kernel kernel, sup_sched sched, const sup_opts* o_in,
                       int on_cpu, const sup_reduce_opts* r_in, double* out, sup_stats* st) {
  LeafCtx c;
  c.kernel = kernel;
  c.sched = sched;
  if (o_in) c.o = *o_in;
  else sup_opts_init(&c.o);
  if (c.o.checkpoint && *c.o.checkpoint) {  // one file per computation; a reduction runs many
    set_error("sup_perman_reduced: checkpoint files are for one permanent (sup_perman with SUP_SCHED_CHUNKS)");
    return SUP_EUNSUPPORTED;
  }
  c.on_cpu = on_cpu;
  sup_reduce_opts r;
  if (r_in) r = *r_in;
  else sup_reduce_opts_init(&r);
  c.preprocessing = r.preprocessing;
  std::memset(&c.acc, 0, sizeof(c.acc));
  int leaves = 0;
  // GPU leaves: leaf_workers() host threads, each on its own context lane of
  // the devices (stream, buffers), so one leaf's planning, uploads, launch
  // gaps and sync overlap the others' walks; host leaves (-c) one at a time
  // (each uses the -t threads).  Same result bits either way: the combine is
  // folded in the sequential order (decompose_batched).
  if (!mat || !out || n < 1 || n > SUP_MAX_READ_N) {
    set_error("sup_perman_reduced: bad argument");
    return SUP_EINVAL;
  }
  std::vector<double> A((size_t)n * n);
  for (size_t i = 0; i < A.size(); ++i)
    A[i] = t == SUP_INT32 ? (double)((const int32_t*)mat)[i]
           : t == SUP_FLOAT32 ? (double)((const float*)mat)[i] : ((const double*)mat)[i];
  std::mutex smu;
  // leaves in batches of up to leaf_batch_max() per launch (run_range_batch),
  // else one at a time; either way the same bits
  const int rc =
      leaf_batching(c)
          // two stages: a worker plans its next batch while its walker thread walks this one
          ? decompose_batched_staged(
                A.data(), n, r, leaf_workers(), leaf_batch_max(),
                [&c, &smu](int w, const std::vector<const double*>& as, int k, const std::vector<double*>& vs,
                           std::function<int()>& walk) {
                  set_ctx_lane(w);
                  auto b = std::make_shared<LeafBatchState>();
                  if (const int e = leaf_plan_batch(c, as, k, vs, *b)) return e;
                  walk = [&c, &smu, b, w]() {
                    set_ctx_lane(w);
                    sup_stats st;
                    if (const int e = leaf_walk_batch(c, *b, &st)) return e;
                    std::lock_guard<std::mutex> g(smu);
                    leaf_accumulate(c, st);
                    return SUP_OK;
                  };
                  return SUP_OK;
                },
                out, &leaves)
          : decompose_batched(A.data(), n, r, c.on_cpu ? 1 : leaf_workers(),
                              [&c, &smu](int w, const double* a, int k, double* v) {
                                set_ctx_lane(w);
                                sup_stats st;
                                const int e = leaf_compute(c, a, k, v, &st);
                                if (e) return e;
                                std::lock_guard<std::mutex> g(smu);
                                leaf_accumulate(c, st);
                                return SUP_OK;
                              },
                              out, &leaves);
  if (rc) return rc;
  if (st) {
    *st = c.acc;
    st->leaves = leaves;
  }
  return SUP_OK;
}

}  // extern "C"
