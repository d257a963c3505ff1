// engine.cpp — the device layer: logical devices and per-device contexts, the
// deferred timing tally, and the launch paths that walk a plan's wave-chunks
// (run_range, run_range_batch, run_range_exact, run_range_dd, warm_devices).
// Plans come from plan.cpp; the schedulers that call these are schedule.cpp.
#include "engine.hpp"
#include "hafnian_exact.hpp"
#include "hafnian_pt.hpp"
#include "hafnian_quad.hpp"
#include "lhaf_table.hpp"
#include "loop_torontonian.hpp"
#include "torontonian.hpp"
#include "torontonian_table.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <mutex>

namespace sup {

// Deferred walk timing (set_defer_timing): event pairs recorded around walks
// whose times are read later (kernel_time).  A pair is pending only once its
// end event was recorded (commit), and a drain that fails partway has already
// moved the pairs it read out of `pending`: no error path leaves an
// unrecorded or twice-counted pair behind.
struct EventTally {
  typedef std::pair<hipEvent_t, hipEvent_t> Pair;
  std::vector<Pair> pending, free;  // recorded and not yet read; ready for reuse
  double sum = 0.0;                 // ms and number of the pairs read since kernel_time
  uint64_t count = 0;
  int take(Pair* ev) {  // a pair to record around a walk; it stays free until commit()
    if (free.empty()) {
      Pair e;
      SUP_HIP(hipEventCreate(&e.first));
      SUP_HIP(hipEventCreate(&e.second));
      free.push_back(e);
    }
    *ev = free.back();
    return SUP_OK;
  }
  void commit() {  // both events of take()'s pair are recorded
    pending.push_back(free.back());
    free.pop_back();
  }
  int drain(bool wait) {  // read the pending pairs in order: all, waiting for each, or the finished ones
    size_t k = 0;
    hipError_t deferred_timing = hipSuccess;  // named for SUP_HIP's message
    for (; k < pending.size(); ++k) {
      if (wait ? (deferred_timing = hipEventSynchronize(pending[k].second)) != hipSuccess
               : hipEventQuery(pending[k].second) != hipSuccess)
        break;
      float m = 0.f;
      if ((deferred_timing = hipEventElapsedTime(&m, pending[k].first, pending[k].second)) != hipSuccess) break;
      sum += m;
      ++count;
      free.push_back(pending[k]);
    }
    pending.erase(pending.begin(), pending.begin() + (long)k);
    SUP_HIP(deferred_timing);
    return SUP_OK;
  }
};

// -------------------------------------------------------- device contexts --
struct DeviceCtx {
  int dev = 0;   // logical id (the API's)
  int phys = 0;  // the HIP device it runs on (phys_device)
  int cus = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  EventTally tally;
  double* d_cols = nullptr;
  size_t cols_cap = 0;
  double* d_jtab = nullptr;
  size_t jtab_cap = 0;
  double* d_start = nullptr;  // the segmented walk's start table (Plan::start_tab)
  size_t start_cap = 0;
  double* d_x0 = nullptr;
  int* d_nblk = nullptr;
  uint64_t* d_rowmask = nullptr;
  double* d_chunk = nullptr;
  size_t chunk_cap = 0;
  double* d_scratch = nullptr;
  size_t scratch_cap = 0;
  unsigned* d_visited = nullptr;
  double* d_wave = nullptr;   // exact path: per-wave residues
  size_t wave_cap = 0;
  double* d_x0dd = nullptr;   // two-block start vectors: double-double walk (hi, lo), complex walk (re, im)
  size_t x0dd_cap = 0;
  size_t visited_cap = 0;
  // queue heads and the fused fold's visited accumulator: head 0 at [0], head 1
  // at [16] (own 64-byte lines), the accumulator (u64) at byte 128
  unsigned* d_counter = nullptr;
  bool head_zero[2] = {false, false};  // head known to be 0 (zeroed by the last run_range's reduction)
  int head = 0;                        // run_range's head for the next fused-fold walk
  unsigned* d_foldcnt = nullptr;       // the fused fold's arrival counters (zero between launches)
  size_t foldcnt_cap = 0;
  double* d_result = nullptr;
  double* h_result = nullptr;  // pinned host slot (mapped): the reduction writes the result here
  double* m_result = nullptr;  // its device address (nullptr: copy from d_result instead)
  unsigned* h_flag = nullptr;  // beside h_result: the sequence number of the last call whose result is there
  unsigned* m_flag = nullptr;
  unsigned flag_seq = 0;
  // leaf batches (run_range_batch): packed tables, descriptors, results
  double* d_batch = nullptr;
  size_t batch_cap = 0;
  LeafDesc* d_desc = nullptr;
  size_t desc_cap = 0;
  double* d_bres = nullptr;
  size_t bres_cap = 0;
  double* h_bres = nullptr;  // pinned, kMaxBatchLeaves doubles
  int occ_batch[2][SUP_MAX_N + 1] = {};
  // batched complex walk (run_cplx_batch): a slab's tables + start vectors,
  // its raw matrices or index lists, the submatrix form's U, its results
  double* d_cbtab = nullptr;
  size_t cbtab_cap = 0;
  double* d_cbmat = nullptr;
  size_t cbmat_cap = 0;
  int32_t* d_cbidx = nullptr;
  size_t cbidx_cap = 0;
  double* d_cbU = nullptr;
  size_t cbU_cap = 0;
  double* d_cbout = nullptr;
  size_t cbout_cap = 0;
  // collision-aware complex walk (run_cplx_fock): a slab's step programs,
  // digits, descriptors and the weight table, packed (16-byte units)
  uint4* d_fock = nullptr;
  size_t fock_cap = 0;
  uint64_t tables_uid = 0;  // Plan::uid whose cols / x0 / nblk / rowmask / jtab the device holds
  std::mutex mu;
  int occ[3][SUP_MAX_N + 1] = {};  // AOT kernels; segmented walk: jit_occupancy
};

static std::mutex g_ctx_mu;
static std::vector<std::unique_ptr<DeviceCtx>> g_ctx;  // [logical device * kCtxLanes + lane]

// Context lane of the calling thread (set_ctx_lane): host threads that run
// independent permanents at once on one device (the -o leaves, engine_leaf)
// each take their own lane — own stream, buffers and queue counter — so their
// launches, copies and syncs overlap instead of queueing on one context.
static thread_local int t_ctx_lane = 0;
void set_ctx_lane(int lane) { t_ctx_lane = std::max(0, std::min(kCtxLanes - 1, lane)); }
int ctx_lane() { return t_ctx_lane; }

// Deferred walk timing (sup_opts.timing = 0, sup_perman_shard): run_range
// records its walk's HIP events as usual but does not wait for the end event
// — the call returns once its result is there, while the kernel's last waves
// may still be exiting — and kernel_time reads the deferred pairs later.
static thread_local bool t_defer_timing = false;
void set_defer_timing(bool on) { t_defer_timing = on; }

// Logical devices.  Every device id of the API (sup_opts::device_id, the
// devices of a multi-device schedule) is a logical id; SUP_DEVICE_MAP (a
// comma list of physical ids, e.g. "0,0,0,0") puts several logical devices on
// one physical GPU, each with its own context (stream, buffers, queue), so the
// multi-device schedulers' per-device threads, combines and item queues run —
// concurrently — on a one-GPU machine.  Unset: logical = physical.  RCCL needs
// distinct physical devices (rccl_allreduce_slots refuses a duplicated map).
static std::vector<int> device_map() {
  std::vector<int> m;
  const char* e = std::getenv("SUP_DEVICE_MAP");
  if (!e || !*e) return m;
  for (const char* p = e; *p;) {
    char* end = nullptr;
    const long v = std::strtol(p, &end, 10);
    if (end == p || v < 0 || v > 1023) return {-1};  // malformed: device_count reports it
    m.push_back((int)v);
    p = *end == ',' ? end + 1 : end;
    if (*end && *end != ',') return {-1};
  }
  return m;
}

int phys_device(int dev) {
  const std::vector<int> m = device_map();
  return (m.empty() || dev < 0 || dev >= (int)m.size()) ? dev : m[dev];
}

static thread_local int t_logical = -1;  // the logical device this thread last selected

hipError_t select_device(int dev) {
  const hipError_t e = hipSetDevice(phys_device(dev));
  t_logical = e == hipSuccess ? dev : -1;
  return e;
}

static bool check_device_on() { static const bool on = env_on("SUP_CHECK_DEVICE", false); return on; }  // read once
static std::atomic<uint64_t> g_device_checks{0};

int check_device(int dev, const char* what) {
  if (!check_device_on()) return SUP_OK;
  int cur = -1;
  const int want = phys_device(dev);
  if (hipGetDevice(&cur) != hipSuccess || cur != want || t_logical != dev) {
    set_error(std::string("SUP_CHECK_DEVICE: ") + what + " for logical device " + std::to_string(dev) +
              " (physical " + std::to_string(want) + ") on a thread whose HIP device is " + std::to_string(cur) +
              " and whose last selected logical device is " + std::to_string(t_logical));
    return SUP_EHIP;
  }
  g_device_checks.fetch_add(1, std::memory_order_relaxed);
  return SUP_OK;
}

uint64_t device_checks_passed() { return g_device_checks.load(); }

int device_count(int* n) {
  int c = 0;
  hipError_t e = hipGetDeviceCount(&c);
  if (e != hipSuccess) {
    *n = 0;
    set_error(std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
    return SUP_ENODEV;
  }
  const std::vector<int> m = device_map();
  if (!m.empty() && c > 0) {
    for (int p : m)
      if (p < 0 || p >= c) {
        *n = 0;
        set_error("SUP_DEVICE_MAP must be a comma list of existing physical device ids (" + std::to_string(c) +
                  " visible)");
        return SUP_ENODEV;
      }
    c = (int)m.size();
  }
  *n = c;
  return SUP_OK;
}

static int get_ctx(int dev, DeviceCtx** out) {
  int cnt = 0;
  int rc = device_count(&cnt);
  if (rc) return rc;
  if (cnt == 0) {
    set_error("no HIP device available (the engine has no CPU fallback for GPU algorithms)");
    return SUP_ENODEV;
  }
  if (dev < 0 || dev >= cnt) {
    set_error("device id " + std::to_string(dev) + " out of range (" + std::to_string(cnt) + " devices)");
    return SUP_ENODEV;
  }
  const int pd = phys_device(dev);
  const size_t slot = (size_t)dev * kCtxLanes + (size_t)t_ctx_lane;
  std::lock_guard<std::mutex> g(g_ctx_mu);
  if (g_ctx.size() < (size_t)cnt * kCtxLanes) g_ctx.resize((size_t)cnt * kCtxLanes);
  if (g_ctx[slot] && g_ctx[slot]->phys != pd) {
    set_error("logical device " + std::to_string(dev) + " moved to another physical device (SUP_DEVICE_MAP "
              "changed after first use)");
    return SUP_EINVAL;
  }
  if (!g_ctx[slot]) {
    auto c = std::make_unique<DeviceCtx>();
    c->dev = dev;
    c->phys = pd;
    SUP_HIP(select_device(dev));
    SUP_ON_DEVICE(dev, "context allocations");
    hipDeviceProp_t prop;
    SUP_HIP(hipGetDeviceProperties(&prop, pd));
    c->cus = prop.multiProcessorCount;
    SUP_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    SUP_HIP(hipEventCreate(&c->ev0));
    SUP_HIP(hipEventCreate(&c->ev1));
    SUP_HIP(hipMalloc(&c->d_x0, SUP_MAX_N * sizeof(double)));
    SUP_HIP(hipMalloc(&c->d_nblk, SUP_MAX_N * sizeof(int)));
    SUP_HIP(hipMalloc(&c->d_rowmask, SUP_MAX_N * sizeof(uint64_t)));
    SUP_HIP(hipMalloc(&c->d_counter, 256));
    // zeroed on the context's own stream: a null-stream hipMemset is not ordered
    // with this non-blocking stream and could land after the first walk began
    SUP_HIP(hipMemsetAsync(c->d_counter, 0, 256, c->stream));
    SUP_HIP(hipStreamSynchronize(c->stream));
    SUP_HIP(hipMalloc(&c->d_result, 64));
    // the result slot is host memory the device writes directly (mapped,
    // coherent): the reduction's last pass stores the partial there, so no
    // D2H copy is queued per call; d_result stays for the -R slot copy
    SUP_HIP(hipHostMalloc(&c->h_result, 64, hipHostMallocMapped | hipHostMallocCoherent));
    if (hipHostGetDevicePointer((void**)&c->m_result, c->h_result, 0) != hipSuccess) c->m_result = nullptr;
    c->h_flag = reinterpret_cast<unsigned*>(c->h_result + 1);
    *c->h_flag = 0u;
    c->m_flag = c->m_result ? reinterpret_cast<unsigned*>(c->m_result + 1) : nullptr;
    g_ctx[slot] = std::move(c);
  }
  *out = g_ctx[slot].get();
  return SUP_OK;
}

// The calling thread's context on logical device `dev`, locked for the guard's
// life, with the device selected on this thread; `what` (optional): what the
// caller is about to do, for the SUP_CHECK_DEVICE check.
struct CtxGuard {
  DeviceCtx* c = nullptr;
  std::unique_lock<std::mutex> lock;
  int open(int dev, const char* what) {
    if (int rc = get_ctx(dev, &c)) return rc;
    lock = std::unique_lock<std::mutex>(c->mu);
    SUP_HIP(select_device(c->dev));
    if (what) SUP_ON_DEVICE(c->dev, what);
    return SUP_OK;
  }
};

// Device warm-up (sup_device_warmup): the HIP runtime's initialisation,
// each device's context (stream, events, buffers) and the ahead-of-time walk
// code objects of order n, so a caller can overlap them with its host-side
// planning instead of paying them after it.
int warm_devices(int first, int count, int n) {
  for (int d = first; d < first + count; ++d) {
    CtxGuard g;
    if (int rc = g.open(d, nullptr)) return rc;
    if (n >= 1 && n <= SUP_MAX_N)
      for (WalkKind k : {kWalkDense, kWalkSparse}) {
        int b = 0;
        SUP_HIP(walk_occupancy(k, n, &b));
      }
  }
  return SUP_OK;
}

// The deferred walk times of the calling thread's context on logical device
// `dev` since the last read: waits for their end events, returns their sum
// and count, and starts a new tally.
int kernel_time(int dev, double* total_ms, uint64_t* launches) {
  CtxGuard g;
  if (int rc = g.open(dev, nullptr)) return rc;
  EventTally& t = g.c->tally;
  if (int rc = t.drain(true)) return rc;
  if (total_ms) *total_ms = t.sum;
  if (launches) *launches = t.count;
  t.sum = 0.0;
  t.count = 0;
  return SUP_OK;
}

// Per-call completion (round 4, tools/probe_launch.hip, profiles/r4/probe_launch_b.log):
// around a 500 us kernel, marker events + one more launch + hipStreamSynchronize
// cost 18.9 us beyond the kernel; waiting instead for a sequence number the
// last kernel stores in mapped host memory, 11.9 us.  (Events carried by the
// launch itself, hipExtModuleLaunchKernel, measured worse: 23.7 / 15.5 us.)
// So a call whose result lands in mapped host memory waits for the sequence
// number the reduction's last pass stores after it; SUP_FLAG_WAIT=0 restores
// the stream sync (A/B).  (These three knobs are read once per process.)
static bool result_flag_wait() { static const bool on = env_on("SUP_FLAG_WAIT", true); return on; }
// The fused fold (run_range; walk_common.hpp chunk_store) is the default;
// SUP_FOLD=0 restores the reduction launches after the walk (A/B: the same
// tree, the same bits).
static bool fold_fused() { static const bool on = env_on("SUP_FOLD", true); return on; }
// Spin on the flag for up to 2 ms (a short walk's wait); false: not seen yet
// (a long walk, or a fault that stopped the stream) — the caller then blocks
// in hipStreamSynchronize, which also reports the stream's error.
static constexpr double kFlagSpinMs = 2.0;
// The fused fold's result slot before a walk whose final fold publishes the
// result itself (WalkParams::fold_sys): a signalling-NaN pattern no fold
// produces in practice (a result that equals it only costs the spin window).
static constexpr uint64_t kResultSentinel = 0x7ff4dead5eedbeefull;
static bool result_sys() { static const bool on = env_on("SUP_RESULT_SYS", true); return on; }
// Spin until done() or the window ends.
template <class F>
static bool spin_wait(F done) {
  const auto t0 = std::chrono::steady_clock::now();
  for (unsigned i = 1;; ++i) {
    if (done()) return true;
    __builtin_ia32_pause();
    if ((i & 255u) == 0 &&
        std::chrono::steady_clock::now() - t0 > std::chrono::microseconds((long)(kFlagSpinMs * 1000.0)))
      return false;
  }
}
static bool wait_result(const double* slot) {
  const uint64_t* w = reinterpret_cast<const uint64_t*>(slot);
  return spin_wait([w] { return __atomic_load_n(w, __ATOMIC_ACQUIRE) != kResultSentinel; });
}
static bool wait_flag(const unsigned* flag, unsigned seq) {
  return spin_wait([flag, seq] { return __atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq; });
}

template <class T>
static int ensure(T*& p, size_t& cap, size_t need) {
  if (need <= cap) return SUP_OK;
  if (p) (void)hipFree(p);
  p = nullptr;
  cap = 0;
  hipError_t e = hipMalloc(&p, need * sizeof(T));
  if (e != hipSuccess) {
    set_error(std::string("hipMalloc: ") + hipGetErrorString(e));
    return SUP_ENOMEM;
  }
  cap = need;
  return SUP_OK;
}

// ------------------------------------------------- launch-path helpers --
// nblk of walk bit k as 4-bit fields, k < 16 in *lo, k >= 16 in *hi
// (WalkParams::nb_lo / nb_hi)
static void pack_nblk(const Plan& P, unsigned long long* lo, unsigned long long* hi) {
  *lo = *hi = 0;
  for (int k = 0; k < P.lay.m && k < 32; ++k) {
    const uint64_t v = (uint64_t)(P.nblk[P.lay.L + k] & 15);
    if (k < 16) *lo |= v << (4 * k);
    else *hi |= v << (4 * (k - 16));
  }
}

// What every walk's parameters share; blocked: with the packed nblk.
static WalkParams walk_params(const Plan& P, const double* cols, const double* x0, uint64_t c0, uint64_t count,
                              unsigned* counter, unsigned group, bool blocked) {
  WalkParams p{};
  p.cols = cols;
  p.x0 = x0;
  p.chunk_begin = c0;
  p.chunk_count = count;
  p.L = P.lay.L;
  p.m = P.lay.m;
  p.n = P.n;
  p.counter = counter;
  p.group = group;
  if (blocked) pack_nblk(P, &p.nb_lo, &p.nb_hi);
  return p;
}

// Blocks of a walk that takes one chunk per wave at a time: the resident
// blocks (occ per CU, at least 1), at most those `count` chunks need, at least one.
static uint64_t capped_grid(const DeviceCtx* c, int occ, uint64_t count) {
  const uint64_t need_blocks = (count + kWavesPerBlock - 1) / kWavesPerBlock;
  return std::max<uint64_t>(1, std::min((uint64_t)c->cus * (uint64_t)std::max(occ, 1), need_blocks));
}

// The exact and double-double walks' own tables (P's columns, their start
// vector x0 into d_x0) replace the cached plan's, and their queue is head 0,
// which they leave nonzero.
static int upload_walk_tables(DeviceCtx* c, const Plan& P, double* d_x0, const std::vector<double>& x0) {
  hipStream_t s = c->stream;
  c->tables_uid = 0;
  SUP_HIP(hipMemcpyAsync(c->d_cols, P.cols.data(), P.cols.size() * sizeof(double), hipMemcpyHostToDevice, s));
  SUP_HIP(hipMemcpyAsync(d_x0, x0.data(), x0.size() * sizeof(double), hipMemcpyHostToDevice, s));
  SUP_HIP(hipMemsetAsync(c->d_counter, 0, sizeof(unsigned), s));
  c->head_zero[0] = false;
  return SUP_OK;
}

// Wait for the stream, then the time between the context's own event pair.
static int timed_sync(DeviceCtx* c, double* kernel_ms) {
  hipStream_t s = c->stream;
  SUP_HIP(hipStreamSynchronize(s));
  float ms = 0.f;
  SUP_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
  if (kernel_ms) *kernel_ms = ms;
  return SUP_OK;
}

// Chunk groups of up to 64 (one lane per partial: a 512-byte store); the
// largest that leaves >= 32 groups per resident wave (tail balance).  n = 40
// on one MI355X: 16 chunks, 128-byte stores (8 chunks: 64-byte partial-line
// stores, 2.5x the partials' bytes in WRITE_SIZE).  A forced group
// (experiments) is rounded down to a power of two <= 64.
// Segmented walk: the last chunks go out in quarter groups, so the waves
// finish within a quarter group of each other (a group of 16 n = 40 chunks
// is ~5 ms of one wave's time).  Smaller tail groups measured 0.25 % faster
// on the headline (tail groups of 4 174.7-174.9 ms, of 2 174.4-174.5, of 1
// 174.3-174.5, profiles/r6/probe_tail_group.log) but each tail chunk then
// costs its own ticket, publish and fold reads: 11.7 -> 16.8 MB of HBM
// traffic per launch (profiles/r6/tail1_hbm_d050.json), so quarter groups stay.
// The tail phase holds ~2 groups per resident wave, rounded to whole groups.
LaunchGeom walk_geometry(uint64_t count, uint64_t resident_blocks, uint64_t waves_per_block, bool seg,
                         int force_group, int force_tail, uint64_t group_cap) {
  const uint64_t res_waves = resident_blocks * waves_per_block;
  LaunchGeom g;
  g.group = 64;
  while (g.group > 1 && (count / ((uint64_t)g.group * res_waves) < 32 || g.group > group_cap)) g.group >>= 1;
  if (force_group > 0) g.group = std::min(64u, 1u << (31 - __builtin_clz((unsigned)force_group)));
  g.tail_group = 0;
  g.tail_begin = count;
  if (seg && g.group >= 2) {
    g.tail_group = force_tail >= 0 ? std::min(g.group, (unsigned)force_tail) : std::max(1u, g.group / 4);
    if (g.tail_group) {
      g.tail_group = 1u << (31 - __builtin_clz(g.tail_group));  // a power of two
      const uint64_t tail = 2 * res_waves * g.group;
      // on a multiple of 64 (so of the group): no 64-group of the fused fold
      // mixes group sizes (walk_common.hpp chunk_store)
      g.tail_begin = count > tail ? (count - tail) / 64 * 64 : 0;
    }
  }
  g.tail_ticket = g.tail_group ? (unsigned)(g.tail_begin / g.group) : 0xffffffffu;
  const uint64_t waves_needed = (count + g.group - 1) / g.group;  // one chunk group per wave at a time
  g.grid = (waves_needed + waves_per_block - 1) / waves_per_block;
  g.grid = std::max<uint64_t>(1, std::min(g.grid, resident_blocks));
  return g;
}

// ---------------------------------- run_range and its steps, in stream order --
// Grow the buffers a walk of `count` chunks of P needs; *grown: a table buffer
// (cols, jtab, start) was reallocated, so its contents are gone (capacities
// are compared, not addresses: a reallocation may return the same address).
static int ensure_walk_buffers(DeviceCtx* c, const Plan& P, uint64_t count, bool visited, bool* grown) {
  const size_t caps = c->cols_cap + c->jtab_cap + c->start_cap;
  const bool seg = P.kind == kWalkSeg;
  int rc;
  if ((rc = ensure(c->d_cols, c->cols_cap, P.cols.size()))) return rc;
  if ((rc = ensure(c->d_chunk, c->chunk_cap, (size_t)count))) return rc;
  if ((rc = ensure(c->d_scratch, c->scratch_cap, (size_t)pairwise_scratch_size(count)))) return rc;
  if (visited && (rc = ensure(c->d_visited, c->visited_cap, (size_t)count))) return rc;
  if (seg && (rc = ensure(c->d_jtab, c->jtab_cap, P.jtab.size()))) return rc;
  if (seg && !P.start_tab.empty() && (rc = ensure(c->d_start, c->start_cap, P.start_tab.size()))) return rc;
  *grown = caps != c->cols_cap + c->jtab_cap + c->start_cap;
  return SUP_OK;
}

// The plan's tables, for the device to hold until another plan's replace them.
static int upload_plan_tables(DeviceCtx* c, const Plan& P) {
  hipStream_t s = c->stream;
  if (P.kind == kWalkSeg)
    SUP_HIP(hipMemcpyAsync(c->d_jtab, P.jtab.data(), P.jtab.size() * sizeof(double), hipMemcpyHostToDevice, s));
  if (P.kind == kWalkSeg && !P.start_tab.empty())
    SUP_HIP(hipMemcpyAsync(c->d_start, P.start_tab.data(), P.start_tab.size() * sizeof(double),
                           hipMemcpyHostToDevice, s));
  SUP_HIP(hipMemcpyAsync(c->d_cols, P.cols.data(), P.cols.size() * sizeof(double), hipMemcpyHostToDevice, s));
  SUP_HIP(hipMemcpyAsync(c->d_x0, P.x0.data(), P.x0.size() * sizeof(double), hipMemcpyHostToDevice, s));
  SUP_HIP(hipMemcpyAsync(c->d_nblk, P.nblk.data(), P.nblk.size() * sizeof(int), hipMemcpyHostToDevice, s));
  SUP_HIP(hipMemcpyAsync(c->d_rowmask, P.rowmask.data(), P.rowmask.size() * sizeof(uint64_t),
                         hipMemcpyHostToDevice, s));
  c->tables_uid = P.uid;
  return SUP_OK;
}

// The fused fold's arrival counters for `count` chunks.
static int ensure_fold_counters(DeviceCtx* c, uint64_t count) {
  // a grown buffer starts at zero (compare capacities: a reallocation may
  // return the same address, with stale contents); zeroed on the context's own
  // stream, which a null-stream memset is not ordered with
  const size_t cap_before = c->foldcnt_cap;
  if (int rc = ensure(c->d_foldcnt, c->foldcnt_cap, (size_t)pairwise_scratch_size(count))) return rc;
  if (c->foldcnt_cap != cap_before)
    SUP_HIP(hipMemsetAsync(c->d_foldcnt, 0, c->foldcnt_cap * sizeof(unsigned), c->stream));
  return SUP_OK;
}

// Resident blocks per CU of P's walk kernel (cached per context; the
// segmented walk: its compiled kernel's, *compile_ms spent on it).
static int walk_occ(DeviceCtx* c, const Plan& P, int* out, double* compile_ms) {
  int occ_seg = 0, occ_lds = 0;
  if (P.kind == kWalkSeg) {
    SUP_ON_DEVICE(c->dev, "segmented-walk module load");
    if (int rc = jit_occupancy(c->phys, P, &occ_seg, compile_ms)) return rc;
  }
  if (P.lds) {  // LDS-staged dense walk: one wave per block, LDS-limited residency
    SUP_HIP(lds_occupancy(P.n, P.lay.m, &occ_lds));
    if (occ_lds < 1) occ_lds = 1;
  }
  int& occ = P.kind == kWalkSeg ? occ_seg : (P.lds ? occ_lds : c->occ[P.kind][P.n]);
  if (occ == 0) {
    int b = 0;
    SUP_HIP(walk_occupancy(P.kind, P.n, &b));
    occ = b > 0 ? b : 1;
  }
  *out = occ;
  return SUP_OK;
}

// SUP_FOLD_CHECK (debugging): every arrival counter back at zero after a fused walk
static int fold_check(DeviceCtx* c, const Plan& P, uint64_t count, const LaunchGeom& g) {
  hipStream_t s = c->stream;
  SUP_HIP(hipStreamSynchronize(s));
  std::vector<unsigned> cc(c->foldcnt_cap);
  SUP_HIP(hipMemcpy(cc.data(), c->d_foldcnt, cc.size() * sizeof(unsigned), hipMemcpyDeviceToHost));
  unsigned hd[64];
  SUP_HIP(hipMemcpy(hd, c->d_counter, 256, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < cc.size(); ++i)
    if (cc[i]) {
      std::fprintf(stderr, "SUP_FOLD_CHECK: counter %zu = %u after a fused walk (kind %d n %d count %llu group %u tail %u/%llu)\n",
                   i, cc[i], (int)P.kind, P.n, (unsigned long long)count, g.group, g.tail_group,
                   (unsigned long long)g.tail_begin);
      break;
    }
  std::fprintf(stderr, "SUP_FOLD_CHECK: kind %d n %d count %llu grid %llu heads %u %u vis %llu result %.17g\n", (int)P.kind,
               P.n, (unsigned long long)count, (unsigned long long)g.grid, hd[0], hd[16],
               *reinterpret_cast<unsigned long long*>(hd + 32), *c->h_result);
  return SUP_OK;
}

// SUP_JIT_TRACE=<file> (diagnostics): the segmented walk's per-wave stamps,
// appended to the file; frees d_trace
static int trace_write(const char* path, unsigned long long* d_trace, uint64_t count, const LaunchGeom& g,
                       uint64_t res_waves, float ms) {
  std::vector<unsigned long long> tr(g.grid * kWavesPerBlock * 8);
  SUP_HIP(hipMemcpy(tr.data(), d_trace, tr.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  SUP_HIP(hipFree(d_trace));
  if (FILE* f = std::fopen(path, "a")) {
    std::fprintf(f, "# launch chunks %llu grid %llu waves_resident %llu group %u tail_group %u kernel_ms %.4f\n",
                 (unsigned long long)count, (unsigned long long)g.grid, (unsigned long long)res_waves, g.group,
                 g.tail_group, ms);
    for (size_t w = 0; w < tr.size() / 8; ++w)
      std::fprintf(f, "%zu %llu %llu %llu %llu %llu %llu\n", w, tr[8 * w], tr[8 * w + 1], tr[8 * w + 2],
                   tr[8 * w + 3], tr[8 * w + 4], tr[8 * w + 5]);
    std::fclose(f);
  }
  return SUP_OK;
}

// Where a walk's result goes and how the host learns that it is there.
struct ResultPath {
  bool fused;    // the walk folds its own partials: no reduction launch follows it
  bool visited;  // the visited sum comes back too (h_result[2])
  bool to_host;  // into mapped host memory (no D2H copy), unless an -R slot copy takes it from d_result
  bool direct;   // ... written there by the last fold or pass itself (old path: one chunk is a copy, not a pass)
  bool flagged;  // ... with a signal the host can wait on: a sequence number, or the slot itself
  unsigned seq;
};

// The fused fold's part of the walk's parameters; its final fold zeroes the
// queue head the walk does not use (qh ^ 1).
static void fold_params(DeviceCtx* c, const ResultPath& rp, int qh, WalkParams* p) {
  p->fold_cnt = c->d_foldcnt;
  p->fold_lv = c->d_scratch;
  p->fold_out = rp.to_host ? c->m_result : c->d_result;
  p->fold_vis = rp.visited ? reinterpret_cast<unsigned long long*>(c->d_counter + 32) : nullptr;
  p->fold_reset = c->d_counter + 16 * (qh ^ 1);
  p->fold_flag = rp.flagged ? c->m_flag : nullptr;
  p->fold_seq = rp.seq;
  if (rp.flagged && result_sys()) {  // the result slot itself is the signal
    p->fold_flag = nullptr;
    p->fold_sys = 1;
    __atomic_store_n(reinterpret_cast<uint64_t*>(c->h_result), kResultSentinel, __ATOMIC_RELEASE);
  }
}

// After the walk: what brings the result to h_result (and the visited sum to
// h_result[2]) where the walk did not write them there itself — the reduction
// launches of the unfused path, D2H copies, the -R slot copy.
static int queue_result_copies(DeviceCtx* c, const ResultPath& rp, uint64_t count, unsigned* head, double* slot) {
  hipStream_t s = c->stream;
  unsigned long long* vsum = reinterpret_cast<unsigned long long*>(c->h_result + 2);
  if (rp.fused) {
    if (!rp.to_host) {
      SUP_HIP(hipMemcpyAsync(c->h_result, c->d_result, sizeof(double), hipMemcpyDeviceToHost, s));
      if (rp.visited)
        SUP_HIP(hipMemcpyAsync(vsum, c->d_result + 2, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    }
  } else {
    // (the -R combine copies d_result into its slot on the device; one chunk is a copy, not a pass)
    SUP_ON_DEVICE(c->dev, "reduction launch");
    SUP_HIP(launch_pairwise_reduce(c->d_chunk, count, c->d_scratch, rp.direct ? c->m_result : c->d_result, s, head,
                                   rp.flagged ? c->m_flag : nullptr, rp.seq));
    if (!rp.direct) SUP_HIP(hipMemcpyAsync(c->h_result, c->d_result, sizeof(double), hipMemcpyDeviceToHost, s));
    // visited states: summed on the device, 8 bytes back (beside the result in
    // the mapped slot: h_result[2])
    if (rp.visited) {
      SUP_HIP(launch_sum_visited(c->d_visited, count, reinterpret_cast<unsigned long long*>(c->d_result + 2), s));
      SUP_HIP(hipMemcpyAsync(vsum, c->d_result + 2, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    }
  }
  if (slot) SUP_HIP(hipMemcpyAsync(slot, c->d_result, sizeof(double), hipMemcpyDeviceToDevice, s));
  return SUP_OK;
}

// The walk's time between the pair `ev`: read now, or (defer) left to the
// tally, whose pending pairs are bounded here by reading the finished ones.
// (After a flag wait the walk's result is there, but its end event may not
// be: waiting for it costs ~8 us per call on config 2 — deferred timing
// leaves it for kernel_time.)
static int walk_time(DeviceCtx* c, bool defer, const EventTally::Pair& ev, float* ms) {
  if (defer) return c->tally.pending.size() >= 256 ? c->tally.drain(false) : SUP_OK;
  hipError_t ee = hipEventElapsedTime(ms, ev.first, ev.second);
  if (ee == hipErrorNotReady) {
    SUP_HIP(hipEventSynchronize(ev.second));
    ee = hipEventElapsedTime(ms, ev.first, ev.second);
  }
  if (ee != hipSuccess) {
    set_error(std::string("hipEventElapsedTime: ") + hipGetErrorString(ee));
    return SUP_EHIP;
  }
  return SUP_OK;
}

int run_range(int dev, const Plan& P, uint64_t c0, uint64_t c1, bool want_visited, RangeResult& r, double* slot) {
  r = RangeResult();
  if (c1 <= c0) return SUP_OK;  // empty range: partial 0
  if (c1 > P.lay.chunks()) {
    set_error("wave-chunk range exceeds the plan");
    return SUP_EINVAL;
  }
  CtxGuard guard;
  int rc = guard.open(dev, "device buffers");
  if (rc) return rc;
  DeviceCtx* c = guard.c;
  hipStream_t s = c->stream;
  const uint64_t count = c1 - c0;
  const bool seg = P.kind == kWalkSeg;
  // walked states per chunk: SkipPer's jumps, the segmented walk's chunk skip
  // (only where the walk leaves rows untouched)
  const bool visited = want_visited && (P.kind == kWalkSkip || (seg && P.outer_tree.tail_hi > P.outer_tree.tail_lo));
  // ... and the prefix-blocked walk's chunk ends: the kernel counts the chunks
  // it ended (kernels.hpp kChunkEndWords), the rest were walked whole
  const bool ends = want_visited && P.kind == kWalkSparse && !P.lds && P.chunk_ends;
  // the plan's tables: uploaded unless this device already holds them (same
  // cached plan, buffers not reallocated) — repeated calls on one matrix
  // (bench steps, -p6 items, reduction leaves) skip five H2D copies
  bool grown = false;
  if ((rc = ensure_walk_buffers(c, P, count, visited, &grown))) return rc;
  if ((P.uid == 0 || P.uid != c->tables_uid || grown) && (rc = upload_plan_tables(c, P))) return rc;
  // The fused fold (walk_common.hpp chunk_store): the walk folds its own
  // partials, so no reduction launch follows it; its final fold zeroes the
  // other queue head, which the next such walk takes (the heads alternate: a
  // wave may still take its last, empty ticket after the fold completes).
  const bool fused = fold_fused() && !P.lds &&
                     (seg || P.kind == kWalkDense || P.kind == kWalkSparse || P.kind == kWalkSkip);
  if (fused && (rc = ensure_fold_counters(c, count))) return rc;
  // the chunk-end words, behind the per-chunk words the unfused chunk_store writes (walk_sparse.hip)
  unsigned* end_words = nullptr;
  if (ends) {
    const size_t first = fused ? 0 : (size_t)count;
    if ((rc = ensure(c->d_visited, c->visited_cap, first + kChunkEndWords))) return rc;
    end_words = c->d_visited + first;
    SUP_HIP(hipMemsetAsync(end_words, 0, kChunkEndWords * sizeof(unsigned), s));
  }
  const int qh = fused ? c->head : 0;
  unsigned* head = c->d_counter + 16 * qh;
  // the queue head: zeroed by the previous run_range's reduction, else here
  if (!c->head_zero[qh]) SUP_HIP(hipMemsetAsync(head, 0, sizeof(unsigned), s));
  c->head_zero[qh] = false;

  int occ = 0;
  if ((rc = walk_occ(c, P, &occ, &r.compile_ms))) return rc;
  const uint64_t wpb = P.lds ? 1 : kWavesPerBlock;             // waves per block
  const uint64_t resident = (uint64_t)c->cus * (uint64_t)occ;  // resident blocks
  const char* fg = std::getenv("SUP_WALK_GROUP");  // experiments, read per call (walk_geometry)
  const char* ft = seg ? std::getenv("SUP_WALK_TAIL") : nullptr;
  const LaunchGeom geo = walk_geometry(count, resident, wpb, seg, fg ? std::max(1, std::atoi(fg)) : 0,
                                       ft ? std::max(0, std::atoi(ft)) : -1);

  WalkParams p = walk_params(P, c->d_cols, c->d_x0, c0, count, head, geo.group, true);
  p.nblk = c->d_nblk;
  p.rowmask = c->d_rowmask;
  p.umask = P.kind == kWalkSparse ? P.chunk_ends : P.umask;  // walk_sparse: its chunk-end rows
  p.chunk_out = c->d_chunk;
  p.visited = (visited && !fused) || ends ? c->d_visited : nullptr;
  p.tail_group = geo.tail_group;
  p.tail_begin = geo.tail_begin;
  p.tail_ticket = geo.tail_ticket;
  p.jtab = seg ? c->d_jtab : nullptr;
  p.start_tab = seg && !P.start_tab.empty() ? c->d_start : nullptr;
  const char* trace_path = seg ? std::getenv("SUP_JIT_TRACE") : nullptr;
  if (trace_path && *trace_path) {
    const size_t bytes = geo.grid * kWavesPerBlock * 8 * sizeof(unsigned long long);
    SUP_HIP(hipMalloc(&p.trace, bytes));
    SUP_HIP(hipMemsetAsync(p.trace, 0, bytes, s));
  }
  ResultPath rp{fused, visited, c->m_result && !slot, false, false, ++c->flag_seq};
  rp.direct = rp.to_host && (fused || count > 1);
  rp.flagged = rp.direct && (fused || !visited) && result_flag_wait();
  if (fused) fold_params(c, rp, qh, &p);

  // launch, between the event pair that times it
  const bool defer = t_defer_timing;
  EventTally::Pair ev(c->ev0, c->ev1);
  if (defer && (rc = c->tally.take(&ev))) return rc;
  SUP_ON_DEVICE(c->dev, "walk launch");
  SUP_HIP(hipEventRecord(ev.first, s));
  if (seg) {
    if ((rc = jit_launch(c->phys, P, p, (int)geo.grid, s))) return rc;
  } else {
    SUP_HIP(P.lds ? launch_lds(P.n, p, (int)geo.grid, s) : launch_walk(P.kind, P.n, p, (int)geo.grid, s));
  }
  SUP_HIP(hipEventRecord(ev.second, s));
  if (defer) c->tally.commit();
  if ((rc = queue_result_copies(c, rp, count, head, slot))) return rc;
  unsigned long long* esum = reinterpret_cast<unsigned long long*>(c->h_result + 3);  // (beside the visited sum)
  if (ends) {
    SUP_HIP(launch_sum_visited(end_words, kChunkEndWords, reinterpret_cast<unsigned long long*>(c->d_result + 3), s));
    SUP_HIP(hipMemcpyAsync(esum, c->d_result + 3, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  }

  // spin on the flag only where the walk is predicted to end within the spin
  // window (cost model on this device's CUs; a longer walk blocks in the
  // stream sync at once instead of holding a host core for 2 ms)
  const double predicted_ms = walk_seconds(P, std::ldexp((double)count, P.lay.L + P.lay.m)) * 1e3 *
                              (256.0 / std::max(1, c->cus));
  const bool seen = rp.flagged && predicted_ms <= kFlagSpinMs &&
                    (p.fold_sys ? wait_result(c->h_result) : wait_flag(c->h_flag, rp.seq));
  if (!seen || ends) SUP_HIP(hipStreamSynchronize(s));  // (the ended chunks' count follows the result)
  if (fused) {  // the final fold zeroed the other head
    c->head_zero[qh ^ 1] = true;
    c->head = qh ^ 1;
    if (std::getenv("SUP_FOLD_CHECK") && (rc = fold_check(c, P, count, geo))) return rc;
  } else {
    c->head_zero[0] = count > 1;  // the reduction's first pass zeroed it (one chunk: a copy, no pass)
  }

  float ms = 0.f;
  if ((rc = walk_time(c, defer, ev, &ms))) return rc;
  r.partial = *c->h_result;
  r.kernel_ms = ms;
  r.grid = (int)geo.grid;
  if (p.trace && (rc = trace_write(trace_path, p.trace, count, geo, resident * wpb, ms))) return rc;
  const unsigned long long* vsum = reinterpret_cast<const unsigned long long*>(c->h_result + 2);
  r.visited = visited ? (uint64_t)*vsum * (uint64_t)(1ull << P.lay.L)
                      : (count - (ends ? (uint64_t)*esum : 0)) << (P.lay.L + P.lay.m);
  return SUP_OK;
}

// Several leaves (the -o / -u reduction's permanents) in one launch: plans of
// one order, walk kind (plain or prefix-blocked) and layout.  Their tables are
// packed into one device buffer, the batch kernel walks the K 2^h wave-chunks
// as one queue (walk_batch.hpp), and each leaf's partials are folded by the
// one-leaf pairwise tree: partial[i] is bit-identical to run_range over plan
// i's whole range (tests/test_gpu_reduce_workers.py).  One launch instead of
// K removes K - 1 launch tails, syncs and result copies.
bool batchable(const Plan& a, const Plan& b) {
  return (a.kind == kWalkDense || a.kind == kWalkSparse) && a.kind == b.kind && !a.lds && !b.lds && a.n == b.n &&
         a.lay.L == b.lay.L && a.lay.m == b.lay.m && a.lay.h == b.lay.h && a.cols.size() == b.cols.size() &&
         a.x0.size() == b.x0.size() && a.lay.chunks() >= 1 &&
         a.lay.chunks() <= (1ull << kMaxBatchLeafChunkBits);  // 32-bit chunk ids (engine.hpp)
}

int run_range_batch(int dev, const std::vector<const Plan*>& plans, std::vector<double>& partial, double* kernel_ms) {
  const size_t K = plans.size();
  partial.assign(K, 0.0);
  if (kernel_ms) *kernel_ms = 0.0;
  if (K == 0) return SUP_OK;
  if (K > (size_t)kMaxBatchLeaves) {
    set_error("leaf batch larger than kMaxBatchLeaves");
    return SUP_EINVAL;
  }
  const Plan& P0 = *plans[0];
  for (const Plan* q : plans)
    if (!batchable(P0, *q)) {
      set_error("leaf batch: plans of different order, walk or layout");
      return SUP_EINVAL;
    }
  CtxGuard guard;
  int rc = guard.open(dev, "device buffers");
  if (rc) return rc;
  DeviceCtx* c = guard.c;
  const uint64_t C = P0.lay.chunks(), count = C * K;
  const size_t colsz = P0.cols.size(), stride = colsz + P0.x0.size();
  if ((rc = ensure(c->d_batch, c->batch_cap, K * stride))) return rc;
  if ((rc = ensure(c->d_desc, c->desc_cap, K))) return rc;
  if ((rc = ensure(c->d_chunk, c->chunk_cap, (size_t)count))) return rc;
  if ((rc = ensure(c->d_scratch, c->scratch_cap, (size_t)(K * pairwise_scratch_size(C))))) return rc;
  if ((rc = ensure(c->d_bres, c->bres_cap, K))) return rc;
  if (!c->h_bres) SUP_HIP(hipHostMalloc(&c->h_bres, kMaxBatchLeaves * sizeof(double), hipHostMallocDefault));
  std::vector<double> tab(K * stride);
  std::vector<LeafDesc> desc(K);
  for (size_t i = 0; i < K; ++i) {
    const Plan& P = *plans[i];
    std::copy(P.cols.begin(), P.cols.end(), tab.begin() + i * stride);
    std::copy(P.x0.begin(), P.x0.end(), tab.begin() + i * stride + colsz);
    desc[i].cols = c->d_batch + i * stride;
    desc[i].x0 = c->d_batch + i * stride + colsz;
    desc[i].ends = P.kind == kWalkSparse ? P.chunk_ends : 0;
    if (P.kind == kWalkSparse) pack_nblk(P, &desc[i].nb_lo, &desc[i].nb_hi);
  }
  hipStream_t s = c->stream;
  SUP_HIP(hipMemcpyAsync(c->d_batch, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, s));
  SUP_HIP(hipMemcpyAsync(c->d_desc, desc.data(), K * sizeof(LeafDesc), hipMemcpyHostToDevice, s));
  SUP_HIP(hipMemsetAsync(c->d_counter, 0, sizeof(unsigned), s));
  c->head_zero[0] = false;  // this walk leaves queue head 0 nonzero
  int& occ = c->occ_batch[P0.kind == kWalkSparse][P0.n];
  if (occ == 0) {
    int b = 0;
    SUP_HIP(walk_batch_occupancy(P0.kind, P0.n, &b));
    occ = b > 0 ? b : 1;
  }
  // groups as run_range picks them, and never larger than one leaf's chunks
  const LaunchGeom geo = walk_geometry(count, (uint64_t)c->cus * (uint64_t)occ, kWavesPerBlock, false, 0, -1, C);
  WalkParams p = walk_params(P0, desc[0].cols, desc[0].x0, 0, count, c->d_counter, geo.group, false);
  p.chunk_out = c->d_chunk;
  p.tail_ticket = geo.tail_ticket;
  LeafBatch lb{c->d_desc, (unsigned)P0.lay.h, 0};
  SUP_HIP(hipEventRecord(c->ev0, s));
  SUP_ON_DEVICE(c->dev, "batch walk launch");
  SUP_HIP(launch_walk_batch(P0.kind, P0.n, p, lb, (int)geo.grid, s));
  SUP_HIP(hipEventRecord(c->ev1, s));
  SUP_HIP(launch_pairwise_reduce_seg(c->d_chunk, C, K, c->d_scratch, c->d_bres, s));
  SUP_HIP(hipMemcpyAsync(c->h_bres, c->d_bres, K * sizeof(double), hipMemcpyDeviceToHost, s));
  if ((rc = timed_sync(c, kernel_ms))) return rc;
  for (size_t i = 0; i < K; ++i) partial[i] = c->h_bres[i];
  return SUP_OK;
}

// Exact residue walk (walk_exact.hip) over wave-chunks [c0, c1) of a dense
// identity-map plan of 2A: per prime, the sum of the terms mod p (in [0, p)).
// Residue sums are exact, so neither the wave a chunk lands on nor the order
// of the per-wave sums changes the result.
int run_range_exact(int dev, const Plan& P, int group, uint64_t c0, uint64_t c1, const std::vector<double>& primes,
                    std::vector<uint64_t>& res, double* kernel_ms) {
  const int np = (int)primes.size();
  res.assign(np, 0);
  if (kernel_ms) *kernel_ms = 0.0;
  if (c1 <= c0) return SUP_OK;
  // group 1, 2, 4: the dense kernel on a dense plan; 8 + g: the prefix-blocked
  // kernel on a prefix-blocked plan (walk_exact.hip)
  const bool blocked = (group & 8) != 0;
  if (np < 1 || np > kMaxPrimes || P.kind != (blocked ? kWalkSparse : kWalkDense) || c1 > P.lay.chunks()) {
    set_error("run_range_exact: bad request");
    return SUP_EINVAL;
  }
  CtxGuard guard;
  int rc = guard.open(dev, "device buffers");
  if (rc) return rc;
  DeviceCtx* c = guard.c;
  int occ = 0;
  SUP_HIP(exact_occupancy(P.n, group, &occ));
  const uint64_t count = c1 - c0;
  const uint64_t grid = capped_grid(c, occ, count);
  const size_t waves = (size_t)grid * kWavesPerBlock;
  if ((rc = ensure(c->d_cols, c->cols_cap, P.cols.size()))) return rc;
  if ((rc = ensure(c->d_wave, c->wave_cap, waves * kMaxPrimes))) return rc;
  hipStream_t s = c->stream;
  if ((rc = upload_walk_tables(c, P, c->d_x0, P.x0))) return rc;
  WalkParams p = walk_params(P, c->d_cols, c->d_x0, c0, count, c->d_counter, 1, blocked);  // walk_exact_blocked: nblk
  p.umask = P.chunk_ends;  // walk_exact: its chunk-end rows (walk_sparse.hip's check)
  ExactParams e{};
  for (int q = 0; q < np; ++q) e.prime[q] = primes[q], e.pinv[q] = 1.0 / primes[q];
  e.nprimes = np;
  e.wave_out = c->d_wave;
  SUP_HIP(hipEventRecord(c->ev0, s));
  SUP_ON_DEVICE(c->dev, "exact walk launch");
  SUP_HIP(launch_exact(P.n, group, p, e, (int)grid, s));
  SUP_HIP(hipEventRecord(c->ev1, s));
  std::vector<double> w(waves * kMaxPrimes);
  SUP_HIP(hipMemcpyAsync(w.data(), c->d_wave, w.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  if ((rc = timed_sync(c, kernel_ms))) return rc;
  for (int q = 0; q < np; ++q) {
    const uint64_t pq = (uint64_t)primes[q];
    uint64_t acc = 0;  // waves x p < 2^64
    for (size_t i = 0; i < waves; ++i) acc = (acc + (uint64_t)w[i * kMaxPrimes + q]) % pq;
    res[q] = acc;
  }
  return SUP_OK;
}

int run_range_dd(int dev, const Plan& P, const std::vector<double>& x0dd, uint64_t c0, uint64_t c1,
                 double* parts, double* kernel_ms) {
  if (kernel_ms) *kernel_ms = 0.0;
  if (c1 <= c0) return SUP_OK;
  const bool blocked = P.kind == kWalkSparse;  // walk_dd_blocked; else the dense walk_dd
  if ((P.kind != kWalkDense && !blocked) || c1 > P.lay.chunks() || x0dd.size() != 2 * (size_t)P.NP) {
    set_error("run_range_dd: bad request");
    return SUP_EINVAL;
  }
  CtxGuard guard;
  int rc = guard.open(dev, "device buffers");
  if (rc) return rc;
  DeviceCtx* c = guard.c;
  int occ = 0;
  SUP_HIP(blocked ? dd_blocked_occupancy(P.n, &occ) : dd_occupancy(P.n, &occ));
  const uint64_t count = c1 - c0;
  const uint64_t grid = capped_grid(c, occ, count);
  if ((rc = ensure(c->d_cols, c->cols_cap, P.cols.size()))) return rc;
  if ((rc = ensure(c->d_x0dd, c->x0dd_cap, x0dd.size()))) return rc;
  if ((rc = ensure(c->d_chunk, c->chunk_cap, (size_t)(2 * count)))) return rc;
  hipStream_t s = c->stream;
  if ((rc = upload_walk_tables(c, P, c->d_x0dd, x0dd))) return rc;
  WalkParams p = walk_params(P, c->d_cols, c->d_x0dd, c0, count, c->d_counter, 1, blocked);  // walk_dd_blocked: nblk
  p.umask = P.chunk_ends;  // walk_dd: its chunk-end rows
  p.chunk_out = c->d_chunk;
  SUP_HIP(hipEventRecord(c->ev0, s));
  SUP_ON_DEVICE(c->dev, "double-double walk launch");
  SUP_HIP(blocked ? launch_dd_blocked(P.n, p, (int)grid, s) : launch_dd(P.n, p, (int)grid, s));
  SUP_HIP(hipEventRecord(c->ev1, s));
  SUP_HIP(hipMemcpyAsync(parts, c->d_chunk, 2 * count * sizeof(double), hipMemcpyDeviceToHost, s));
  return timed_sync(c, kernel_ms);
}

// Complex fp64 walk (walk_cplx.hip) over wave-chunks [c0, c1) of a dense
// identity plan whose column table holds the Re plane, then the Im plane.
// The start vector (re block, im block) shares the double-double walk's
// two-block buffer.
int run_range_cplx(int dev, const Plan& P, const std::vector<double>& x0c, uint64_t c0, uint64_t c1, double* parts,
                   double* kernel_ms, int* grid_out) {
  if (kernel_ms) *kernel_ms = 0.0;
  if (grid_out) *grid_out = 0;
  if (c1 <= c0) return SUP_OK;
  const size_t plane = (size_t)2 * std::max(P.n - 1, 1) * P.NP;
  if (P.kind != kWalkDense || c1 > P.lay.chunks() || x0c.size() != 2 * (size_t)P.NP || P.cols.size() != 2 * plane) {
    set_error("run_range_cplx: bad request");
    return SUP_EINVAL;
  }
  CtxGuard guard;
  int rc = guard.open(dev, "device buffers");
  if (rc) return rc;
  DeviceCtx* c = guard.c;
  int occ = 0;
  SUP_HIP(cplx_occupancy(P.n, &occ));
  const uint64_t count = c1 - c0;
  const uint64_t grid = capped_grid(c, occ, count);
  if ((rc = ensure(c->d_cols, c->cols_cap, P.cols.size()))) return rc;
  if ((rc = ensure(c->d_x0dd, c->x0dd_cap, x0c.size()))) return rc;
  if ((rc = ensure(c->d_chunk, c->chunk_cap, (size_t)(2 * count)))) return rc;
  hipStream_t s = c->stream;
  if ((rc = upload_walk_tables(c, P, c->d_x0dd, x0c))) return rc;
  WalkParams p = walk_params(P, c->d_cols, c->d_x0dd, c0, count, c->d_counter, 1, false);
  p.chunk_out = c->d_chunk;
  SUP_HIP(hipEventRecord(c->ev0, s));
  SUP_ON_DEVICE(c->dev, "complex walk launch");
  SUP_HIP(launch_cplx(P.n, p, (int)grid, s));
  SUP_HIP(hipEventRecord(c->ev1, s));
  SUP_HIP(hipMemcpyAsync(parts, c->d_chunk, 2 * count * sizeof(double), hipMemcpyDeviceToHost, s));
  if (grid_out) *grid_out = (int)grid;
  return timed_sync(c, kernel_ms);
}

// Complex double-double walk (walk_cplxdd.hip) over wave-chunks [c0, c1) of
// the same kind of plan (run_range_cplx's), n <= SUP_CPLX_QUAD_MAX_DEVICE_N.
// The start vector is four blocks (re.hi, re.lo, im.hi, im.lo) in the
// two-block walks' buffer; a wave-chunk's partial is four doubles.
int run_range_cplxdd(int dev, const Plan& P, const std::vector<double>& x0q, uint64_t c0, uint64_t c1, double* parts,
                     double* kernel_ms, int* grid_out) {
  if (kernel_ms) *kernel_ms = 0.0;
  if (grid_out) *grid_out = 0;
  if (c1 <= c0) return SUP_OK;
  const size_t plane = (size_t)2 * std::max(P.n - 1, 1) * P.NP;
  if (P.kind != kWalkDense || P.n < 1 || P.n > SUP_CPLX_QUAD_MAX_DEVICE_N || c1 > P.lay.chunks() ||
      x0q.size() != 4 * (size_t)P.NP || P.cols.size() != 2 * plane) {
    set_error("run_range_cplxdd: bad request");
    return SUP_EINVAL;
  }
  CtxGuard guard;
  int rc = guard.open(dev, "device buffers");
  if (rc) return rc;
  DeviceCtx* c = guard.c;
  int occ = 0;
  SUP_HIP(cplxdd_occupancy(P.n, &occ));
  const uint64_t count = c1 - c0;
  const uint64_t grid = capped_grid(c, occ, count);
  if ((rc = ensure(c->d_cols, c->cols_cap, P.cols.size()))) return rc;
  if ((rc = ensure(c->d_x0dd, c->x0dd_cap, x0q.size()))) return rc;
  if ((rc = ensure(c->d_chunk, c->chunk_cap, (size_t)(4 * count)))) return rc;
  hipStream_t s = c->stream;
  if ((rc = upload_walk_tables(c, P, c->d_x0dd, x0q))) return rc;
  WalkParams p = walk_params(P, c->d_cols, c->d_x0dd, c0, count, c->d_counter, 1, false);
  p.chunk_out = c->d_chunk;
  SUP_HIP(hipEventRecord(c->ev0, s));
  SUP_ON_DEVICE(c->dev, "complex double-double walk launch");
  SUP_HIP(launch_cplxdd(P.n, p, (int)grid, s));
  SUP_HIP(hipEventRecord(c->ev1, s));
  SUP_HIP(hipMemcpyAsync(parts, c->d_chunk, 4 * count * sizeof(double), hipMemcpyDeviceToHost, s));
  if (grid_out) *grid_out = (int)grid;
  return timed_sync(c, kernel_ms);
}

// Exact complex residue walk (walk_cplxexact.hip) over wave-chunks [c0, c1) of
// a complex plan of the doubled matrix (run_range_cplx's tables and start
// vector): per prime and part, the sum of the terms mod p in [0, p).  Residue
// sums are exact, so neither the wave a chunk lands on nor the order of the
// per-wave sums changes the result.  The kernel takes its primes in pairs: an
// odd count is padded with a repeat of the last prime, whose result is dropped.
int run_range_cplxexact(int dev, const Plan& P, const std::vector<double>& x0c, int group, uint64_t c0, uint64_t c1,
                        const std::vector<double>& primes, std::vector<uint64_t>& res_re,
                        std::vector<uint64_t>& res_im, double* kernel_ms, int* grid_out) {
  const int np = (int)primes.size();
  res_re.assign(np, 0);
  res_im.assign(np, 0);
  if (kernel_ms) *kernel_ms = 0.0;
  if (grid_out) *grid_out = 0;
  if (c1 <= c0) return SUP_OK;
  const size_t plane = (size_t)2 * std::max(P.n - 1, 1) * P.NP;
  if (np < 1 || np > kMaxCxPrimes || (group != 1 && group != 2) || P.kind != kWalkDense || P.n < 1 ||
      P.n > SUP_CPLX_EXACT_MAX_DEVICE_N || c1 > P.lay.chunks() || x0c.size() != 2 * (size_t)P.NP ||
      P.cols.size() != 2 * plane) {
    set_error("run_range_cplxexact: bad request");
    return SUP_EINVAL;
  }
  CtxGuard guard;
  int rc = guard.open(dev, "device buffers");
  if (rc) return rc;
  DeviceCtx* c = guard.c;
  int occ = 0;
  SUP_HIP(cplxexact_occupancy(P.n, group, &occ));
  const uint64_t count = c1 - c0;
  const uint64_t grid = capped_grid(c, occ, count);
  const size_t waves = (size_t)grid * kWavesPerBlock, per_wave = (size_t)2 * kMaxCxPrimes;
  if ((rc = ensure(c->d_cols, c->cols_cap, P.cols.size()))) return rc;
  if ((rc = ensure(c->d_x0dd, c->x0dd_cap, x0c.size()))) return rc;
  if ((rc = ensure(c->d_wave, c->wave_cap, waves * per_wave))) return rc;
  hipStream_t s = c->stream;
  if ((rc = upload_walk_tables(c, P, c->d_x0dd, x0c))) return rc;
  WalkParams p = walk_params(P, c->d_cols, c->d_x0dd, c0, count, c->d_counter, 1, false);
  CxExactParams e{};
  const int npad = (np + 1) & ~1;
  for (int q = 0; q < npad; ++q) e.prime[q] = primes[std::min(q, np - 1)], e.pinv[q] = 1.0 / e.prime[q];
  e.nprimes = npad;
  e.wave_out = c->d_wave;
  SUP_HIP(hipEventRecord(c->ev0, s));
  SUP_ON_DEVICE(c->dev, "exact complex walk launch");
  SUP_HIP(launch_cplxexact(P.n, group, p, e, (int)grid, s));
  SUP_HIP(hipEventRecord(c->ev1, s));
  std::vector<double> w(waves * per_wave);
  SUP_HIP(hipMemcpyAsync(w.data(), c->d_wave, w.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  if (grid_out) *grid_out = (int)grid;
  if ((rc = timed_sync(c, kernel_ms))) return rc;
  for (int q = 0; q < np; ++q) {
    const uint64_t pq = (uint64_t)primes[q];
    uint64_t are = 0, aim = 0;  // waves x p < 2^64
    for (size_t i = 0; i < waves; ++i) {
      are = (are + (uint64_t)w[(i * kMaxCxPrimes + q) * 2]) % pq;
      aim = (aim + (uint64_t)w[(i * kMaxCxPrimes + q) * 2 + 1]) % pq;
    }
    res_re[q] = are, res_im[q] = aim;
  }
  return SUP_OK;
}

// Batched complex walk (walk_cplxb.hip, cplx_batch.hip) of matrices [k0, k1)
// of `in` (order n <= 32, layout lay) on device `dev`, in slabs of K matrices:
// per slab one upload of its raw matrices (or its index lists; U goes up once
// per call), then prepare, walk and fold on the context's stream with no host
// work between them, and one download of 16 K bytes into out[2 (k - k0)].
// K: as many matrices as keep a slab's tables, partials and input under
// kCplxBatchCapBytes (at least one), or SUP_CPLX_BATCH_SLAB.
static constexpr size_t kCplxBatchCapBytes = (size_t)256 << 20;
int run_cplx_batch(int dev, int n, const Layout& lay, const CplxBatchIn& in, uint64_t k0, uint64_t k1, double* out,
                   double* kernel_ms, int* grid_out) {
  if (kernel_ms) *kernel_ms = 0.0;
  if (grid_out) *grid_out = 0;
  if (k1 <= k0) return SUP_OK;
  if (n < 1 || n > 32 || lay.L + lay.m + lay.h != n - 1 || lay.h > 24 || (!in.mats && !(in.U && in.rows && in.cols))) {
    set_error("run_cplx_batch: bad request");
    return SUP_EINVAL;
  }
  const bool sub = in.U != nullptr;
  const size_t NP = (size_t)pad8(n), plane = (size_t)2 * std::max(n - 1, 1) * NP, nn = (size_t)n * n;
  const size_t tab = 2 * plane, per_chunks = (size_t)1 << lay.h;
  const size_t per_bytes = (tab + 2 * NP + 2 * per_chunks + 2 + (sub ? (size_t)n : 2 * nn)) * sizeof(double);
  uint64_t K = std::max<uint64_t>(1, kCplxBatchCapBytes / per_bytes);
  if (const char* e = std::getenv("SUP_CPLX_BATCH_SLAB")) {
    const long long v = std::atoll(e);
    if (v > 0) K = (uint64_t)v;
  }
  K = std::min({K, k1 - k0, (uint64_t)0x7fffffffu >> lay.h});  // 32-bit queue tickets
  CtxGuard guard;
  int rc = guard.open(dev, "device buffers");
  if (rc) return rc;
  DeviceCtx* c = guard.c;
  int occ = 0;
  SUP_HIP(cplx_batch_occupancy(n, &occ));
  if ((rc = ensure(c->d_cbtab, c->cbtab_cap, (size_t)K * (tab + 2 * NP)))) return rc;
  if ((rc = ensure(c->d_chunk, c->chunk_cap, (size_t)K * 2 * per_chunks))) return rc;
  if ((rc = ensure(c->d_cbout, c->cbout_cap, (size_t)K * 2))) return rc;
  if (sub) {
    if ((rc = ensure(c->d_cbidx, c->cbidx_cap, (size_t)K * 2 * n))) return rc;
    if ((rc = ensure(c->d_cbU, c->cbU_cap, (size_t)2 * in.R * in.C))) return rc;
  } else if ((rc = ensure(c->d_cbmat, c->cbmat_cap, (size_t)K * 2 * nn))) {
    return rc;
  }
  hipStream_t s = c->stream;
  c->tables_uid = 0;  // the walk leaves head 0 nonzero
  c->head_zero[0] = false;
  if (sub)
    SUP_HIP(hipMemcpyAsync(c->d_cbU, in.U, (size_t)2 * in.R * in.C * sizeof(double), hipMemcpyHostToDevice, s));
  double* d_tabs = c->d_cbtab;
  double* d_x0s = c->d_cbtab + (size_t)K * tab;
  const uint64_t resident = (uint64_t)c->cus * (uint64_t)std::max(occ, 1);
  double total_ms = 0.0;
  for (uint64_t a = k0; a < k1; a += K) {
    const uint64_t kk = std::min(K, k1 - a);
    CplxBatchSrc src{};
    if (sub) {
      int32_t* d_rows = c->d_cbidx;
      int32_t* d_cols = c->d_cbidx + (size_t)K * n;
      SUP_HIP(hipMemcpyAsync(d_rows, in.rows + a * n, (size_t)kk * n * sizeof(int32_t), hipMemcpyHostToDevice, s));
      SUP_HIP(hipMemcpyAsync(d_cols, in.cols + a * n, (size_t)kk * n * sizeof(int32_t), hipMemcpyHostToDevice, s));
      src.U = c->d_cbU, src.rows = d_rows, src.cols = d_cols, src.C = in.C;
    } else {
      SUP_HIP(hipMemcpyAsync(c->d_cbmat, in.mats + a * 2 * nn, (size_t)kk * 2 * nn * sizeof(double),
                             hipMemcpyHostToDevice, s));
      src.mats = c->d_cbmat;
    }
    SUP_HIP(hipMemsetAsync(c->d_counter, 0, sizeof(unsigned), s));
    const uint64_t chunks = kk << lay.h;
    const LaunchGeom geo = walk_geometry(chunks, resident, kWavesPerBlock, false);
    WalkParams p{};
    p.cols = d_tabs;
    p.x0 = d_x0s;
    p.chunk_begin = 0;
    p.chunk_count = chunks;
    p.L = lay.L;
    p.m = lay.m;
    p.n = n;
    p.counter = c->d_counter;
    p.group = geo.group;
    p.chunk_out = c->d_chunk;
    SUP_HIP(hipEventRecord(c->ev0, s));
    SUP_ON_DEVICE(c->dev, "batched complex walk launch");
    SUP_HIP(launch_cplx_batch_prepare(src, n, kk, d_tabs, d_x0s, s));
    SUP_HIP(launch_cplx_batch(n, p, lay.h, (int)geo.grid, s));
    SUP_HIP(launch_cplx_batch_fold(c->d_chunk, n, lay.h, kk, c->d_cbout, s));
    SUP_HIP(hipEventRecord(c->ev1, s));
    SUP_HIP(hipMemcpyAsync(out + 2 * (a - k0), c->d_cbout, (size_t)kk * 2 * sizeof(double), hipMemcpyDeviceToHost, s));
    double ms = 0.0;
    if ((rc = timed_sync(c, &ms))) return rc;
    total_ms += ms;
    if (grid_out) *grid_out = (int)geo.grid;
  }
  if (kernel_ms) *kernel_ms = total_ms;
  return SUP_OK;
}

// One-walk minors (walk_cplxm.hip, cplx_minors.hip) of matrices [k0, k1) of
// `in` (n rows, n - 1 columns, 2 <= n <= 32; lay: the layout of order n - 1)
// on device `dev`, in slabs of K matrices as run_cplx_batch's: U goes up once
// per call, per slab its index lists, then prepare, walk and fold
// (cplx_batch_fold over K n outputs of order n - 1) on the context's stream and
// one download of 16 K n bytes into out[2 (k - k0) n].  c0 < c1 (one matrix,
// k1 = k0 + 1): the range form, no fold, the partials [j][c - c0] come down.
// The buffers are the batched walk's (same context lock).
static int run_cplx_minors_impl(int dev, int n, const Layout& lay, const CplxBatchIn& in, uint64_t k0, uint64_t k1,
                                uint64_t c0, uint64_t c1, double* out, double* kernel_ms, int* grid_out) {
  if (kernel_ms) *kernel_ms = 0.0;
  if (grid_out) *grid_out = 0;
  if (k1 <= k0) return SUP_OK;
  const bool range = c1 > c0;
  const int q = n - 1;
  if (n < 2 || n > 32 || lay.L + lay.m + lay.h != q - 1 || lay.h > 24 || !(in.U && in.rows && in.cols) || !out ||
      (range && (k1 != k0 + 1 || c1 > lay.chunks()))) {
    set_error("run_cplx_minors: bad request");
    return SUP_EINVAL;
  }
  const size_t NP = (size_t)pad8(n), plane = (size_t)2 * std::max(q - 1, 1) * NP;
  const size_t tab = 2 * plane, per_chunks = range ? (size_t)(c1 - c0) : (size_t)1 << lay.h;
  const size_t per_bytes = (tab + 2 * NP + (2 * per_chunks + 2) * n + (size_t)n) * sizeof(double);
  uint64_t K = std::max<uint64_t>(1, kCplxBatchCapBytes / per_bytes);
  if (const char* e = std::getenv("SUP_CPLX_MINORS_SLAB")) {
    const long long v = std::atoll(e);
    if (v > 0) K = (uint64_t)v;
  }
  K = std::min({K, k1 - k0, (uint64_t)0x7fffffffu >> lay.h});  // 32-bit queue tickets
  CtxGuard guard;
  int rc = guard.open(dev, "device buffers");
  if (rc) return rc;
  DeviceCtx* c = guard.c;
  int occ = 0;
  SUP_HIP(cplx_minors_occupancy(n, &occ));
  if ((rc = ensure(c->d_cbtab, c->cbtab_cap, (size_t)K * (tab + 2 * NP)))) return rc;
  if ((rc = ensure(c->d_chunk, c->chunk_cap, (size_t)K * 2 * per_chunks * n))) return rc;
  if ((rc = ensure(c->d_cbout, c->cbout_cap, (size_t)K * 2 * n))) return rc;
  if ((rc = ensure(c->d_cbidx, c->cbidx_cap, (size_t)K * 2 * n))) return rc;
  if ((rc = ensure(c->d_cbU, c->cbU_cap, (size_t)2 * in.R * in.C))) return rc;
  hipStream_t s = c->stream;
  c->tables_uid = 0;  // the walk leaves head 0 nonzero
  c->head_zero[0] = false;
  SUP_HIP(hipMemcpyAsync(c->d_cbU, in.U, (size_t)2 * in.R * in.C * sizeof(double), hipMemcpyHostToDevice, s));
  double* d_tabs = c->d_cbtab;
  double* d_x0s = c->d_cbtab + (size_t)K * tab;
  const uint64_t resident = (uint64_t)c->cus * (uint64_t)std::max(occ, 1);
  const char* fg = std::getenv("SUP_WALK_GROUP");  // tests, read per call: chunks per ticket (the bits do not change)
  double total_ms = 0.0;
  for (uint64_t a = k0; a < k1; a += K) {
    const uint64_t kk = std::min(K, k1 - a);
    int32_t* d_rows = c->d_cbidx;
    int32_t* d_cols = c->d_cbidx + (size_t)K * n;
    SUP_HIP(hipMemcpyAsync(d_rows, in.rows + a * n, (size_t)kk * n * sizeof(int32_t), hipMemcpyHostToDevice, s));
    SUP_HIP(hipMemcpyAsync(d_cols, in.cols + a * q, (size_t)kk * q * sizeof(int32_t), hipMemcpyHostToDevice, s));
    CplxBatchSrc src{};
    src.U = c->d_cbU, src.rows = d_rows, src.cols = d_cols, src.C = in.C;
    SUP_HIP(hipMemsetAsync(c->d_counter, 0, sizeof(unsigned), s));
    const uint64_t chunks = range ? c1 - c0 : kk << lay.h;
    const LaunchGeom geo =
        walk_geometry(chunks, resident, kWavesPerBlock, false, fg ? std::max(1, std::atoi(fg)) : 0);
    WalkParams p{};
    p.cols = d_tabs;
    p.x0 = d_x0s;
    p.chunk_begin = range ? c0 : 0;
    p.chunk_count = chunks;
    p.L = lay.L;
    p.m = lay.m;
    p.n = n;
    p.counter = c->d_counter;
    p.group = geo.group;
    p.chunk_out = c->d_chunk;
    SUP_HIP(hipEventRecord(c->ev0, s));
    SUP_ON_DEVICE(c->dev, "minors walk launch");
    SUP_HIP(launch_cplx_minors_prepare(src, n, kk, d_tabs, d_x0s, s));
    SUP_HIP(launch_cplx_minors(n, p, lay.h, (unsigned long long)per_chunks, (int)geo.grid, s));
    if (!range) SUP_HIP(launch_cplx_batch_fold(c->d_chunk, q, lay.h, kk * (uint64_t)n, c->d_cbout, s));
    SUP_HIP(hipEventRecord(c->ev1, s));
    if (range)
      SUP_HIP(hipMemcpyAsync(out, c->d_chunk, (size_t)2 * per_chunks * n * sizeof(double), hipMemcpyDeviceToHost, s));
    else
      SUP_HIP(hipMemcpyAsync(out + 2 * (a - k0) * n, c->d_cbout, (size_t)kk * 2 * n * sizeof(double),
                             hipMemcpyDeviceToHost, s));
    double ms = 0.0;
    if ((rc = timed_sync(c, &ms))) return rc;
    total_ms += ms;
    if (grid_out) *grid_out = (int)geo.grid;
  }
  if (kernel_ms) *kernel_ms = total_ms;
  return SUP_OK;
}

int run_cplx_minors(int dev, int n, const Layout& lay, const CplxBatchIn& in, uint64_t k0, uint64_t k1, double* out,
                    double* kernel_ms, int* grid_out) {
  return run_cplx_minors_impl(dev, n, lay, in, k0, k1, 0, 0, out, kernel_ms, grid_out);
}

int run_cplx_minors_range(int dev, int n, const Layout& lay, const CplxBatchIn& in, uint64_t c0, uint64_t c1,
                          double* parts, double* kernel_ms, int* grid_out) {
  if (c1 <= c0) {
    if (kernel_ms) *kernel_ms = 0.0;
    if (grid_out) *grid_out = 0;
    return SUP_OK;
  }
  return run_cplx_minors_impl(dev, n, lay, in, 0, 1, c0, c1, parts, kernel_ms, grid_out);
}

// Collision-aware complex walk (walk_cplxf.hip, cplx_fock.hip) of slab S on
// device `dev`: U, the slab's index lists and its descriptor pools go up, then
// prepare (tables and x(0) written on the device), the walk over the slab's
// queue and the per-matrix fold run on the context's stream with no host work
// between them, and one download brings 16 bytes per matrix into out.
// minors: the slab of the collision-aware one-walk minors (walk_cplxfm.hip):
// tables of S.n rows from the row lists alone (the column groups are in
// S.grp), S.n partials per wave-chunk and S.n outputs per matrix.
static int run_cplx_fock_impl(int dev, const FockSlab& S, const CplxBatchIn& in, bool minors, double* out,
                              double* kernel_ms, int* grid_out) {
  if (kernel_ms) *kernel_ms = 0.0;
  if (grid_out) *grid_out = 0;
  const uint64_t K = S.mats.size(), chunks = S.chunks.size();
  if (K == 0) return SUP_OK;
  const uint64_t outs = minors ? (uint64_t)S.n : 1;  // partials per chunk, results per matrix
  if (S.n < (minors ? 2 : 1) || S.n > (minors ? 32 : SUP_MAX_N) || chunks == 0 || chunks * outs > 0x7fffffffull || !out ||
      !in.U || !in.rows || (!minors && !in.cols) || in.R < 1 || in.C < 1) {
    set_error("run_cplx_fock: bad request");
    return SUP_EINVAL;
  }
  const std::vector<double>& wts = fock_weights();
  // the packed pools, each starting on a 16-byte unit
  auto units = [](size_t bytes) { return (bytes + 15) / 16; };
  const size_t u_prog = 0, u_dig = u_prog + units(S.prog.size() * sizeof(FockStep));
  const size_t u_mats = u_dig + units(S.dig.size() * sizeof(FockDigit));
  const size_t u_chunks = u_mats + units(K * sizeof(FockMat));
  const size_t u_wts = u_chunks + units(chunks * sizeof(FockChunk));
  const size_t u_grp = u_wts + units(wts.size() * sizeof(double));
  const size_t u_end = u_grp + units(S.grp.size() * sizeof(int32_t));
  const size_t n = (size_t)S.n;
  CtxGuard guard;
  int rc = guard.open(dev, "device buffers");
  if (rc) return rc;
  DeviceCtx* c = guard.c;
  int occ = 0;
  SUP_HIP(minors ? cplx_fock_minors_occupancy(S.n, &occ) : cplx_fock_occupancy(S.n, &occ));
  if ((rc = ensure(c->d_cbtab, c->cbtab_cap, (size_t)(S.tab_doubles + S.x0_doubles)))) return rc;
  if ((rc = ensure(c->d_cbidx, c->cbidx_cap, (size_t)K * 2 * n))) return rc;
  if ((rc = ensure(c->d_cbU, c->cbU_cap, (size_t)2 * in.R * in.C))) return rc;
  if ((rc = ensure(c->d_chunk, c->chunk_cap, (size_t)(2 * chunks * outs)))) return rc;
  if ((rc = ensure(c->d_cbout, c->cbout_cap, (size_t)(K * outs * 2)))) return rc;
  if ((rc = ensure(c->d_fock, c->fock_cap, u_end))) return rc;
  hipStream_t s = c->stream;
  c->tables_uid = 0;  // the walk leaves head 0 nonzero
  c->head_zero[0] = false;
  double* d_tabs = c->d_cbtab;
  double* d_x0s = c->d_cbtab + S.tab_doubles;
  int32_t* d_rows = c->d_cbidx;
  // the minors' prepare has side 0 everywhere: it reads the row lists and S.grp, never the column lists
  int32_t* d_cols = minors ? d_rows : c->d_cbidx + (size_t)K * n;
  auto up = [&](void* dst, const void* src, size_t bytes) {
    return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s) : hipSuccess;
  };
  SUP_HIP(up(c->d_cbU, in.U, (size_t)2 * in.R * in.C * sizeof(double)));
  SUP_HIP(up(d_rows, in.rows + S.first * n, (size_t)K * n * sizeof(int32_t)));
  if (!minors) SUP_HIP(up(d_cols, in.cols + S.first * n, (size_t)K * n * sizeof(int32_t)));
  SUP_HIP(up(c->d_fock + u_grp, S.grp.data(), S.grp.size() * sizeof(int32_t)));
  SUP_HIP(up(c->d_fock + u_prog, S.prog.data(), S.prog.size() * sizeof(FockStep)));
  SUP_HIP(up(c->d_fock + u_dig, S.dig.data(), S.dig.size() * sizeof(FockDigit)));
  SUP_HIP(up(c->d_fock + u_mats, S.mats.data(), K * sizeof(FockMat)));
  SUP_HIP(up(c->d_fock + u_chunks, S.chunks.data(), chunks * sizeof(FockChunk)));
  SUP_HIP(up(c->d_fock + u_wts, wts.data(), wts.size() * sizeof(double)));
  SUP_HIP(hipMemsetAsync(c->d_counter, 0, sizeof(unsigned), s));
  const uint64_t resident = (uint64_t)c->cus * (uint64_t)std::max(occ, 1);
  const char* fg = std::getenv("SUP_WALK_GROUP");  // tests, read per call: chunks per ticket (the bits do not change)
  const LaunchGeom geo = walk_geometry(chunks, resident, kWavesPerBlock, false, fg ? std::max(1, std::atoi(fg)) : 0);
  FockParams p{};
  p.tabs = d_tabs;
  p.x0s = d_x0s;
  p.prog = reinterpret_cast<const FockStep*>(c->d_fock + u_prog);
  p.dig = reinterpret_cast<const FockDigit*>(c->d_fock + u_dig);
  p.mats = reinterpret_cast<const FockMat*>(c->d_fock + u_mats);
  p.chunks = reinterpret_cast<const FockChunk*>(c->d_fock + u_chunks);
  p.wts = reinterpret_cast<const double*>(c->d_fock + u_wts);
  p.chunk_count = chunks;
  p.chunk_out = c->d_chunk;
  p.counter = c->d_counter;
  p.group = geo.group;
  SUP_HIP(hipEventRecord(c->ev0, s));
  SUP_ON_DEVICE(c->dev, "collision-aware complex walk launch");
  SUP_HIP(launch_cplx_fock_prepare(c->d_cbU, in.C, d_rows, d_cols, reinterpret_cast<const int32_t*>(c->d_fock + u_grp),
                                   p.mats, S.n, K, d_tabs, d_x0s, s));
  if (minors) {
    SUP_HIP(launch_cplx_fock_minors(S.n, p, (int)geo.grid, s));
    SUP_HIP(launch_cplx_fock_minors_fold(c->d_chunk, p.mats, K, S.n, c->d_cbout, s));
  } else {
    SUP_HIP(launch_cplx_fock(S.n, p, (int)geo.grid, s));
    SUP_HIP(launch_cplx_fock_fold(c->d_chunk, p.mats, K, c->d_cbout, s));
  }
  SUP_HIP(hipEventRecord(c->ev1, s));
  SUP_HIP(hipMemcpyAsync(out, c->d_cbout, (size_t)(K * outs * 2) * sizeof(double), hipMemcpyDeviceToHost, s));
  if (grid_out) *grid_out = (int)geo.grid;
  return timed_sync(c, kernel_ms);
}

int run_cplx_fock(int dev, const FockSlab& S, const CplxBatchIn& in, double* out, double* kernel_ms, int* grid_out) {
  return run_cplx_fock_impl(dev, S, in, false, out, kernel_ms, grid_out);
}

// The collision-aware one-walk minors (walk_cplxfm.hip) of slab S: the same
// uploads, three launches and one download, 16 S.n bytes per matrix.
int run_cplx_fock_minors(int dev, const FockSlab& S, const CplxBatchIn& in, double* out, double* kernel_ms,
                         int* grid_out) {
  return run_cplx_fock_impl(dev, S, in, true, out, kernel_ms, grid_out);
}

// Hafnian walk (walk_haf.hip) of slab S on device `dev`, as run_cplx_fock's:
// A, mu and the slab's descriptor pools go up, then prepare (tables written on
// the device), the walk over the slab's queue and the per-matrix fold run on
// the context's stream with no host work between them, and one download
// brings 16 bytes per matrix into out.  The buffers are the collision-aware
// walk's (same context lock).  A ragged slab (S.each; walk_lhafe.hip) sends up
// the displacement rows it reads and one row number per matrix, and its walk
// and prepare kernels take the order, the coefficient row and the
// displacement per matrix.
int run_hafnian(int dev, const HafSlab& S, const HafIn& in, double* out, double* kernel_ms, int* grid_out) {
  if (kernel_ms) *kernel_ms = 0.0;
  if (grid_out) *grid_out = 0;
  const uint64_t K = S.mats.size(), chunks = S.chunks.size();
  if (K == 0) return SUP_OK;
  const bool shape_ok =
      S.each ? S.n == 0 && S.loop && S.mu_row.size() == K && S.mu_rows >= 1 && S.mu_lo >= 0 && !S.coef.empty()
             : S.n >= 1 && S.n <= SUP_MAX_N && (S.loop || !(S.n & 1)) && (!S.loop || S.coef.size() == (size_t)S.n / 2 + 1);
  if (!shape_ok || chunks == 0 || chunks > 0x7fffffffull || !out || !in.A || in.M < 1 || (S.loop && !in.mu)) {
    set_error("run_hafnian: bad request");
    return SUP_EINVAL;
  }
  const std::vector<double>& wts = fock_weights();
  // the packed pools, each starting on a 16-byte unit
  auto units = [](size_t bytes) { return (bytes + 15) / 16; };
  const size_t u_prog = 0, u_dig = u_prog + units(S.prog.size() * sizeof(HafStep));
  const size_t u_mats = u_dig + units(S.dig.size() * sizeof(HafDigit));
  const size_t u_chunks = u_mats + units(K * sizeof(HafMat));
  const size_t u_wts = u_chunks + units(chunks * sizeof(FockChunk));
  const size_t u_grp = u_wts + units(wts.size() * sizeof(double));
  const size_t u_coef = u_grp + units(S.grp.size() * sizeof(int32_t));
  const size_t u_murow = u_coef + units(S.coef.size() * sizeof(double));
  const size_t u_end = u_murow + units(S.mu_row.size() * sizeof(int32_t)) + 1;
  const size_t a_doubles = (size_t)2 * in.M * in.M;
  const size_t mu_doubles = S.each ? (size_t)2 * in.M * (size_t)S.mu_rows : S.loop ? (size_t)2 * in.M : 0;
  const double* mu_src = S.each ? in.mu + (size_t)2 * in.M * (size_t)S.mu_lo : in.mu;
  CtxGuard guard;
  int rc = guard.open(dev, "device buffers");
  if (rc) return rc;
  DeviceCtx* c = guard.c;
  int occ = 0;
  SUP_HIP(S.each ? lhafe_occupancy(&occ) : haf_occupancy(S.loop, &occ));
  if ((rc = ensure(c->d_cbtab, c->cbtab_cap, (size_t)S.tab_doubles))) return rc;
  if ((rc = ensure(c->d_cbU, c->cbU_cap, a_doubles + mu_doubles))) return rc;
  if ((rc = ensure(c->d_chunk, c->chunk_cap, (size_t)(2 * chunks)))) return rc;
  if ((rc = ensure(c->d_cbout, c->cbout_cap, (size_t)(K * 2)))) return rc;
  if ((rc = ensure(c->d_fock, c->fock_cap, u_end))) return rc;
  hipStream_t s = c->stream;
  c->tables_uid = 0;  // the walk leaves head 0 nonzero
  c->head_zero[0] = false;
  auto up = [&](void* dst, const void* src, size_t bytes) {
    return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s) : hipSuccess;
  };
  SUP_HIP(up(c->d_cbU, in.A, a_doubles * sizeof(double)));
  SUP_HIP(up(c->d_cbU + a_doubles, mu_src, mu_doubles * sizeof(double)));
  SUP_HIP(up(c->d_fock + u_murow, S.mu_row.data(), S.mu_row.size() * sizeof(int32_t)));
  SUP_HIP(up(c->d_fock + u_grp, S.grp.data(), S.grp.size() * sizeof(int32_t)));
  SUP_HIP(up(c->d_fock + u_prog, S.prog.data(), S.prog.size() * sizeof(HafStep)));
  SUP_HIP(up(c->d_fock + u_dig, S.dig.data(), S.dig.size() * sizeof(HafDigit)));
  SUP_HIP(up(c->d_fock + u_mats, S.mats.data(), K * sizeof(HafMat)));
  SUP_HIP(up(c->d_fock + u_chunks, S.chunks.data(), chunks * sizeof(FockChunk)));
  SUP_HIP(up(c->d_fock + u_wts, wts.data(), wts.size() * sizeof(double)));
  SUP_HIP(up(c->d_fock + u_coef, S.coef.data(), S.coef.size() * sizeof(double)));
  SUP_HIP(hipMemsetAsync(c->d_counter, 0, sizeof(unsigned), s));
  const uint64_t resident = (uint64_t)c->cus * (uint64_t)std::max(occ, 1);
  const char* fg = std::getenv("SUP_WALK_GROUP");  // tests, read per call: chunks per ticket (the bits do not change)
  const LaunchGeom geo = walk_geometry(chunks, resident, kWavesPerBlock, false, fg ? std::max(1, std::atoi(fg)) : 0);
  HafParams p{};
  p.tabs = c->d_cbtab;
  p.prog = reinterpret_cast<const HafStep*>(c->d_fock + u_prog);
  p.dig = reinterpret_cast<const HafDigit*>(c->d_fock + u_dig);
  p.mats = reinterpret_cast<const HafMat*>(c->d_fock + u_mats);
  p.chunks = reinterpret_cast<const FockChunk*>(c->d_fock + u_chunks);
  p.wts = reinterpret_cast<const double*>(c->d_fock + u_wts);
  p.coef = reinterpret_cast<const double*>(c->d_fock + u_coef);
  p.chunk_count = chunks;
  p.chunk_out = c->d_chunk;
  p.counter = c->d_counter;
  p.group = geo.group;
  p.n = (unsigned)S.n;
  SUP_HIP(hipEventRecord(c->ev0, s));
  SUP_ON_DEVICE(c->dev, "hafnian walk launch");
  if (S.each) {
    SUP_HIP(launch_lhafe_prepare(c->d_cbU, in.M, c->d_cbU + a_doubles,
                                 reinterpret_cast<const int32_t*>(c->d_fock + u_murow),
                                 reinterpret_cast<const int32_t*>(c->d_fock + u_grp), p.mats, K, c->d_cbtab, s));
    SUP_HIP(launch_lhafe(p, (int)geo.grid, s));
  } else {
    SUP_HIP(launch_haf_prepare(c->d_cbU, in.M, S.loop ? c->d_cbU + a_doubles : nullptr,
                               reinterpret_cast<const int32_t*>(c->d_fock + u_grp), p.mats, K, c->d_cbtab, s));
    SUP_HIP(launch_haf(S.loop, p, (int)geo.grid, s));
  }
  SUP_HIP(launch_haf_fold(c->d_chunk, p.mats, K, S.div, c->d_cbout, s));
  SUP_HIP(hipEventRecord(c->ev1, s));
  SUP_HIP(hipMemcpyAsync(out, c->d_cbout, (size_t)(K * 2) * sizeof(double), hipMemcpyDeviceToHost, s));
  if (grid_out) *grid_out = (int)geo.grid;
  return timed_sync(c, kernel_ms);
}

// Double-double hafnian walk (walk_hafdd.hip) of slab S on device `dev`, as
// run_hafnian's: A, mu and the slab's descriptor pools (the dd program, the dd
// weight triangle, the dd coefficients) go up, then prepare, the walk over the
// slab's queue and the per-matrix fold run on the context's stream, and one
// download brings 32 bytes per matrix into out.  The buffers are the
// collision-aware walk's (same context lock).
int run_hafnian_quad(int dev, const HafddSlab& S, const HafIn& in, double* out, double* kernel_ms, int* grid_out) {
  if (kernel_ms) *kernel_ms = 0.0;
  if (grid_out) *grid_out = 0;
  const uint64_t K = S.mats.size(), chunks = S.chunks.size();
  if (K == 0) return SUP_OK;
  const bool shape_ok = S.n >= 1 && S.n <= SUP_MAX_N && (S.loop || !(S.n & 1)) &&
                        (!S.loop || S.coef.size() == 2 * ((size_t)S.n / 2 + 1));
  if (!shape_ok || chunks == 0 || chunks > 0x7fffffffull || !out || !in.A || in.M < 1 || (S.loop && !in.mu)) {
    set_error("run_hafnian_quad: bad request");
    return SUP_EINVAL;
  }
  const std::vector<double>& wts = hafdd_weights();
  // the packed pools, each starting on a 16-byte unit (the program first: its entries are read 16 bytes at a time)
  auto units = [](size_t bytes) { return (bytes + 15) / 16; };
  const size_t u_prog = 0, u_dig = u_prog + units(S.prog.size() * sizeof(HafddStep));
  const size_t u_mats = u_dig + units(S.dig.size() * sizeof(HafDigit));
  const size_t u_chunks = u_mats + units(K * sizeof(HafMat));
  const size_t u_wts = u_chunks + units(chunks * sizeof(FockChunk));
  const size_t u_grp = u_wts + units(wts.size() * sizeof(double));
  const size_t u_coef = u_grp + units(S.grp.size() * sizeof(int32_t));
  const size_t u_end = u_coef + units(S.coef.size() * sizeof(double)) + 1;
  const size_t a_doubles = (size_t)2 * in.M * in.M;
  const size_t mu_doubles = S.loop ? (size_t)2 * in.M : 0;
  CtxGuard guard;
  int rc = guard.open(dev, "device buffers");
  if (rc) return rc;
  DeviceCtx* c = guard.c;
  int occ = 0;
  SUP_HIP(hafdd_occupancy(S.loop, &occ));
  if ((rc = ensure(c->d_cbtab, c->cbtab_cap, (size_t)S.tab_doubles))) return rc;
  if ((rc = ensure(c->d_cbU, c->cbU_cap, a_doubles + mu_doubles))) return rc;
  if ((rc = ensure(c->d_chunk, c->chunk_cap, (size_t)(4 * chunks)))) return rc;
  if ((rc = ensure(c->d_cbout, c->cbout_cap, (size_t)(K * 4)))) return rc;
  if ((rc = ensure(c->d_fock, c->fock_cap, u_end))) return rc;
  hipStream_t s = c->stream;
  c->tables_uid = 0;  // the walk leaves head 0 nonzero
  c->head_zero[0] = false;
  auto up = [&](void* dst, const void* src, size_t bytes) {
    return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s) : hipSuccess;
  };
  SUP_HIP(up(c->d_cbU, in.A, a_doubles * sizeof(double)));
  SUP_HIP(up(c->d_cbU + a_doubles, in.mu, mu_doubles * sizeof(double)));
  SUP_HIP(up(c->d_fock + u_grp, S.grp.data(), S.grp.size() * sizeof(int32_t)));
  SUP_HIP(up(c->d_fock + u_prog, S.prog.data(), S.prog.size() * sizeof(HafddStep)));
  SUP_HIP(up(c->d_fock + u_dig, S.dig.data(), S.dig.size() * sizeof(HafDigit)));
  SUP_HIP(up(c->d_fock + u_mats, S.mats.data(), K * sizeof(HafMat)));
  SUP_HIP(up(c->d_fock + u_chunks, S.chunks.data(), chunks * sizeof(FockChunk)));
  SUP_HIP(up(c->d_fock + u_wts, wts.data(), wts.size() * sizeof(double)));
  SUP_HIP(up(c->d_fock + u_coef, S.coef.data(), S.coef.size() * sizeof(double)));
  SUP_HIP(hipMemsetAsync(c->d_counter, 0, sizeof(unsigned), s));
  const uint64_t resident = (uint64_t)c->cus * (uint64_t)std::max(occ, 1);
  const char* fg = std::getenv("SUP_WALK_GROUP");  // tests, read per call: chunks per ticket (the bits do not change)
  const LaunchGeom geo = walk_geometry(chunks, resident, kWavesPerBlock, false, fg ? std::max(1, std::atoi(fg)) : 0);
  HafddParams p{};
  p.tabs = c->d_cbtab;
  p.prog = reinterpret_cast<const HafddStep*>(c->d_fock + u_prog);
  p.dig = reinterpret_cast<const HafDigit*>(c->d_fock + u_dig);
  p.mats = reinterpret_cast<const HafMat*>(c->d_fock + u_mats);
  p.chunks = reinterpret_cast<const FockChunk*>(c->d_fock + u_chunks);
  p.wts = reinterpret_cast<const double*>(c->d_fock + u_wts);
  p.coef = reinterpret_cast<const double*>(c->d_fock + u_coef);
  p.chunk_count = chunks;
  p.chunk_out = c->d_chunk;
  p.counter = c->d_counter;
  p.group = geo.group;
  p.n = (unsigned)S.n;
  SUP_HIP(hipEventRecord(c->ev0, s));
  SUP_ON_DEVICE(c->dev, "double-double hafnian walk launch");
  SUP_HIP(launch_hafdd_prepare(c->d_cbU, in.M, S.loop ? c->d_cbU + a_doubles : nullptr,
                               reinterpret_cast<const int32_t*>(c->d_fock + u_grp), p.mats, K, c->d_cbtab, s));
  SUP_HIP(launch_hafdd(S.loop, p, (int)geo.grid, s));
  SUP_HIP(launch_hafdd_fold(c->d_chunk, p.mats, K, S.div.hi, S.div.lo, S.loop, c->d_cbout, s));
  SUP_HIP(hipEventRecord(c->ev1, s));
  SUP_HIP(hipMemcpyAsync(out, c->d_cbout, (size_t)(K * 4) * sizeof(double), hipMemcpyDeviceToHost, s));
  if (grid_out) *grid_out = (int)geo.grid;
  return timed_sync(c, kernel_ms);
}

// Exact hafnian walk (walk_hafexact.hip) of slab S on device `dev`, as
// run_hafnian's: A, mu and the slab's descriptor pools go up and prepare writes
// the integer tables once; then, per launch of at most kHafxPrimes primes,
// those primes' blocks of ptab go up, the walk runs over the slab's queue and
// the per-matrix fold leaves 16 kHafxPrimes bytes per matrix, which one
// download brings back.  The buffers are the collision-aware walk's (same
// context lock).  A launch's kernels are timed by the context's event pair.
int run_hafnian_exact(int dev, const HafSlab& S, const HafIn& in, const std::vector<double>& primes,
                      const std::vector<double>& ptab, uint64_t* res, double* kernel_ms, int* grid_out,
                      int* launches_out) {
  if (kernel_ms) *kernel_ms = 0.0;
  if (grid_out) *grid_out = 0;
  if (launches_out) *launches_out = 0;
  const uint64_t K = S.mats.size(), chunks = S.chunks.size();
  if (K == 0) return SUP_OK;
  const size_t np = primes.size();
  const uint64_t stride = hafx_stride(S.prog.size());
  if (S.n < 1 || S.n > SUP_MAX_N || (!S.loop && (S.n & 1)) || chunks == 0 || chunks > 0x7fffffffull || !res || !in.A ||
      in.M < 1 || (S.loop && !in.mu) || np == 0 || ptab.size() != np * stride ||
      stride * 8 * (uint64_t)kHafxPrimes > 0xffffffffull) {
    set_error("run_hafnian_exact: bad request");
    return SUP_EINVAL;
  }
  // the packed pools, each starting on a 16-byte unit
  auto units = [](size_t bytes) { return (bytes + 15) / 16; };
  const size_t u_prog = 0, u_dig = u_prog + units(S.prog.size() * sizeof(HafStep));
  const size_t u_mats = u_dig + units(S.dig.size() * sizeof(HafDigit));
  const size_t u_chunks = u_mats + units(K * sizeof(HafMat));
  const size_t u_grp = u_chunks + units(chunks * sizeof(FockChunk));
  const size_t u_ptab = (u_grp + units(S.grp.size() * sizeof(int32_t)) + 3) / 4 * 4;  // on 64 bytes
  const size_t u_end = u_ptab + units((size_t)kHafxPrimes * stride * sizeof(double)) + 1;
  const size_t a_doubles = (size_t)2 * in.M * in.M, mu_doubles = S.loop ? (size_t)2 * in.M : 0;
  constexpr size_t per = 2 * (size_t)kHafxPrimes;  // doubles per wave-chunk and per matrix of a launch
  CtxGuard guard;
  int rc = guard.open(dev, "device buffers");
  if (rc) return rc;
  DeviceCtx* c = guard.c;
  int occ = 0;
  SUP_HIP(hafexact_occupancy(S.loop, &occ));
  if ((rc = ensure(c->d_cbtab, c->cbtab_cap, (size_t)S.tab_doubles))) return rc;
  if ((rc = ensure(c->d_cbU, c->cbU_cap, a_doubles + mu_doubles))) return rc;
  if ((rc = ensure(c->d_chunk, c->chunk_cap, (size_t)chunks * per))) return rc;
  if ((rc = ensure(c->d_cbout, c->cbout_cap, (size_t)K * per))) return rc;
  if ((rc = ensure(c->d_fock, c->fock_cap, u_end))) return rc;
  hipStream_t s = c->stream;
  c->tables_uid = 0;  // the walk leaves head 0 nonzero
  c->head_zero[0] = false;
  auto up = [&](void* dst, const void* src, size_t bytes) {
    return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s) : hipSuccess;
  };
  SUP_HIP(up(c->d_cbU, in.A, a_doubles * sizeof(double)));
  SUP_HIP(up(c->d_cbU + a_doubles, in.mu, mu_doubles * sizeof(double)));
  SUP_HIP(up(c->d_fock + u_grp, S.grp.data(), S.grp.size() * sizeof(int32_t)));
  SUP_HIP(up(c->d_fock + u_prog, S.prog.data(), S.prog.size() * sizeof(HafStep)));
  SUP_HIP(up(c->d_fock + u_dig, S.dig.data(), S.dig.size() * sizeof(HafDigit)));
  SUP_HIP(up(c->d_fock + u_mats, S.mats.data(), K * sizeof(HafMat)));
  SUP_HIP(up(c->d_fock + u_chunks, S.chunks.data(), chunks * sizeof(FockChunk)));
  const uint64_t resident = (uint64_t)c->cus * (uint64_t)std::max(occ, 1);
  const char* fg = std::getenv("SUP_WALK_GROUP");  // tests, read per call: chunks per ticket (the residues do not change)
  const LaunchGeom geo = walk_geometry(chunks, resident, kWavesPerBlock, false, fg ? std::max(1, std::atoi(fg)) : 0);
  HafxParams p{};
  p.tabs = c->d_cbtab;
  p.prog = reinterpret_cast<const HafStep*>(c->d_fock + u_prog);
  p.dig = reinterpret_cast<const HafDigit*>(c->d_fock + u_dig);
  p.mats = reinterpret_cast<const HafMat*>(c->d_fock + u_mats);
  p.chunks = reinterpret_cast<const FockChunk*>(c->d_fock + u_chunks);
  p.ptab = reinterpret_cast<const double*>(c->d_fock + u_ptab);
  p.chunk_count = chunks;
  p.chunk_out = c->d_chunk;
  p.counter = c->d_counter;
  p.group = geo.group;
  p.n = (unsigned)S.n;
  p.stride = (unsigned)stride;
  std::vector<double> sums((size_t)K * per);
  for (size_t q0 = 0; q0 < np; q0 += (size_t)kHafxPrimes) {
    const size_t nq = std::min(np - q0, (size_t)kHafxPrimes);
    p.nprimes = (unsigned)nq;
    SUP_HIP(up(c->d_fock + u_ptab, ptab.data() + q0 * stride, nq * stride * sizeof(double)));
    SUP_HIP(hipMemsetAsync(c->d_counter, 0, sizeof(unsigned), s));
    SUP_HIP(hipEventRecord(c->ev0, s));
    SUP_ON_DEVICE(c->dev, "exact hafnian walk launch");
    if (q0 == 0)
      SUP_HIP(launch_hafexact_prepare(c->d_cbU, in.M, S.loop ? c->d_cbU + a_doubles : nullptr,
                                      reinterpret_cast<const int32_t*>(c->d_fock + u_grp), p.mats, K, c->d_cbtab, s));
    SUP_HIP(launch_hafexact(S.loop, p, (int)geo.grid, s));
    SUP_HIP(launch_hafexact_fold(c->d_chunk, p.mats, K, (uint32_t)nq, c->d_cbout, s));
    SUP_HIP(hipEventRecord(c->ev1, s));
    SUP_HIP(hipMemcpyAsync(sums.data(), c->d_cbout, sums.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    double ms = 0.0;
    if ((rc = timed_sync(c, &ms))) return rc;
    if (kernel_ms) *kernel_ms += ms;
    if (launches_out) ++*launches_out;
    // a matrix's sum of chunk residues is an exact integer below 2^49
    for (uint64_t k = 0; k < K; ++k)
      for (size_t q = 0; q < nq; ++q) {
        const uint64_t pq = (uint64_t)primes[q0 + q];
        res[(k * np + q0 + q) * 2] = (uint64_t)sums[k * per + 2 * q] % pq;
        res[(k * np + q0 + q) * 2 + 1] = (uint64_t)sums[k * per + 2 * q + 1] % pq;
      }
  }
  if (grid_out) *grid_out = (int)geo.grid;
  return SUP_OK;
}

// Power-trace hafnian kernel (walk_hafpt.hip) on matrices [first, first + K) of
// in.idx, subsets [z_begin, z_end) of each: A, mu, the index lists and the
// coefficient table go up, then prepare (tables gathered on the device), the
// walk over the slab's queue and the per-matrix fold run on the context's
// stream, and one download brings 16 bytes per matrix into out.  The buffers
// are the collision-aware walk's (same context lock).
int run_hafnian_pt(int dev, const HafIn& in, int n, int np, uint64_t first, uint64_t K, uint64_t z_begin,
                   uint64_t z_end, const double* coef, double* out, double* kernel_ms, int* grid_out) {
  if (kernel_ms) *kernel_ms = 0.0;
  if (grid_out) *grid_out = 0;
  if (K == 0) return SUP_OK;
  const int m = np / 2, llog = hafpt_chunk_log(m);
  if (n < 1 || np != n + (n & 1) || np > SUP_HAFNIAN_PT_MAX_DEVICE_N || hafpt_lds_bytes(np) > 65536 || !out || !in.A ||
      !in.idx || in.M < 1 || (in.loop && !in.mu) || !coef || z_begin >= z_end || z_end > (1ull << m)) {
    set_error("run_hafnian_pt: bad request");
    return SUP_EINVAL;
  }
  const uint64_t cfirst = z_begin >> llog, cm = ((z_end + (1ull << llog) - 1) >> llog) - cfirst;
  const uint64_t chunks = K * cm, tab_doubles = 2 * hafpt_pairs(np);
  if (cm > 0xffffffffull || chunks > 0x7fffffffull) {
    set_error("run_hafnian_pt: too many wave-chunks in one slab");
    return SUP_EINVAL;
  }
  const size_t a_doubles = (size_t)2 * in.M * in.M, mu_doubles = in.loop ? (size_t)2 * in.M : 0;
  const size_t u_coef = (kPtCoef * sizeof(double) + 15) / 16;
  CtxGuard guard;
  int rc = guard.open(dev, "device buffers");
  if (rc) return rc;
  DeviceCtx* c = guard.c;
  int occ = 0;
  SUP_HIP(hafpt_occupancy(in.loop, np, &occ));
  if ((rc = ensure(c->d_cbtab, c->cbtab_cap, (size_t)(K * tab_doubles)))) return rc;
  if ((rc = ensure(c->d_cbidx, c->cbidx_cap, (size_t)K * n))) return rc;
  if ((rc = ensure(c->d_cbU, c->cbU_cap, a_doubles + mu_doubles))) return rc;
  if ((rc = ensure(c->d_chunk, c->chunk_cap, (size_t)(2 * chunks)))) return rc;
  if ((rc = ensure(c->d_cbout, c->cbout_cap, (size_t)(K * 2)))) return rc;
  if ((rc = ensure(c->d_fock, c->fock_cap, u_coef))) return rc;
  hipStream_t s = c->stream;
  c->tables_uid = 0;  // the walk leaves head 0 nonzero
  c->head_zero[0] = false;
  SUP_HIP(hipMemcpyAsync(c->d_cbU, in.A, a_doubles * sizeof(double), hipMemcpyHostToDevice, s));
  if (mu_doubles)
    SUP_HIP(hipMemcpyAsync(c->d_cbU + a_doubles, in.mu, mu_doubles * sizeof(double), hipMemcpyHostToDevice, s));
  SUP_HIP(hipMemcpyAsync(c->d_cbidx, in.idx + first * n, (size_t)K * n * sizeof(int32_t), hipMemcpyHostToDevice, s));
  SUP_HIP(hipMemcpyAsync(c->d_fock, coef, kPtCoef * sizeof(double), hipMemcpyHostToDevice, s));
  SUP_HIP(hipMemsetAsync(c->d_counter, 0, sizeof(unsigned), s));
  const uint64_t resident = (uint64_t)c->cus * (uint64_t)std::max(occ, 1);
  const char* fg = std::getenv("SUP_WALK_GROUP");  // tests, read per call: chunks per ticket (the bits do not change)
  const LaunchGeom geo = walk_geometry(chunks, resident, 1, false, fg ? std::max(1, std::atoi(fg)) : 0);
  PtParams p{};
  p.tabs = c->d_cbtab;
  p.coef = reinterpret_cast<const double*>(c->d_fock);
  p.chunk_count = chunks;
  p.chunk_out = c->d_chunk;
  p.counter = c->d_counter;
  p.group = geo.group;
  p.np = (unsigned)np;
  p.m = (unsigned)m;
  p.llog = (unsigned)llog;
  p.cm = (unsigned)cm;
  p.tab_doubles = (unsigned)tab_doubles;
  p.z_begin = z_begin;
  p.z_end = z_end;
  p.chunk_first = cfirst;
  SUP_HIP(hipEventRecord(c->ev0, s));
  SUP_ON_DEVICE(c->dev, "power-trace hafnian launch");
  SUP_HIP(launch_hafpt_prepare(c->d_cbU, in.M, in.loop ? c->d_cbU + a_doubles : nullptr, c->d_cbidx, n, np, K,
                               (uint32_t)tab_doubles, c->d_cbtab, s));
  SUP_HIP(launch_hafpt(in.loop, p, (int)geo.grid, s));
  SUP_HIP(launch_hafpt_fold(c->d_chunk, (uint32_t)cm, K, c->d_cbout, s));
  SUP_HIP(hipEventRecord(c->ev1, s));
  SUP_HIP(hipMemcpyAsync(out, c->d_cbout, (size_t)(K * 2) * sizeof(double), hipMemcpyDeviceToHost, s));
  if (grid_out) *grid_out = (int)geo.grid;
  return timed_sync(c, kernel_ms);
}

// Torontonian kernel (walk_tor.hip) on lists [first, first + K) of in.modes,
// subsets [z_begin, z_end) of each: O and the lists go up, then prepare (the
// gathered matrices, on the device), the walk over the slab's queue and the
// per-list fold run on the context's stream, and one download brings 8 bytes
// per list into out.  The buffers are the collision-aware walk's (same context
// lock).
int run_torontonian(int dev, const TorIn& in, int n, uint64_t first, uint64_t K, uint64_t z_begin, uint64_t z_end,
                    double* out, double* kernel_ms, int* grid_out) {
  if (kernel_ms) *kernel_ms = 0.0;
  if (grid_out) *grid_out = 0;
  if (K == 0) return SUP_OK;
  if (n < 1 || n > SUP_TORONTONIAN_MAX_DEVICE_N || tor_lds_bytes(n) > 65536 || !out || !in.O || !in.modes || in.M < 1 ||
      z_begin >= z_end || z_end > (1ull << n)) {
    set_error("run_torontonian: bad request");
    return SUP_EINVAL;
  }
  const int llog = tor_chunk_log(n);
  const uint64_t cfirst = z_begin >> llog, cm = ((z_end + (1ull << llog) - 1) >> llog) - cfirst;
  const uint64_t chunks = K * cm, g_doubles = tor_g_doubles(n);
  if (cm > 0xffffffffull || chunks > 0x7fffffffull) {
    set_error("run_torontonian: too many wave-chunks in one slab");
    return SUP_EINVAL;
  }
  const size_t o_doubles = (size_t)8 * in.M * in.M;
  CtxGuard guard;
  int rc = guard.open(dev, "device buffers");
  if (rc) return rc;
  DeviceCtx* c = guard.c;
  int occ = 0;
  SUP_HIP(tor_occupancy(n, &occ));
  if ((rc = ensure(c->d_cbtab, c->cbtab_cap, (size_t)(K * g_doubles)))) return rc;
  if ((rc = ensure(c->d_cbidx, c->cbidx_cap, (size_t)K * n))) return rc;
  if ((rc = ensure(c->d_cbU, c->cbU_cap, o_doubles))) return rc;
  if ((rc = ensure(c->d_chunk, c->chunk_cap, (size_t)(2 * chunks)))) return rc;
  if ((rc = ensure(c->d_cbout, c->cbout_cap, (size_t)K))) return rc;
  hipStream_t s = c->stream;
  c->tables_uid = 0;  // the walk leaves head 0 nonzero
  c->head_zero[0] = false;
  SUP_HIP(hipMemcpyAsync(c->d_cbU, in.O, o_doubles * sizeof(double), hipMemcpyHostToDevice, s));
  SUP_HIP(hipMemcpyAsync(c->d_cbidx, in.modes + first * n, (size_t)K * n * sizeof(int32_t), hipMemcpyHostToDevice, s));
  SUP_HIP(hipMemsetAsync(c->d_counter, 0, sizeof(unsigned), s));
  const uint64_t resident = (uint64_t)c->cus * (uint64_t)std::max(occ, 1);
  const char* fg = std::getenv("SUP_WALK_GROUP");  // tests, read per call: chunks per ticket (the bits do not change)
  const LaunchGeom geo = walk_geometry(chunks, resident, 1, false, fg ? std::max(1, std::atoi(fg)) : 0);
  TorParams p{};
  p.G = c->d_cbtab;
  p.chunk_count = chunks;
  p.chunk_out = c->d_chunk;
  p.counter = c->d_counter;
  p.group = geo.group;
  p.n = (unsigned)n;
  p.nn = (unsigned)tor_nn(n);
  p.llog = (unsigned)llog;
  p.cm = (unsigned)cm;
  p.z_begin = z_begin;
  p.z_end = z_end;
  p.chunk_first = cfirst;
  SUP_HIP(hipEventRecord(c->ev0, s));
  SUP_ON_DEVICE(c->dev, "torontonian launch");
  SUP_HIP(launch_tor_prepare(c->d_cbU, in.M, c->d_cbidx, n, K, c->d_cbtab, s));
  SUP_HIP(launch_tor(p, (int)geo.grid, s));
  SUP_HIP(launch_tor_fold(c->d_chunk, (uint32_t)cm, K, c->d_cbout, s));
  SUP_HIP(hipEventRecord(c->ev1, s));
  SUP_HIP(hipMemcpyAsync(out, c->d_cbout, (size_t)K * sizeof(double), hipMemcpyDeviceToHost, s));
  if (grid_out) *grid_out = (int)geo.grid;
  return timed_sync(c, kernel_ms);
}

// Loop torontonian kernel (walk_ltor.hip), as run_torontonian: O, gamma (behind
// O in the same buffer) and the lists go up once, prepare gathers the matrices
// and border rows on the device, then the walk and the torontonian's fold.
int run_loop_torontonian(int dev, const LtorIn& in, int n, uint64_t first, uint64_t K, uint64_t z_begin, uint64_t z_end,
                         double* out, double* kernel_ms, int* grid_out) {
  if (kernel_ms) *kernel_ms = 0.0;
  if (grid_out) *grid_out = 0;
  if (K == 0) return SUP_OK;
  if (n < 1 || n > SUP_LOOP_TORONTONIAN_MAX_DEVICE_N || ltor_lds_bytes(n) > 65536 || !out || !in.O || !in.gamma ||
      !in.modes || in.M < 1 || z_begin >= z_end || z_end > (1ull << n)) {
    set_error("run_loop_torontonian: bad request");
    return SUP_EINVAL;
  }
  const int llog = tor_chunk_log(n);
  const uint64_t cfirst = z_begin >> llog, cm = ((z_end + (1ull << llog) - 1) >> llog) - cfirst;
  const uint64_t chunks = K * cm, g_doubles = ltor_g_doubles(n);
  if (cm > 0xffffffffull || chunks > 0x7fffffffull) {
    set_error("run_loop_torontonian: too many wave-chunks in one slab");
    return SUP_EINVAL;
  }
  const size_t o_doubles = (size_t)8 * in.M * in.M, gm_doubles = (size_t)4 * in.M;
  CtxGuard guard;
  int rc = guard.open(dev, "device buffers");
  if (rc) return rc;
  DeviceCtx* c = guard.c;
  int occ = 0;
  SUP_HIP(ltor_occupancy(n, &occ));
  if ((rc = ensure(c->d_cbtab, c->cbtab_cap, (size_t)(K * g_doubles)))) return rc;
  if ((rc = ensure(c->d_cbidx, c->cbidx_cap, (size_t)K * n))) return rc;
  if ((rc = ensure(c->d_cbU, c->cbU_cap, o_doubles + gm_doubles))) return rc;
  if ((rc = ensure(c->d_chunk, c->chunk_cap, (size_t)(2 * chunks)))) return rc;
  if ((rc = ensure(c->d_cbout, c->cbout_cap, (size_t)K))) return rc;
  hipStream_t s = c->stream;
  c->tables_uid = 0;  // the walk leaves head 0 nonzero
  c->head_zero[0] = false;
  SUP_HIP(hipMemcpyAsync(c->d_cbU, in.O, o_doubles * sizeof(double), hipMemcpyHostToDevice, s));
  SUP_HIP(hipMemcpyAsync(c->d_cbU + o_doubles, in.gamma, gm_doubles * sizeof(double), hipMemcpyHostToDevice, s));
  SUP_HIP(hipMemcpyAsync(c->d_cbidx, in.modes + first * n, (size_t)K * n * sizeof(int32_t), hipMemcpyHostToDevice, s));
  SUP_HIP(hipMemsetAsync(c->d_counter, 0, sizeof(unsigned), s));
  const uint64_t resident = (uint64_t)c->cus * (uint64_t)std::max(occ, 1);
  const char* fg = std::getenv("SUP_WALK_GROUP");  // tests, read per call: chunks per ticket (the bits do not change)
  const LaunchGeom geo = walk_geometry(chunks, resident, 1, false, fg ? std::max(1, std::atoi(fg)) : 0);
  TorParams p{};
  p.G = c->d_cbtab;
  p.chunk_count = chunks;
  p.chunk_out = c->d_chunk;
  p.counter = c->d_counter;
  p.group = geo.group;
  p.n = (unsigned)n;
  p.nn = (unsigned)tor_nn(n);
  p.llog = (unsigned)llog;
  p.cm = (unsigned)cm;
  p.z_begin = z_begin;
  p.z_end = z_end;
  p.chunk_first = cfirst;
  SUP_HIP(hipEventRecord(c->ev0, s));
  SUP_ON_DEVICE(c->dev, "loop torontonian launch");
  SUP_HIP(launch_ltor_prepare(c->d_cbU, in.M, c->d_cbU + o_doubles, c->d_cbidx, n, K, c->d_cbtab, s));
  SUP_HIP(launch_ltor(p, (int)geo.grid, s));
  SUP_HIP(launch_tor_fold(c->d_chunk, (uint32_t)cm, K, c->d_cbout, s));
  SUP_HIP(hipEventRecord(c->ev1, s));
  SUP_HIP(hipMemcpyAsync(out, c->d_cbout, (size_t)K * sizeof(double), hipMemcpyDeviceToHost, s));
  if (grid_out) *grid_out = (int)geo.grid;
  return timed_sync(c, kernel_ms);
}

// The ragged loop torontonian kernel (walk_ltore in walk_ltor.hip) on one slab
// of items of any orders: O, the slab's gamma rows (behind O), the lists and
// the descriptors go up once, then the ragged prepare, the walk over the
// slab's one queue and the per-item fold, and one download brings 8 bytes per
// item into out.  The buffers are run_loop_torontonian's, the descriptors in
// the collision-aware walk's.
int run_loop_torontonian_each(int dev, const LtorEachIn& in, const LtorEachSlab& S, double* out, double* kernel_ms,
                              int* grid_out) {
  if (kernel_ms) *kernel_ms = 0.0;
  if (grid_out) *grid_out = 0;
  const uint64_t K = S.items.size();
  if (K == 0) return SUP_OK;
  if (!out || !in.O || !in.gamma || in.M < 1 || S.stride < 1 || S.modes.size() != K * (uint64_t)S.stride || S.max_n < 1 ||
      S.max_n > SUP_LOOP_TORONTONIAN_MAX_DEVICE_N || ltor_lds_bytes(S.max_n) > 65536 || S.rows < 1 ||
      S.row_lo + S.rows > in.ngamma || S.chunks < K || S.chunks > 0x7fffffffull) {
    set_error("run_loop_torontonian_each: bad request");
    return SUP_EINVAL;
  }
  // the kernel trusts the descriptors: every one is checked here
  uint64_t goff = 0, coff = 0;
  for (const LtorItem& d : S.items) {
    if (d.n < 1 || d.n > (unsigned)S.max_n || d.nn != (unsigned)tor_nn((int)d.n) || d.llog != (unsigned)tor_chunk_log((int)d.n) ||
        d.cm != ltor_item_chunks((int)d.n) || d.g_off != goff || d.chunk0 != coff || d.row >= S.rows) {
      set_error("run_loop_torontonian_each: bad item descriptor");
      return SUP_EINVAL;
    }
    goff += ltor_g_doubles((int)d.n), coff += d.cm;
  }
  if (goff != S.g_doubles || coff != S.chunks) {
    set_error("run_loop_torontonian_each: bad slab totals");
    return SUP_EINVAL;
  }
  const size_t o_doubles = (size_t)8 * in.M * in.M, gm_doubles = (size_t)4 * in.M * (size_t)S.rows;
  CtxGuard guard;
  int rc = guard.open(dev, "device buffers");
  if (rc) return rc;
  DeviceCtx* c = guard.c;
  int occ = 0;
  SUP_HIP(ltore_occupancy(S.max_n, &occ));
  if ((rc = ensure(c->d_cbtab, c->cbtab_cap, (size_t)S.g_doubles))) return rc;
  if ((rc = ensure(c->d_cbidx, c->cbidx_cap, S.modes.size()))) return rc;
  if ((rc = ensure(c->d_cbU, c->cbU_cap, o_doubles + gm_doubles))) return rc;
  if ((rc = ensure(c->d_chunk, c->chunk_cap, (size_t)(2 * S.chunks)))) return rc;
  if ((rc = ensure(c->d_cbout, c->cbout_cap, (size_t)K))) return rc;
  if ((rc = ensure(c->d_fock, c->fock_cap, (size_t)K * (sizeof(LtorItem) / 16)))) return rc;
  hipStream_t s = c->stream;
  c->tables_uid = 0;  // the walk leaves head 0 nonzero
  c->head_zero[0] = false;
  SUP_HIP(hipMemcpyAsync(c->d_cbU, in.O, o_doubles * sizeof(double), hipMemcpyHostToDevice, s));
  SUP_HIP(hipMemcpyAsync(c->d_cbU + o_doubles, in.gamma + 4ull * (uint64_t)in.M * S.row_lo, gm_doubles * sizeof(double),
                         hipMemcpyHostToDevice, s));
  SUP_HIP(hipMemcpyAsync(c->d_cbidx, S.modes.data(), S.modes.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
  SUP_HIP(hipMemcpyAsync(c->d_fock, S.items.data(), (size_t)K * sizeof(LtorItem), hipMemcpyHostToDevice, s));
  SUP_HIP(hipMemsetAsync(c->d_counter, 0, sizeof(unsigned), s));
  const uint64_t resident = (uint64_t)c->cus * (uint64_t)std::max(occ, 1);
  const char* fg = std::getenv("SUP_WALK_GROUP");  // tests, read per call: slots per ticket (the bits do not change)
  const LaunchGeom geo = walk_geometry(S.chunks, resident, 1, false, fg ? std::max(1, std::atoi(fg)) : 0);
  LtorEachParams p{};
  p.G = c->d_cbtab;
  p.items = reinterpret_cast<const LtorItem*>(c->d_fock);
  p.item_count = (unsigned)K;
  p.group = geo.group;
  p.chunk_count = S.chunks;
  p.chunk_out = c->d_chunk;
  p.counter = c->d_counter;
  SUP_HIP(hipEventRecord(c->ev0, s));
  SUP_ON_DEVICE(c->dev, "ragged loop torontonian launch");
  SUP_HIP(launch_ltore_prepare(c->d_cbU, in.M, c->d_cbU + o_doubles, c->d_cbidx, S.stride, p.items, K, c->d_cbtab, s));
  SUP_HIP(launch_ltore(p, S.max_n, (int)geo.grid, s));
  SUP_HIP(launch_ltore_fold(c->d_chunk, p.items, K, c->d_cbout, s));
  SUP_HIP(hipEventRecord(c->ev1, s));
  SUP_HIP(hipMemcpyAsync(out, c->d_cbout, (size_t)K * sizeof(double), hipMemcpyDeviceToHost, s));
  if (grid_out) *grid_out = (int)geo.grid;
  return timed_sync(c, kernel_ms);
}

// A table of 2^n doubles lives in d_cbout; one above kTableKeepBytes is given
// back after the call instead of staying with the context.
constexpr size_t kTableKeepBytes = (size_t)256 << 20;
static void release_table(DeviceCtx* c) {
  if (c->cbout_cap * sizeof(double) <= kTableKeepBytes) return;
  (void)hipFree(c->d_cbout);
  c->d_cbout = nullptr;
  c->cbout_cap = 0;
}

// Torontonian table (walk_tor.hip's and walk_ltor.hip's table forms, then
// mobius.hip) of the one list in.modes: O (and gamma behind it) and the list go
// up, prepare gathers the matrix on the device, the table walk stores f(z) of
// every z, the transform's passes follow on the same stream, and one download
// brings the 2^n doubles into out.
int run_torontonian_table(int dev, const LtorIn& in, bool loop, int n, bool transform, int L, int K, double* out,
                          double* kernel_ms, int* grid_out) {
  if (kernel_ms) *kernel_ms = 0.0;
  if (grid_out) *grid_out = 0;
  if (n < 1 || n > kTorTabMaxN || (loop ? ltor_lds_bytes(n) : tor_lds_bytes(n)) > 65536 || !out || !in.O || !in.modes ||
      (loop && !in.gamma) || in.M < 1) {
    set_error("run_torontonian_table: bad request");
    return SUP_EINVAL;
  }
  const int llog = tor_chunk_log(n);
  const uint64_t total = 1ull << n, cm = (total + (1ull << llog) - 1) >> llog;
  const uint64_t g_doubles = loop ? ltor_g_doubles(n) : tor_g_doubles(n);
  const size_t o_doubles = (size_t)8 * in.M * in.M, gm_doubles = loop ? (size_t)4 * in.M : 0;
  CtxGuard guard;
  int rc = guard.open(dev, "device buffers");
  if (rc) return rc;
  DeviceCtx* c = guard.c;
  int occ = 0;
  SUP_HIP(loop ? ltor_table_occupancy(n, &occ) : tor_table_occupancy(n, &occ));
  if ((rc = ensure(c->d_cbtab, c->cbtab_cap, (size_t)g_doubles))) return rc;
  if ((rc = ensure(c->d_cbidx, c->cbidx_cap, (size_t)n))) return rc;
  if ((rc = ensure(c->d_cbU, c->cbU_cap, o_doubles + gm_doubles))) return rc;
  if ((rc = ensure(c->d_cbout, c->cbout_cap, (size_t)total))) return rc;
  hipStream_t s = c->stream;
  c->tables_uid = 0;  // the walk leaves head 0 nonzero
  c->head_zero[0] = false;
  SUP_HIP(hipMemcpyAsync(c->d_cbU, in.O, o_doubles * sizeof(double), hipMemcpyHostToDevice, s));
  if (loop) SUP_HIP(hipMemcpyAsync(c->d_cbU + o_doubles, in.gamma, gm_doubles * sizeof(double), hipMemcpyHostToDevice, s));
  SUP_HIP(hipMemcpyAsync(c->d_cbidx, in.modes, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
  SUP_HIP(hipMemsetAsync(c->d_counter, 0, sizeof(unsigned), s));
  const uint64_t resident = (uint64_t)c->cus * (uint64_t)std::max(occ, 1);
  const char* fg = std::getenv("SUP_WALK_GROUP");  // tests, read per call: chunks per ticket (the bits do not change)
  const LaunchGeom geo = walk_geometry(cm, resident, 1, false, fg ? std::max(1, std::atoi(fg)) : 0);
  TorParams p{};
  p.G = c->d_cbtab;
  p.chunk_count = cm;
  p.chunk_out = c->d_cbout;
  p.counter = c->d_counter;
  p.group = geo.group;
  p.n = (unsigned)n;
  p.nn = (unsigned)tor_nn(n);
  p.llog = (unsigned)llog;
  p.cm = (unsigned)cm;
  p.z_begin = 0;
  p.z_end = total;
  p.chunk_first = 0;
  SUP_HIP(hipEventRecord(c->ev0, s));
  SUP_ON_DEVICE(c->dev, "torontonian table launch");
  if (loop) {
    SUP_HIP(launch_ltor_prepare(c->d_cbU, in.M, c->d_cbU + o_doubles, c->d_cbidx, n, 1, c->d_cbtab, s));
    SUP_HIP(launch_ltor_table(p, (int)geo.grid, s));
  } else {
    SUP_HIP(launch_tor_prepare(c->d_cbU, in.M, c->d_cbidx, n, 1, c->d_cbtab, s));
    SUP_HIP(launch_tor_table(p, (int)geo.grid, s));
  }
  if (transform) SUP_HIP(launch_mobius(c->d_cbout, n, L, K, c->cus * 8, s));
  SUP_HIP(hipEventRecord(c->ev1, s));
  SUP_HIP(hipMemcpyAsync(out, c->d_cbout, (size_t)total * sizeof(double), hipMemcpyDeviceToHost, s));
  if (grid_out) *grid_out = (int)geo.grid;
  rc = timed_sync(c, kernel_ms);
  release_table(c);
  return rc;
}

// t[0 .. 2^n) up, mobius.hip's passes, and down again (sup_mobius_subsets).
int run_mobius(int dev, double* t, int n, int L, int K) {
  if (!t || n < 0 || n > kTorTabMaxN) {
    set_error("run_mobius: bad request");
    return SUP_EINVAL;
  }
  if (n == 0) return SUP_OK;
  const uint64_t total = 1ull << n;
  CtxGuard guard;
  int rc = guard.open(dev, "device buffers");
  if (rc) return rc;
  DeviceCtx* c = guard.c;
  if ((rc = ensure(c->d_cbout, c->cbout_cap, (size_t)total))) return rc;
  hipStream_t s = c->stream;
  SUP_HIP(hipMemcpyAsync(c->d_cbout, t, (size_t)total * sizeof(double), hipMemcpyHostToDevice, s));
  SUP_HIP(hipEventRecord(c->ev0, s));
  SUP_ON_DEVICE(c->dev, "mobius launch");
  SUP_HIP(launch_mobius(c->d_cbout, n, L, K, c->cus * 8, s));
  SUP_HIP(hipEventRecord(c->ev1, s));
  SUP_HIP(hipMemcpyAsync(t, c->d_cbout, (size_t)total * sizeof(double), hipMemcpyDeviceToHost, s));
  double ms = 0.0;
  rc = timed_sync(c, &ms);
  release_table(c);
  return rc;
}

// out[i] = ltor_exp(x[i]) on the device (sup_ltor_exp_device), in the
// collision-aware walk's buffers.
int run_ltor_exp(int dev, const double* x, uint64_t count, double* out) {
  if (count == 0) return SUP_OK;
  if (!x || !out) {
    set_error("run_ltor_exp: null pointer");
    return SUP_EINVAL;
  }
  CtxGuard guard;
  int rc = guard.open(dev, "device buffers");
  if (rc) return rc;
  DeviceCtx* c = guard.c;
  if ((rc = ensure(c->d_cbtab, c->cbtab_cap, (size_t)count))) return rc;
  if ((rc = ensure(c->d_cbout, c->cbout_cap, (size_t)count))) return rc;
  hipStream_t s = c->stream;
  SUP_HIP(hipMemcpyAsync(c->d_cbtab, x, (size_t)count * sizeof(double), hipMemcpyHostToDevice, s));
  SUP_HIP(hipEventRecord(c->ev0, s));
  SUP_ON_DEVICE(c->dev, "ltor_exp launch");
  SUP_HIP(launch_ltor_exp(c->d_cbtab, count, c->d_cbout, s));
  SUP_HIP(hipEventRecord(c->ev1, s));
  SUP_HIP(hipMemcpyAsync(out, c->d_cbout, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, s));
  double ms = 0.0;
  return timed_sync(c, &ms);
}

// Loop-hafnian table (lhaftab.hip): A, zeta and the two root tables go up, the
// low kernel and the slab launches follow on the context's stream, and one
// download brings the 2 * entries doubles into out.  The table lives in d_cbout
// and follows release_table's rule.
int run_lhaf_table(int dev, const double* A, int M, const double* zeta, const int32_t* dims, uint64_t entries, uint32_t low,
                   double* out, double* kernel_ms, int* grid_out, uint64_t* launches) {
  if (kernel_ms) *kernel_ms = 0.0;
  if (grid_out) *grid_out = 0;
  if (launches) *launches = 0;
  if (!A || !zeta || !dims || !out || M < 1 || M > kLhafTabMaxM || entries < 1 || entries > kLhafTabMaxEntries || low < 1 ||
      low > kLhafLowTile) {
    set_error("run_lhaf_table: bad request");
    return SUP_EINVAL;
  }
  double roots[2 * kLhafTabMaxDim];
  lhaf_roots(roots, roots + kLhafTabMaxDim);
  const size_t a_doubles = (size_t)2 * M * M, z_doubles = (size_t)2 * M;
  CtxGuard guard;
  int rc = guard.open(dev, "device buffers");
  if (rc) return rc;
  DeviceCtx* c = guard.c;
  if ((rc = ensure(c->d_cbU, c->cbU_cap, a_doubles + z_doubles + 2 * kLhafTabMaxDim))) return rc;
  if ((rc = ensure(c->d_cbout, c->cbout_cap, (size_t)(2 * entries)))) return rc;
  hipStream_t s = c->stream;
  double* dz = c->d_cbU + a_doubles;
  double* ds = dz + z_doubles;
  SUP_HIP(hipMemcpyAsync(c->d_cbU, A, a_doubles * sizeof(double), hipMemcpyHostToDevice, s));
  SUP_HIP(hipMemcpyAsync(dz, zeta, z_doubles * sizeof(double), hipMemcpyHostToDevice, s));
  SUP_HIP(hipMemcpyAsync(ds, roots, sizeof(roots), hipMemcpyHostToDevice, s));
  SUP_HIP(hipEventRecord(c->ev0, s));
  SUP_ON_DEVICE(c->dev, "loop-hafnian table launch");
  SUP_HIP(launch_lhaf_table(A, zeta, roots + kLhafTabMaxDim, dims, M, low, c->d_cbU, dz, ds, ds + kLhafTabMaxDim, c->d_cbout, s,
                            launches, grid_out));
  SUP_HIP(hipEventRecord(c->ev1, s));
  SUP_HIP(hipMemcpyAsync(out, c->d_cbout, (size_t)(2 * entries) * sizeof(double), hipMemcpyDeviceToHost, s));
  rc = timed_sync(c, kernel_ms);
  release_table(c);
  return rc;
}

}  // namespace sup
