// loop_torontonian.cpp — loop torontonians of complex Hermitian matrices and a
// displacement vector gathered by lists of distinct modes:
// sup_loop_torontonian, sup_loop_torontonian_range and
// sup_loop_torontonian_plan.
//
// The sum runs over the 2^n subsets z of a list's positions (tor.hpp), each
// term the torontonian's times an exponential whose argument is the diagonal
// chain of one more row of the same factor, the border (ltor.hpp).  The
// checks, the chunking and the host twin are here.  The twin keeps the compact
// factor and the border row of the current subset and, stepping z upwards,
// recomputes only the rows and border columns at and below the highest
// position that changed.  Result k is a function of (O, gamma, modes[k]) only.
// sup_loop_torontonian_each, at the end of the file, runs lists
// of different orders, each with its own gamma row, through the same chunks.
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "cx.hpp"
#include "engine.hpp"
#include "loop_torontonian.hpp"
#include "ltor.hpp"

namespace sup {

namespace {

constexpr size_t kLtorSlabCapBytes = (size_t)256 << 20;

// The 64-lane xor butterfly (walk_ltor.hip ltor_wave_sum) on v[0..63].
double ltor_butterfly(double* v) {
  for (int off = 1; off <= 32; off <<= 1) {
    double w[64];
    for (int l = 0; l < 64; ++l) w[l] = v[l] + v[l ^ off];
    std::copy(w, w + 64, v);
  }
  return v[0];
}

// The compact factor and border row of one subset, kept between subsets.
struct LtorState {
  int N = 0;               // row stride of G and L; the border is row N of G
  std::vector<cx> L;       // compact rows, N pairs each
  std::vector<cx> w;       // the border row
  std::vector<double> rho, prod, dsum;  // dsum[i]: the border's diagonal chain after i columns
  std::vector<int> row;    // full index of compact row i
  uint64_t zprev = 0;
  bool have = false;
  explicit LtorState(int nn) : N(2 * nn), L((size_t)N * N), w(N), rho(N), prod(N + 1), dsum(N + 1), row(N) {
    prod[0] = 1.0;
    dsum[0] = 0.0;
  }
};

// Row i of the factor from rows < i, then column i of the border (tor.hpp's
// and ltor.hpp's chains).  sel: the row is selected; an unselected one is an
// identity row with w_i = +0.  selv (or null: every row above is selected):
// which of the rows above are; the columns of the others are +0.
void ltor_row(const double* G, LtorState& S, int i, bool sel, const char* selv = nullptr) {
  cx* Li = S.L.data() + (size_t)i * S.N;
  if (!sel) {
    for (int c = 0; c < i; ++c) Li[c] = cx{0.0, 0.0};
    S.rho[i] = 1.0;
    S.prod[i + 1] = S.prod[i] * S.rho[i];
    S.w[i] = cx{0.0, 0.0};
    S.dsum[i + 1] = tor_chain_diag(S.dsum[i], S.w[i]);
    return;
  }
  const int R = S.row[i];
  for (int c = 0; c < i; ++c) {
    const cx* Lc = S.L.data() + (size_t)c * S.N;
    const int C = S.row[c];
    cx acc{G[2 * ((size_t)R * S.N + C)], G[2 * ((size_t)R * S.N + C) + 1]};
    for (int l = 0; l < c; ++l) acc = tor_chain(acc, Li[l], Lc[l]);
    Li[c] = (selv && !selv[c]) ? cx{0.0, 0.0} : tor_scale(acc, S.rho[c]);
  }
  double d = G[2 * ((size_t)R * S.N + R)];
  for (int l = 0; l < i; ++l) d = tor_chain_diag(d, Li[l]);
  S.rho[i] = tor_rho(d);
  S.prod[i + 1] = S.prod[i] * S.rho[i];
  cx acc{G[2 * ((size_t)S.N * S.N + R)], G[2 * ((size_t)S.N * S.N + R) + 1]};
  for (int l = 0; l < i; ++l) acc = tor_chain(acc, S.w[l], Li[l]);
  S.w[i] = tor_scale(acc, S.rho[i]);
  S.dsum[i + 1] = tor_chain_diag(S.dsum[i], S.w[i]);
}

double ltor_term(const LtorState& S, int P) { return S.prod[P] * ltor_exp(-0.5 * S.dsum[P]); }

// f(z), compact form, reusing the rows the previous subset shares.
double ltor_f(const double* G, int nn, LtorState& S, uint64_t z) {
  int keep = 0;
  if (S.have && z != S.zprev) {
    const int top = 63 - __builtin_clzll(z ^ S.zprev);
    keep = top >= 63 ? 0 : 2 * __builtin_popcountll(z >> (top + 1));
  } else if (S.have) {
    keep = 2 * __builtin_popcountll(z);
  }
  int P = 0;
  for (int b = nn - 1; b >= 0; --b)
    if ((z >> b) & 1ull) {
      if (P >= keep) S.row[P] = 2 * (nn - 1 - b), S.row[P + 1] = 2 * (nn - 1 - b) + 1;
      P += 2;
    }
  for (int i = keep; i < P; ++i) ltor_row(G, S, i, true);
  S.zprev = z, S.have = true;
  return ltor_term(S, P);
}

// f(z) from nothing, the positions below `tail` kept in place as identity rows
// where z does not select them (the kernel's form with W = tail; tail = 0: the
// compact form without reuse).
double ltor_f_masked(const double* G, int n, int nn, LtorState& S, uint64_t z, int tail) {
  int P = 0;
  std::vector<char> sel((size_t)S.N, 1);
  for (int b = nn - 1; b >= 0; --b) {
    const bool on = (z >> b) & 1ull;
    if (!on && (b >= tail || b >= n)) continue;
    S.row[P] = 2 * (nn - 1 - b), S.row[P + 1] = 2 * (nn - 1 - b) + 1;
    sel[P] = sel[P + 1] = on;
    P += 2;
  }
  for (int i = 0; i < P; ++i) ltor_row(G, S, i, sel[i], sel.data());
  S.have = false;
  return ltor_term(S, P);
}

// The partial of wave-chunk c (tor.hpp): its 64-aligned groups ascending from
// +0, z outside [z0, z1) as +0.
double ltor_chunk(const double* G, int n, int nn, int tail, uint64_t c, uint64_t z0, uint64_t z1, LtorState& S) {
  const int llog = tor_chunk_log(n);
  const uint64_t lo = std::max(z0, c << llog), hi = std::min(z1, (c + 1) << llog);
  double acc = 0.0;
  S.have = false;
  for (uint64_t g = lo >> 6; (g << 6) < hi; ++g) {
    double v[64];
    for (int l = 0; l < 64; ++l) {
      const uint64_t z = (g << 6) + (uint64_t)l;
      if (z < lo || z >= hi) {
        v[l] = 0.0;
        continue;
      }
      // the masked form is the check on the other: it starts every subset from nothing
      const double f = tail < 0 ? ltor_f(G, nn, S, z) : ltor_f_masked(G, n, nn, S, z, tail);
      v[l] = ((n - __builtin_popcountll(z)) & 1) ? -f : f;
    }
    acc = acc + ltor_butterfly(v);
  }
  return acc;
}

void ltor_gather(const LtorIn& in, const int32_t* s, int n, std::vector<double>& G) {
  const int N = 2 * tor_nn(n);
  G.resize((size_t)ltor_g_doubles(n));
  for (int R = 0; R < N; ++R)
    for (int C = 0; C < N; ++C) {
      const cx v = tor_entry(in.O, in.M, s, n, R, C);
      G[2 * ((size_t)R * N + C)] = v.re, G[2 * ((size_t)R * N + C) + 1] = v.im;
    }
  for (int C = 0; C < N; ++C) {
    const cx v = ltor_border(in.gamma, in.M, s, n, C);
    G[2 * ((size_t)N * N + C)] = v.re, G[2 * ((size_t)N * N + C) + 1] = v.im;
  }
}

}  // namespace

// The raw table of one list (tortab.hpp), as tor_table_raw_cpu with the border.
void ltor_table_raw_cpu(const LtorIn& in, int n, int threads, double* out) {
  const int nn = tor_nn(n);
  std::vector<double> G;
  ltor_gather(in, in.modes, n, G);
  const uint64_t total = 1ull << n, run = std::min<uint64_t>(total, 512), runs = total / run;
  const int T = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)std::max(threads, 1), runs));
  std::atomic<uint64_t> next{0};
  auto work = [&]() {
    LtorState S(nn);
    for (uint64_t a = next.fetch_add(1); a < runs; a = next.fetch_add(1)) {
      S.have = false;
      for (uint64_t z = a * run; z < (a + 1) * run; ++z) out[z] = ltor_f(G.data(), nn, S, z);
    }
  };
  std::vector<std::thread> th;
  for (int w = 1; w < T; ++w) th.emplace_back(work);
  work();
  for (auto& t : th) t.join();
}

int loop_torontonian_plan(int n, uint64_t* subsets, double* est_ops) {
  if (n < 1 || n > kTorMaxN) {
    set_error("sup_loop_torontonian_plan: n = " + std::to_string(n) + " outside [1, 32]");
    return SUP_EINVAL;
  }
  if (subsets) *subsets = 1ull << n;
  if (est_ops) *est_ops = ltor_ops(n);
  return SUP_OK;
}

int loop_torontonian(const LtorIn& in, int n, uint64_t count, bool range, uint64_t z_begin, uint64_t z_end,
                     const sup_opts& o, bool on_cpu, double* out, TorInfo* info) {
  const std::string who = range ? "sup_loop_torontonian_range" : "sup_loop_torontonian";
  if (!out || !in.O || !in.gamma || !in.modes) {
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
  for (uint64_t k = 0; k < count; ++k)
    for (int j = 0; j < n; ++j) {
      const int32_t v = in.modes[k * n + j];
      if (v < 0 || v >= in.M) {
        set_error(who + ": modes[k = " + std::to_string(k) + "][position " + std::to_string(j) + "] = " +
                  std::to_string(v) + " outside [0, " + std::to_string(in.M) + ")");
        return SUP_EINVAL;
      }
      for (int i = 0; i < j; ++i)
        if (in.modes[k * n + i] == v) {
          set_error(who + ": modes[k = " + std::to_string(k) + "] names mode " + std::to_string(v) + " at positions " +
                    std::to_string(i) + " and " + std::to_string(j) + ": the modes of a list must be distinct");
          return SUP_EINVAL;
        }
    }
  if (range && (z_begin > z_end || z_end > (1ull << n))) {
    set_error(who + ": subsets [" + std::to_string(z_begin) + ", " + std::to_string(z_end) +
              ") outside 0 <= z_begin <= z_end <= 2^" + std::to_string(n));
    return SUP_EINVAL;
  }
  TorInfo ti;
  if (info) *info = ti;
  if (count == 0) return SUP_OK;
  if (!on_cpu && (n > SUP_LOOP_TORONTONIAN_MAX_DEVICE_N || ltor_lds_bytes(n) > 65536)) {
    set_error(who + ": n = " + std::to_string(n) + " above the device cap SUP_LOOP_TORONTONIAN_MAX_DEVICE_N = " +
              std::to_string(SUP_LOOP_TORONTONIAN_MAX_DEVICE_N) + " (on_cpu = 1 serves n <= 32)");
    return SUP_EUNSUPPORTED;
  }
  int G = 1;
  if (!on_cpu) {
    int ndev = 0;
    int rc = device_count(&ndev);
    if (rc) return rc;
    if (ndev == 0) {
      set_error("no HIP device available (" + who + " has no CPU fallback; on_cpu = 1 runs host threads)");
      return SUP_ENODEV;
    }
    if (o.device_id < 0 || o.device_id >= ndev) {
      set_error(who + ": device_id out of range");
      return SUP_EINVAL;
    }
    G = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)std::max(1, std::min(o.gpu_num, ndev - o.device_id)), count));
  }
  const uint64_t z0 = range ? z_begin : 0, z1 = range ? z_end : (1ull << n);
  if (z0 >= z1) {  // no subset: exactly zero, nothing visited
    std::fill(out, out + count, 0.0);
    return SUP_OK;
  }
  ti.subsets = count * (z1 - z0);
  ti.ops = ltor_ops(n);
  const int llog = tor_chunk_log(n), nn = tor_nn(n);
  const uint64_t cfirst = z0 >> llog, cm = ((z1 + (1ull << llog) - 1) >> llog) - cfirst;
  if (on_cpu) {
    // LTOR_TWIN_TAIL = W (tests, read per call): every subset from nothing with
    // the low W positions masked in place, the kernel's form; 0: the compact
    // form without reuse
    const char* tw = std::getenv("LTOR_TWIN_TAIL");
    const int tail = tw ? std::min(std::max(std::atoi(tw), 0), nn) : -1;
    const int T = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)std::max(o.threads, 1), count * cm));
    try {
      std::vector<std::vector<double>> Gs((size_t)count);
      for (uint64_t k = 0; k < count; ++k) ltor_gather(in, in.modes + k * n, n, Gs[(size_t)k]);
      std::vector<double> parts((size_t)(2 * count * cm), 0.0);
      std::atomic<uint64_t> next{0};
      auto work = [&]() {
        LtorState S(nn);
        for (uint64_t a = next.fetch_add(1); a < count * cm; a = next.fetch_add(1))
          parts[(size_t)(2 * a)] = ltor_chunk(Gs[(size_t)(a / cm)].data(), n, nn, tail, cfirst + a % cm, z0, z1, S);
      };
      std::vector<std::thread> th;
      for (int w = 1; w < T; ++w) th.emplace_back(work);
      work();
      for (auto& t : th) t.join();
      for (uint64_t k = 0; k < count; ++k) out[k] = fock_fold(parts.data() + 2 * k * cm, (uint32_t)cm).re;
    } catch (const std::bad_alloc&) {
      set_error("out of host memory for the loop torontonian matrices and partials");
      return SUP_ENOMEM;
    }
    if (info) *info = ti;
    return SUP_OK;
  }
  // lists [a, b) of a device in slabs: as many as keep a slab under
  // kLtorSlabCapBytes and 2^31 chunks (at least one)
  const uint64_t per = 8 * ltor_g_doubles(n) + cm * 16 + (uint64_t)n * 4 + 8;
  const uint64_t slab = std::max<uint64_t>(1, std::min<uint64_t>(kLtorSlabCapBytes / per, 0x7fffffffull / cm));
  std::vector<int> drc(G, SUP_OK), dgrid(G, 0);
  std::vector<double> dms(G, 0.0);
  std::vector<std::string> derr(G);  // g_err is thread_local: carry worker messages back
  auto work = [&](int g) {
    const uint64_t a = count * (uint64_t)g / (uint64_t)G, b = count * (uint64_t)(g + 1) / (uint64_t)G;
    for (uint64_t k = a; k < b && !drc[g]; k += slab) {
      double ms = 0.0;
      drc[g] = run_loop_torontonian(o.device_id + g, in, n, k, std::min(slab, b - k), z0, z1, out + k, &ms, &dgrid[g]);
      if (drc[g]) derr[g] = last_error();
      dms[g] += ms;
    }
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
  ti.kernel_ms = *std::max_element(dms.begin(), dms.end());
  ti.grid = dgrid[0];
  ti.devices = G;
  if (info) *info = ti;
  return SUP_OK;
}

// ---- the ragged batch: sup_loop_torontonian_each ----

static_assert(kTorMaxN <= SUP_LOOP_TORONTONIAN_MAX_DEVICE_N, "every order the ragged entry takes runs on the device");

size_t ltor_item_bytes(int n, int stride) {
  return (size_t)(8 * ltor_g_doubles(n)) + (size_t)ltor_item_chunks(n) * 16 + (size_t)stride * 4 + 8 + sizeof(LtorItem);
}
size_t ltor_slab_cap_bytes() { return kLtorSlabCapBytes; }

namespace {

template <class F>
void ltor_threads(int T, F&& work) {
  std::vector<std::thread> th;
  for (int w = 1; w < T; ++w) th.emplace_back(work);
  work();
  for (auto& t : th) t.join();
}

// The host twin of one slab: every item gathered as loop_torontonian's twin
// gathers it, the queue's slots over the threads (slot chunk0 + c of an item
// is ltor_chunk c of that item alone), then fock_fold over each item's slots.
void ltor_each_cpu(const LtorEachIn& in, const LtorEachSlab& S, int tail_env, int threads, double* out) {
  const uint64_t K = S.items.size();
  std::vector<std::vector<double>> Gs((size_t)K);
  std::vector<double> parts((size_t)(2 * S.chunks), 0.0);
  {
    std::atomic<uint64_t> next{0};
    ltor_threads((int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)threads, K)), [&]() {
      for (uint64_t k = next.fetch_add(1); k < K; k = next.fetch_add(1)) {
        LtorIn li;
        li.O = in.O, li.M = in.M;
        li.gamma = in.gamma + 4ull * (uint64_t)in.M * (S.row_lo + S.items[(size_t)k].row);
        ltor_gather(li, S.modes.data() + k * (uint64_t)S.stride, (int)S.items[(size_t)k].n, Gs[(size_t)k]);
      }
    });
  }
  std::atomic<uint64_t> next{0};
  ltor_threads((int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)threads, S.chunks)), [&]() {
    int have_nn = 0;
    std::vector<LtorState> st;  // one state, rebuilt when the padded order changes
    for (uint64_t a = next.fetch_add(1); a < S.chunks; a = next.fetch_add(1)) {
      const auto it = std::upper_bound(S.items.begin(), S.items.end(), a,
                                       [](uint64_t v, const LtorItem& d) { return v < (uint64_t)d.chunk0; });
      const LtorItem& d = *(it - 1);
      const int n = (int)d.n, nn = (int)d.nn;
      if (nn != have_nn) {
        st.clear();
        st.emplace_back(nn);
        have_nn = nn;
      }
      const int tail = tail_env < 0 ? -1 : std::min(tail_env, nn);
      parts[(size_t)(2 * a)] = ltor_chunk(Gs[(size_t)(&d - S.items.data())].data(), n, nn, tail, a - d.chunk0, 0, 1ull << n, st[0]);
    }
  });
  for (uint64_t k = 0; k < K; ++k)
    out[k] = fock_fold(parts.data() + 2 * (uint64_t)S.items[(size_t)k].chunk0, S.items[(size_t)k].cm).re;
}

}  // namespace

int loop_torontonian_each(const LtorEachIn& in, uint64_t count, const sup_opts& o, bool on_cpu, double* out, TorInfo* info) {
  const std::string who = "sup_loop_torontonian_each";
  if (!out || !in.O || !in.gamma || !in.modes || !in.n) {
    set_error(who + ": null pointer");
    return SUP_EINVAL;
  }
  if (in.M < 1) {
    set_error(who + ": O must have at least two rows (M = " + std::to_string(in.M) + ")");
    return SUP_EINVAL;
  }
  for (uint64_t k = 0; k < count; ++k) {
    const int32_t nk = in.n[k];
    if (nk < 0 || nk > kTorMaxN) {
      set_error(who + ": n[k = " + std::to_string(k) + "] = " + std::to_string(nk) + " outside [0, 32]");
      return SUP_EINVAL;
    }
    if (nk > in.stride) {
      set_error(who + ": stride = " + std::to_string(in.stride) + " < n[k = " + std::to_string(k) + "] = " + std::to_string(nk));
      return SUP_EINVAL;
    }
    const int64_t row = in.gamma_of ? (int64_t)in.gamma_of[k] : (int64_t)k;
    if (row < 0 || (uint64_t)row >= in.ngamma) {
      set_error(who + ": gamma_of[k = " + std::to_string(k) + "] = " + std::to_string(row) + " outside [0, " +
                std::to_string(in.ngamma) + ")");
      return SUP_EINVAL;
    }
    const int32_t* s = in.modes + k * (uint64_t)in.stride;
    for (int j = 0; j < nk; ++j) {
      if (s[j] < 0 || s[j] >= in.M) {
        set_error(who + ": modes[k = " + std::to_string(k) + "][position " + std::to_string(j) + "] = " +
                  std::to_string(s[j]) + " outside [0, " + std::to_string(in.M) + ")");
        return SUP_EINVAL;
      }
      for (int i = 0; i < j; ++i)
        if (s[i] == s[j]) {
          set_error(who + ": modes[k = " + std::to_string(k) + "] names mode " + std::to_string(s[j]) + " at positions " +
                    std::to_string(i) + " and " + std::to_string(j) + ": the modes of a list must be distinct");
          return SUP_EINVAL;
        }
    }
  }
  // SUP_LTOR_EACH_SLAB (tests, read per call): items per slab at most
  uint64_t slab_max = ~0ull;
  if (const char* e = std::getenv("SUP_LTOR_EACH_SLAB")) {
    char* end = nullptr;
    const long long v = std::strtoll(e, &end, 10);
    if (end == e || *end != '\0' || v < 1) {
      set_error(who + ": SUP_LTOR_EACH_SLAB = \"" + std::string(e) + "\" is not a positive count of items");
      return SUP_EINVAL;
    }
    slab_max = (uint64_t)v;
  }
  TorInfo ti;
  if (info) *info = ti;
  int G = 1;
  if (!on_cpu) {
    int ndev = 0;
    int rc = device_count(&ndev);
    if (rc) return rc;
    if (ndev == 0) {
      set_error("no HIP device available (" + who + " has no CPU fallback; on_cpu = 1 runs host threads)");
      return SUP_ENODEV;
    }
    if (o.device_id < 0 || o.device_id >= ndev) {
      set_error(who + ": device_id out of range");
      return SUP_EINVAL;
    }
    G = std::max(1, std::min(o.gpu_num, ndev - o.device_id));
  }
  try {
    // the items that walk: an item of order 0 is the empty list's f(0) = 1
    std::vector<uint64_t> live;
    double ops_of[kTorMaxN + 1], ops_sum = 0.0;
    for (int n = 0; n <= kTorMaxN; ++n) ops_of[n] = -1.0;
    for (uint64_t k = 0; k < count; ++k) {
      const int n = in.n[k];
      if (n == 0) {
        out[k] = 1.0;
        continue;
      }
      live.push_back(k);
      if (ops_of[n] < 0.0) ops_of[n] = ltor_ops(n);
      ti.subsets += 1ull << n;
      ops_sum += (double)(1ull << n) * ops_of[n];
    }
    const uint64_t L = live.size();
    if (L == 0) return SUP_OK;
    ti.ops = ops_sum / (double)ti.subsets;
    G = (int)std::min<uint64_t>((uint64_t)G, L);
    const char* tw = std::getenv("LTOR_TWIN_TAIL");  // as loop_torontonian's twin
    const int tail = tw ? std::max(std::atoi(tw), 0) : -1;
    std::vector<int> drc(G, SUP_OK), dgrid(G, 0);
    std::vector<double> dms(G, 0.0);
    std::vector<std::string> derr(G);
    // live items [a, b) of a device in slabs under the caps; orders mix freely
    auto work = [&](int g) {
      const uint64_t a = L * (uint64_t)g / (uint64_t)G, b = L * (uint64_t)(g + 1) / (uint64_t)G;
      try {
        std::vector<double> res;
        for (uint64_t i = a; i < b && !drc[g];) {
          LtorEachSlab S;
          S.stride = in.stride;
          size_t bytes = 0;
          const uint64_t i0 = i;
          uint64_t lo = ~0ull, hi = 0;
          for (; i < b && i - i0 < slab_max; ++i) {
            const uint64_t k = live[i];
            const int n = in.n[k];
            const size_t add = ltor_item_bytes(n, in.stride);
            const uint64_t cm = ltor_item_chunks(n);
            if (i > i0 && (bytes + add > kLtorSlabCapBytes || S.chunks + cm > 0x7fffffffull)) break;
            LtorItem d{};
            d.g_off = S.g_doubles, d.chunk0 = (unsigned)S.chunks, d.cm = (unsigned)cm;
            d.n = (unsigned)n, d.nn = (unsigned)tor_nn(n), d.llog = (unsigned)tor_chunk_log(n);
            const uint64_t row = in.gamma_of ? (uint64_t)in.gamma_of[k] : k;
            lo = std::min(lo, row), hi = std::max(hi, row);
            S.items.push_back(d);
            S.modes.resize(S.modes.size() + (size_t)in.stride, 0);  // the entries past n[k] are not read
            std::copy(in.modes + k * (uint64_t)in.stride, in.modes + k * (uint64_t)in.stride + n, S.modes.end() - in.stride);
            S.g_doubles += ltor_g_doubles(n), S.chunks += cm, S.max_n = std::max(S.max_n, n);
            bytes += add;
          }
          // the device takes rows [lo, hi] of gamma alone
          S.row_lo = lo, S.rows = hi - lo + 1;
          for (uint64_t q = i0; q < i; ++q)
            S.items[(size_t)(q - i0)].row = (unsigned)((in.gamma_of ? (uint64_t)in.gamma_of[live[q]] : live[q]) - lo);
          res.assign((size_t)(i - i0), 0.0);
          if (on_cpu) {
            ltor_each_cpu(in, S, tail, std::max(o.threads, 1), res.data());
          } else {
            double ms = 0.0;
            drc[g] = run_loop_torontonian_each(o.device_id + g, in, S, res.data(), &ms, &dgrid[g]);
            if (drc[g]) derr[g] = last_error();
            dms[g] += ms;
          }
          if (!drc[g])
            for (uint64_t q = i0; q < i; ++q) out[live[q]] = res[(size_t)(q - i0)];
        }
      } catch (const std::bad_alloc&) {
        derr[g] = "out of host memory for a slab's matrices and partials";
        drc[g] = SUP_ENOMEM;
      }
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
    if (!on_cpu) {
      ti.kernel_ms = *std::max_element(dms.begin(), dms.end());
      ti.grid = dgrid[0];
      ti.devices = G;
    }
  } catch (const std::bad_alloc&) {
    set_error(who + ": out of host memory for the items' lists");
    return SUP_ENOMEM;
  }
  if (info) *info = ti;
  return SUP_OK;
}

}  // namespace sup
