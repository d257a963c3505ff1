// torontonian.cpp — torontonians of complex Hermitian matrices gathered by
// lists of distinct modes: sup_torontonian, sup_torontonian_range and
// sup_torontonian_plan.
//
// The sum runs over the 2^n subsets z of a list's positions (tor.hpp).  The
// checks, the chunking and the host twin are here.  The twin keeps the compact
// factor of the current subset and, stepping z upwards, recomputes only the
// rows at and below the highest position that changed; tor.hpp says why that,
// and the kernel's masked tail, give the same bits.  Result k is a function of
// (O, modes[k]) only.
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "cx.hpp"
#include "engine.hpp"
#include "tor.hpp"
#include "torontonian.hpp"

namespace sup {

namespace {

constexpr size_t kTorSlabCapBytes = (size_t)256 << 20;

// The 64-lane xor butterfly (walk_tor.hip tor_wave_sum) on v[0..63].
double tor_butterfly(double* v) {
  for (int off = 1; off <= 32; off <<= 1) {
    double w[64];
    for (int l = 0; l < 64; ++l) w[l] = v[l] + v[l ^ off];
    std::copy(w, w + 64, v);
  }
  return v[0];
}

// The compact factor of one subset, kept between subsets.
struct TorState {
  int N = 0;               // row stride of G and L
  std::vector<cx> L;       // compact rows, N pairs each
  std::vector<double> rho, prod;
  std::vector<int> row;    // full index of compact row i
  uint64_t zprev = 0;
  bool have = false;
  explicit TorState(int nn) : N(2 * nn), L((size_t)N * N), rho(N), prod(N + 1), row(N) { prod[0] = 1.0; }
};

// Row i of the factor from rows < i (tor.hpp's chains).  sel: the row is
// selected; an unselected one is an identity row.  selv (or null: every row
// above is selected): which of the rows above are; the columns of the others
// are +0.
void tor_row(const double* G, TorState& S, int i, bool sel, const char* selv = nullptr) {
  cx* Li = S.L.data() + (size_t)i * S.N;
  if (!sel) {
    for (int c = 0; c < i; ++c) Li[c] = cx{0.0, 0.0};
    S.rho[i] = 1.0;
    S.prod[i + 1] = S.prod[i] * S.rho[i];
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
}

// f(z), compact form, reusing the rows the previous subset shares.
double tor_f(const double* G, int nn, TorState& S, uint64_t z) {
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
  for (int i = keep; i < P; ++i) tor_row(G, S, i, true);
  S.zprev = z, S.have = true;
  return S.prod[P];
}

// f(z) from nothing, the positions below `tail` kept in place as identity rows
// where z does not select them (the kernel's form with W = tail; tail = 0: the
// compact form without reuse).
double tor_f_masked(const double* G, int n, int nn, TorState& S, uint64_t z, int tail) {
  int P = 0;
  std::vector<char> sel((size_t)S.N, 1);
  for (int b = nn - 1; b >= 0; --b) {
    const bool on = (z >> b) & 1ull;
    if (!on && (b >= tail || b >= n)) continue;
    S.row[P] = 2 * (nn - 1 - b), S.row[P + 1] = 2 * (nn - 1 - b) + 1;
    sel[P] = sel[P + 1] = on;
    P += 2;
  }
  for (int i = 0; i < P; ++i) tor_row(G, S, i, sel[i], sel.data());
  S.have = false;
  return S.prod[P];
}

// The partial of wave-chunk c (tor.hpp): its 64-aligned groups ascending from
// +0, z outside [z0, z1) as +0.
double tor_chunk(const double* G, int n, int nn, int tail, uint64_t c, uint64_t z0, uint64_t z1, TorState& S) {
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
      const double f = tail < 0 ? tor_f(G, nn, S, z) : tor_f_masked(G, n, nn, S, z, tail);
      v[l] = ((n - __builtin_popcountll(z)) & 1) ? -f : f;
    }
    acc = acc + tor_butterfly(v);
  }
  return acc;
}

void tor_gather(const TorIn& in, const int32_t* s, int n, std::vector<double>& G) {
  const int N = 2 * tor_nn(n);
  G.resize((size_t)2 * N * N);
  for (int R = 0; R < N; ++R)
    for (int C = 0; C < N; ++C) {
      const cx v = tor_entry(in.O, in.M, s, n, R, C);
      G[2 * ((size_t)R * N + C)] = v.re, G[2 * ((size_t)R * N + C) + 1] = v.im;
    }
}

}  // namespace

// The raw table of one list (tortab.hpp): out[z] = f(z) for every z in [0,
// 2^n), runs of 2^9 consecutive z over the threads, each from nothing and then
// with the rows the previous subset shares (the bits do not depend on the cut).
void tor_table_raw_cpu(const TorIn& in, int n, int threads, double* out) {
  const int nn = tor_nn(n);
  std::vector<double> G;
  tor_gather(in, in.modes, n, G);
  const uint64_t total = 1ull << n, run = std::min<uint64_t>(total, 512), runs = total / run;
  const int T = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)std::max(threads, 1), runs));
  std::atomic<uint64_t> next{0};
  auto work = [&]() {
    TorState S(nn);
    for (uint64_t a = next.fetch_add(1); a < runs; a = next.fetch_add(1)) {
      S.have = false;
      for (uint64_t z = a * run; z < (a + 1) * run; ++z) out[z] = tor_f(G.data(), nn, S, z);
    }
  };
  std::vector<std::thread> th;
  for (int w = 1; w < T; ++w) th.emplace_back(work);
  work();
  for (auto& t : th) t.join();
}

int torontonian_plan(int n, uint64_t* subsets, double* est_ops) {
  if (n < 1 || n > kTorMaxN) {
    set_error("sup_torontonian_plan: n = " + std::to_string(n) + " outside [1, 32]");
    return SUP_EINVAL;
  }
  if (subsets) *subsets = 1ull << n;
  if (est_ops) *est_ops = tor_ops(n);
  return SUP_OK;
}

int torontonian(const TorIn& in, int n, uint64_t count, bool range, uint64_t z_begin, uint64_t z_end,
                const sup_opts& o, bool on_cpu, double* out, TorInfo* info) {
  const std::string who = range ? "sup_torontonian_range" : "sup_torontonian";
  if (!out || !in.O || !in.modes) {
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
  if (!on_cpu && n > SUP_TORONTONIAN_MAX_DEVICE_N) {
    set_error(who + ": n = " + std::to_string(n) + " above the device cap SUP_TORONTONIAN_MAX_DEVICE_N = " +
              std::to_string(SUP_TORONTONIAN_MAX_DEVICE_N) + " (on_cpu = 1 serves n <= 32)");
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
  ti.ops = tor_ops(n);
  const int llog = tor_chunk_log(n), nn = tor_nn(n);
  const uint64_t cfirst = z0 >> llog, cm = ((z1 + (1ull << llog) - 1) >> llog) - cfirst;
  if (on_cpu) {
    // TOR_TWIN_TAIL = W (tests, read per call): every subset from nothing with
    // the low W positions masked in place, the kernel's form; 0: the compact
    // form without reuse
    const char* tw = std::getenv("TOR_TWIN_TAIL");
    const int tail = tw ? std::min(std::max(std::atoi(tw), 0), nn) : -1;
    const int T = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)std::max(o.threads, 1), count * cm));
    try {
      std::vector<std::vector<double>> Gs((size_t)count);
      for (uint64_t k = 0; k < count; ++k) tor_gather(in, in.modes + k * n, n, Gs[(size_t)k]);
      std::vector<double> parts((size_t)(2 * count * cm), 0.0);
      std::atomic<uint64_t> next{0};
      auto work = [&]() {
        TorState S(nn);
        for (uint64_t a = next.fetch_add(1); a < count * cm; a = next.fetch_add(1))
          parts[(size_t)(2 * a)] = tor_chunk(Gs[(size_t)(a / cm)].data(), n, nn, tail, cfirst + a % cm, z0, z1, S);
      };
      std::vector<std::thread> th;
      for (int w = 1; w < T; ++w) th.emplace_back(work);
      work();
      for (auto& t : th) t.join();
      for (uint64_t k = 0; k < count; ++k) out[k] = fock_fold(parts.data() + 2 * k * cm, (uint32_t)cm).re;
    } catch (const std::bad_alloc&) {
      set_error("out of host memory for the torontonian matrices and partials");
      return SUP_ENOMEM;
    }
    if (info) *info = ti;
    return SUP_OK;
  }
  // lists [a, b) of a device in slabs: as many as keep a slab under
  // kTorSlabCapBytes and 2^31 chunks (at least one)
  const uint64_t per = 8 * tor_g_doubles(n) + cm * 16 + (uint64_t)n * 4 + 8;
  const uint64_t slab = std::max<uint64_t>(1, std::min<uint64_t>(kTorSlabCapBytes / per, 0x7fffffffull / cm));
  std::vector<int> drc(G, SUP_OK), dgrid(G, 0);
  std::vector<double> dms(G, 0.0);
  std::vector<std::string> derr(G);  // g_err is thread_local: carry worker messages back
  auto work = [&](int g) {
    const uint64_t a = count * (uint64_t)g / (uint64_t)G, b = count * (uint64_t)(g + 1) / (uint64_t)G;
    for (uint64_t k = a; k < b && !drc[g]; k += slab) {
      double ms = 0.0;
      drc[g] = run_torontonian(o.device_id + g, in, n, k, std::min(slab, b - k), z0, z1, out + k, &ms, &dgrid[g]);
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

}  // namespace sup
