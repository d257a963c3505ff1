// hafnian.cpp — hafnians and loop hafnians of complex symmetric matrices
// gathered by index lists that may repeat: sup_hafnian_complex,
// sup_loop_hafnian_complex and sup_hafnian_complex_plan.
//
// Matrix k is A[idx_i][idx_j].  Its sum (haf.hpp) runs over the multiplicity
// vectors of the K distinct values of idx; the grouping and the layout (digits,
// walk digits, Tw, H) are cplx_fock.cpp's fock_group_of and fock_layout, a pure
// function of the multiplicity vector.  Per matrix the builder below writes
// what walk_haf.hip reads, and the host twin reads the same arrays, running the
// same operations in the same order: chunk partials, fock_fold per matrix,
// (2 x the sum) / m!.  Result k is a function of (A, mu, idx[k]) only.
//
// sup_loop_hafnian_complex_each (loop_hafnian_each below) builds
// the same slabs from items whose orders and displacement rows differ: the
// order and the coefficient row travel per matrix in HafMat::ord, the row of mu
// per matrix in HafSlab::mu_row, and walk_lhafe.hip and the host twin read them
// there.  Item k is a function of (A, its row of mu, its list) only, with the
// bits of sup_loop_hafnian_complex on it alone.
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <map>
#include <new>
#include <string>
#include <thread>

#include "cplx_fock_build.hpp"
#include "cx.hpp"
#include "engine.hpp"
#include "haf.hpp"

namespace sup {

namespace {

constexpr size_t kHafSlabCapBytes = (size_t)256 << 20;

inline uint32_t wt_row(int t) { return (uint32_t)(t * (t + 1) / 2); }

using HafProgs = std::map<std::vector<uint32_t>, uint32_t>;

struct HafChoice {
  FockGroups g;
  FockLayout lay;
};

HafChoice haf_choose(const int32_t* idx, int n) {
  HafChoice c;
  c.g = fock_group_of(idx, n);
  c.lay = fock_layout(c.g);
  return c;
}

// Bytes a matrix adds to a slab (table, partials of partial_bytes per
// wave-chunk, descriptors).
size_t haf_bytes(const HafChoice& c, size_t partial_bytes) {
  const size_t chunks = (size_t)((c.lay.H + 63) / 64);
  return (size_t)haf_pairs(c.lay.nwalk, c.lay.nd - c.lay.nwalk) * 16 + chunks * (sizeof(FockChunk) + partial_bytes) +
         (size_t)c.lay.nd * (sizeof(HafDigit) + 4) + (size_t)c.g.K * 8 + sizeof(HafMat) + 80;
}

// The step program of a walk-digit radix list: the reflected mixed-radix Gray
// order of cplx_fock.cpp's fock_append_desc; entry t names the digit that
// moves, its direction and the weight of the state reached.
uint32_t haf_program(HafSlab& S, const FockLayout& l, HafProgs& progs) {
  const std::vector<double>& wts = fock_weights();
  std::vector<uint32_t> key(l.radix, l.radix + l.nwalk);
  auto it = progs.find(key);
  if (it != progs.end()) return it->second;
  const uint32_t base = (uint32_t)S.prog.size();
  uint32_t a[SUP_MAX_N] = {0}, g[SUP_MAX_N] = {0};
  bool odd[SUP_MAX_N] = {false};
  for (uint32_t tt = 0; tt < l.Tw; ++tt) {
    HafStep s{0u, 0u, 1.0};
    if (tt > 0) {
      int c = 0;
      while (a[c] == l.radix[c] - 1u) a[c] = 0, odd[c] = !odd[c], ++c;
      ++a[c];
      for (int i = 0; i <= c; ++i) {
        const uint32_t v = odd[i] ? l.radix[i] - 1u - a[i] : a[i];
        if (v != g[i]) {  // v up: delta = +1 (row 2 i), v down: row 2 i + 1
          s.dsg = (uint32_t)(2 * i + (v > g[i] ? 0 : 1));
          s.row = (uint32_t)(16 * (kHafStart + (int)s.dsg * kHafRow));
        }
        g[i] = v;
      }
    }
    for (int i = 0; i < l.nwalk; ++i) s.w = s.w * wts[wt_row((int)l.radix[i] - 1) + g[i]];
    S.prog.push_back(s);
  }
  S.prog.push_back(HafStep{(uint32_t)(16 * kHafStart), 0u, 0.0});  // padding: the walk asks for entry t + 1 ahead
  progs.emplace(std::move(key), base);
  return base;
}

// Appends the matrix with groups and layout c to S.  host_tables: write the
// table here (the host twin) with displacement mu (null: the plain hafnian);
// the device path leaves it to haf_prepare.  ord: HafMat::ord.
void haf_append(HafSlab& S, const HafIn& in, const HafChoice& c, HafProgs& progs, bool host_tables, const double* mu,
                uint32_t ord) {
  const FockLayout& l = c.lay;
  HafMat M{};
  M.tab = S.tab_doubles;
  M.prog = haf_program(S, l, progs);
  M.Tw = l.Tw;
  M.W = (uint32_t)l.nwalk;
  M.ndig = (uint32_t)(l.nd - l.nwalk);
  M.H = (uint32_t)l.H;
  M.K = (uint32_t)c.g.K;
  M.pairs = haf_pairs(l.nwalk, l.nd - l.nwalk);
  M.ord = ord;
  M.grp = (uint32_t)S.grp.size();
  for (int k = 0; k < c.g.K; ++k) S.grp.push_back(c.g.val[k]), S.grp.push_back(c.g.mult[k]);
  for (int d = 0; d < l.nd; ++d) S.grp.push_back(l.col[d]);
  M.dig = (uint32_t)S.dig.size();
  for (int d = l.nwalk; d < l.nd; ++d) S.dig.push_back(HafDigit{l.radix[d], wt_row((int)l.radix[d] - 1)});
  M.chunk0 = (uint32_t)S.chunks.size();
  M.chunks = (uint32_t)((l.H + 63) / 64);
  const uint32_t mi = (uint32_t)S.mats.size();
  for (uint32_t ci = 0; ci < M.chunks; ++ci) S.chunks.push_back(FockChunk{mi, ci});
  // tables start on 64 bytes: the walk reads step rows in 64-byte pieces
  S.tab_doubles += (2 * (uint64_t)M.pairs + 7) / 8 * 8;
  if (host_tables) {
    S.tabs.resize(S.tab_doubles, 0.0);
    double* t = S.tabs.data() + M.tab;
    const int32_t* g = S.grp.data() + M.grp;
    for (uint32_t e = 0; e < M.pairs; ++e) {
      const cx v = haf_entry(in.A, in.M, mu, g, (int)M.K, (int)M.W, (int)M.ndig, e);
      t[2 * (size_t)e] = v.re, t[2 * (size_t)e + 1] = v.im;
    }
  }
  S.mats.push_back(M);
}

inline cx fma_cx(double s, cx b, cx x) { return cx{__builtin_fma(s, b.re, x.re), __builtin_fma(s, b.im, x.im)}; }

// One wave-chunk of the slab's queue, every lane, then the 64-lane xor
// butterfly (walk_haf.hip's order).
cx haf_chunk(const HafSlab& S, uint64_t a) {
  const FockChunk ck = S.chunks[a];
  const HafMat& M = S.mats[ck.mat];
  const std::vector<double>& wts = fock_weights();
  const double* tab = S.tabs.data() + M.tab;
  auto ld = [&](size_t pair) { return cx{tab[2 * pair], tab[2 * pair + 1]}; };
  const HafStep* prog = S.prog.data() + M.prog;
  // a ragged slab's matrix carries its own order and coefficient row
  const uint32_t n = S.each ? M.ord & 0xffu : (uint32_t)S.n, m = n >> 1;
  const double* coef = S.coef.data() + (M.ord >> 8);
  const size_t hs = (size_t)kHafHigh + M.ndig, high0 = (size_t)kHafStart + 2 * (size_t)M.W * kHafRow;
  const int ge = M.W > 4u ? kHafWalkDigits : 4;  // the G entries the walk updates
  auto term = [&](cx Q, cx r) { return S.loop ? haf_loop_poly(Q, r, coef, n) : haf_pow(Q, m); };
  cx v[64];
  for (uint32_t lane = 0; lane < 64; ++lane) {
    const uint32_t h = 64u * ck.local + lane;
    if (h >= M.H) {  // the device walks such a lane at h = 0 and drops its value
      v[lane] = cx{0.0, 0.0};
      continue;
    }
    cx Q = ld(0), r = ld(1), G[kHafWalkDigits];
    for (int e = 0; e < kHafWalkDigits; ++e) G[e] = ld(2 + (size_t)e);
    double dv[kHafHighDigits];
    uint32_t rem = h;
    double hw = 1.0;
    for (uint32_t d = 0; d < M.ndig; ++d) {
      const HafDigit& D = S.dig[M.dig + d];
      const uint32_t qd = rem / D.radix, vd = rem - qd * D.radix;
      rem = qd;
      hw = hw * wts[D.wt_off + vd];
      const double dvd = -(double)vd;
      const size_t row = high0 + d * hs;
      cx t = ld(row);
      for (uint32_t e = 0; e < d; ++e) t = fma_cx(dv[e], ld(row + kHafHigh + e), t);
      const double d2 = dvd + dvd, dd = dvd * dvd;
      Q = fma_cx(d2, t, Q);
      Q = fma_cx(dd, ld(row + 1), Q);
      if (S.loop) r = fma_cx(dvd, ld(row + 2), r);
      for (int e = 0; e < ge; ++e) G[e] = fma_cx(dvd, ld(row + 3 + (size_t)e), G[e]);
      dv[d] = dvd;
    }
    cx acc = term(Q, r);
    for (uint32_t t = 1; t < M.Tw; ++t) {
      const size_t row = prog[t].row / 16;
      const double m2 = (prog[t].dsg & 1u) ? 2.0 : -2.0;
      Q = fma_cx(m2, G[prog[t].dsg >> 1], Q);
      Q = cx_add(Q, ld(row + kHafWalkDigits));
      for (int e = 0; e < ge; ++e) G[e] = cx_add(G[e], ld(row + (size_t)e));
      if (S.loop) r = cx_add(r, ld(row + kHafWalkDigits + 1));
      const cx tm = term(Q, r);
      const double mr = prog[t].w * tm.re, mi = prog[t].w * tm.im;
      acc = cx{acc.re + mr, acc.im + mi};
    }
    v[lane] = cx{acc.re * hw, acc.im * hw};
  }
  for (int off = 1; off <= 32; off <<= 1) {
    cx w[64];
    for (int l = 0; l < 64; ++l) w[l] = cx_add(v[l], v[l ^ off]);
    std::copy(w, w + 64, v);
  }
  return v[0];
}

// The host twin on a slab: `threads` threads share the queue's chunks, then
// each matrix's partials are folded.
void haf_cpu(const HafSlab& S, int threads, double* out) {
  const uint64_t count = S.chunks.size();
  std::vector<double> parts(2 * (size_t)count, 0.0);
  const int nt = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)std::max(threads, 1), count));
  auto work = [&](int w) {
    for (uint64_t a = (uint64_t)w; a < count; a += (uint64_t)nt) {
      const cx v = haf_chunk(S, a);
      parts[2 * a] = v.re, parts[2 * a + 1] = v.im;
    }
  };
  std::vector<std::thread> th;
  for (int w = 1; w < nt; ++w) th.emplace_back(work, w);
  work(0);
  for (auto& t : th) t.join();
  for (size_t k = 0; k < S.mats.size(); ++k) {
    const cx v = fock_fold(parts.data() + 2 * (size_t)S.mats[k].chunk0, S.mats[k].chunks);
    out[2 * k] = (2.0 * v.re) / S.div;
    out[2 * k + 1] = (2.0 * v.im) / S.div;
  }
}

}  // namespace

uint64_t haf_fill_slab(HafSlab& S, const HafIn& in, int n, uint64_t k, uint64_t kend, uint64_t slab_max,
                       size_t partial_bytes, bool host_tables) {
  HafProgs progs;
  size_t bytes = 0;
  const uint64_t k0 = k;
  for (; k < kend && k - k0 < slab_max; ++k) {
    const HafChoice c = haf_choose(in.idx + k * n, n);
    const size_t add = haf_bytes(c, partial_bytes);
    const uint64_t chunks = (c.lay.H + 63) / 64;
    if (k > k0 && (bytes + add > kHafSlabCapBytes || S.chunks.size() + chunks > 0x7fffffffull)) break;
    haf_append(S, in, c, progs, host_tables, in.loop ? in.mu : nullptr, 0u);
    bytes += add;
  }
  return k;
}

int hafnian_plan(const int32_t* idx, int n, uint64_t count, uint64_t* terms) {
  if (!idx) {
    set_error("sup_hafnian_complex_plan: null index list");
    return SUP_EINVAL;
  }
  if (n < 1 || n > SUP_MAX_N) {
    set_error("n = " + std::to_string(n) + " outside [1, 64] (64-bit Gray index)");
    return SUP_EINVAL;
  }
  for (uint64_t k = 0; k < count; ++k)
    if (terms) terms[k] = haf_choose(idx + k * n, n).lay.T;
  return SUP_OK;
}

int haf_check_request(const HafIn& in, int n, uint64_t count, const std::string& who) {
  if (n < 1 || n > SUP_MAX_N) {
    set_error("n = " + std::to_string(n) + " outside [1, 64] (64-bit Gray index)");
    return SUP_EINVAL;
  }
  if (in.M < 1) {
    set_error(who + ": A must have at least one row (M = " + std::to_string(in.M) + ")");
    return SUP_EINVAL;
  }
  for (int i = 0; i < in.M; ++i)
    for (int j = 0; j < i; ++j)
      if (std::memcmp(in.A + 2 * ((size_t)i * in.M + j), in.A + 2 * ((size_t)j * in.M + i), 2 * sizeof(double)) != 0) {
        set_error(who + ": A[" + std::to_string(j) + "][" + std::to_string(i) + "] and A[" + std::to_string(i) + "][" +
                  std::to_string(j) + "] differ: A must be symmetric bit for bit");
        return SUP_EINVAL;
      }
  for (uint64_t k = 0; k < count; ++k)
    for (int j = 0; j < n; ++j) {
      const int32_t v = in.idx[k * n + j];
      if (v < 0 || v >= in.M) {
        set_error(who + ": idx[k = " + std::to_string(k) + "][position " + std::to_string(j) + "] = " +
                  std::to_string(v) + " outside [0, " + std::to_string(in.M) + ")");
        return SUP_EINVAL;
      }
    }
  return SUP_OK;
}

int hafnian_complex(const HafIn& in, int n, uint64_t count, const sup_opts& o, bool on_cpu, double* out,
                    HafInfo* info) {
  const std::string who = in.loop ? "sup_loop_hafnian_complex" : "sup_hafnian_complex";
  if (!out || !in.A || !in.idx || (in.loop && !in.mu)) {
    set_error(who + ": null pointer");
    return SUP_EINVAL;
  }
  if (int rc = haf_check_request(in, n, count, who)) return rc;
  HafInfo hi;
  if (info) *info = hi;
  if (count == 0) return SUP_OK;
  if (!in.loop && (n & 1)) {  // no perfect matching: exactly zero, nothing walked
    std::fill(out, out + 2 * count, 0.0);
    return SUP_OK;
  }
  // every matrix's terms before any work (planned on o.threads host threads):
  // the sums for the stats, and the cap
  const int T = std::max(o.threads, 1);
  {
    std::vector<uint64_t> sum(T, 0), bad(T, ~0ull);
    std::vector<double> ops(T, 0.0);
    std::atomic<int> next{0};
    fock_parallel(count, T, [&](uint64_t a, uint64_t b) {
      const int w = next.fetch_add(1);
      for (uint64_t k = a; k < b; ++k) {
        const HafChoice c = haf_choose(in.idx + k * n, n);
        if ((c.lay.H + 63) / 64 > kFockMaxChunks) bad[w] = std::min(bad[w], k);
        sum[w] += c.lay.T;
        ops[w] += (double)c.lay.T * haf_ops(c.lay.nwalk, n, in.loop);
      }
    });
    const uint64_t k = *std::min_element(bad.begin(), bad.end());
    if (k != ~0ull) {
      const HafChoice c = haf_choose(in.idx + k * n, n);
      set_error(who + ": matrix k = " + std::to_string(k) + " has " + std::to_string(c.lay.T) +
                " terms, more than 2^40 (2^24 wave-chunks of 64 lanes x 2^10 steps)");
      return SUP_EUNSUPPORTED;
    }
    double osum = 0.0;
    for (int w = 0; w < T; ++w) hi.terms += sum[w], osum += ops[w];
    hi.ops = hi.terms ? osum / (double)hi.terms : 0.0;
  }
  uint64_t slab_max = ~0ull;
  if (const char* e = std::getenv("SUP_HAFNIAN_SLAB")) {
    const long long v = std::atoll(e);
    if (v > 0) slab_max = (uint64_t)v;
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
  // n!: exact in a double up to 22!, correctly ordered products above
  double fact[SUP_MAX_N + 1];
  fact[0] = 1.0;
  for (int i = 1; i <= n; ++i) fact[i] = fact[i - 1] * (double)i;
  std::vector<double> coef;
  if (in.loop)
    for (int j = 0; j <= n / 2; ++j) coef.push_back(1.0 / (fact[j] * fact[n - 2 * j]));
  std::vector<int> drc(G, SUP_OK), dgrid(G, 0);
  std::vector<double> dms(G, 0.0);
  std::vector<std::string> derr(G);  // g_err is thread_local: carry worker messages back
  // matrices [a, b) in slabs: as many as keep a slab under kHafSlabCapBytes
  // and 2^31 chunks (at least one), or SUP_HAFNIAN_SLAB
  auto work = [&](int g) {
    const uint64_t a = count * (uint64_t)g / (uint64_t)G, b = count * (uint64_t)(g + 1) / (uint64_t)G;
    try {
      for (uint64_t k = a; k < b && !drc[g];) {
        HafSlab S;
        S.n = n;
        S.loop = in.loop;
        S.coef = coef;
        S.div = in.loop ? 1.0 : fact[n / 2];
        const uint64_t k0 = k;
        k = haf_fill_slab(S, in, n, k, b, slab_max, 16, on_cpu);
        if (on_cpu) {
          haf_cpu(S, std::max(o.threads, 1), out + 2 * k0);
        } else {
          double ms = 0.0;
          drc[g] = run_hafnian(o.device_id + g, S, in, out + 2 * k0, &ms, &dgrid[g]);
          if (drc[g]) derr[g] = last_error();
          dms[g] += ms;
        }
      }
    } catch (const std::bad_alloc&) {
      derr[g] = "out of host memory for a slab's tables and partials";
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
    hi.kernel_ms = *std::max_element(dms.begin(), dms.end());
    hi.grid = dgrid[0];
    hi.devices = G;
  }
  if (info) *info = hi;
  return SUP_OK;
}

// ---- the ragged batch: sup_loop_hafnian_complex_each ----

size_t haf_item_bytes(const int32_t* idx, int n) { return haf_bytes(haf_choose(idx, n), 16); }
size_t haf_slab_cap_bytes() { return kHafSlabCapBytes; }

int loop_hafnian_each(const HafEachIn& in, uint64_t count, const sup_opts& o, bool on_cpu, double* out, HafInfo* info) {
  const std::string who = "sup_loop_hafnian_complex_each";
  if (!out || !in.A || !in.mu || !in.idx || !in.n) {
    set_error(who + ": null pointer");
    return SUP_EINVAL;
  }
  HafIn hin;
  hin.A = in.A, hin.M = in.M, hin.mu = in.mu, hin.idx = in.idx, hin.loop = true;
  if (int rc = haf_check_request(hin, 1, 0, who)) return rc;  // M and the symmetry of A: no list is read
  for (uint64_t k = 0; k < count; ++k) {
    const int32_t nk = in.n[k];
    if (nk < 0 || nk > SUP_MAX_N) {
      set_error(who + ": n[k = " + std::to_string(k) + "] = " + std::to_string(nk) + " outside [0, 64]");
      return SUP_EINVAL;
    }
    if (nk > in.stride) {
      set_error(who + ": stride = " + std::to_string(in.stride) + " < n[k = " + std::to_string(k) + "] = " +
                std::to_string(nk));
      return SUP_EINVAL;
    }
    const int64_t row = in.mu_of ? (int64_t)in.mu_of[k] : (int64_t)k;
    if (row < 0 || (uint64_t)row >= in.nmu) {
      set_error(who + ": mu_of[k = " + std::to_string(k) + "] = " + std::to_string(row) + " outside [0, " +
                std::to_string(in.nmu) + ")");
      return SUP_EINVAL;
    }
    for (int j = 0; j < nk; ++j) {
      const int32_t v = in.idx[k * (uint64_t)in.stride + j];
      if (v < 0 || v >= in.M) {
        set_error(who + ": idx[k = " + std::to_string(k) + "][position " + std::to_string(j) + "] = " +
                  std::to_string(v) + " outside [0, " + std::to_string(in.M) + ")");
        return SUP_EINVAL;
      }
    }
  }
  HafInfo hi;
  if (info) *info = hi;
  // the items that walk: an item of order 0 is the empty product
  std::vector<uint64_t> live;
  for (uint64_t k = 0; k < count; ++k) {
    if (in.n[k] > 0) live.push_back(k);
    else out[2 * k] = 1.0, out[2 * k + 1] = 0.0;
  }
  const uint64_t L = live.size();
  if (L == 0) return SUP_OK;
  auto list_of = [&](uint64_t k) { return in.idx + k * (uint64_t)in.stride; };
  auto row_of = [&](uint64_t k) { return in.mu_of ? (int64_t)in.mu_of[k] : (int64_t)k; };
  // every item's terms before any work, as hafnian_complex plans them
  const int T = std::max(o.threads, 1);
  {
    std::vector<uint64_t> sum(T, 0), bad(T, ~0ull);
    std::vector<double> ops(T, 0.0);
    std::atomic<int> next{0};
    fock_parallel(L, T, [&](uint64_t a, uint64_t b) {
      const int w = next.fetch_add(1);
      for (uint64_t i = a; i < b; ++i) {
        const uint64_t k = live[i];
        const HafChoice c = haf_choose(list_of(k), in.n[k]);
        if ((c.lay.H + 63) / 64 > kFockMaxChunks) bad[w] = std::min(bad[w], k);
        sum[w] += c.lay.T;
        ops[w] += (double)c.lay.T * haf_ops(c.lay.nwalk, in.n[k], true);
      }
    });
    const uint64_t k = *std::min_element(bad.begin(), bad.end());
    if (k != ~0ull) {
      const HafChoice c = haf_choose(list_of(k), in.n[k]);
      set_error(who + ": item k = " + std::to_string(k) + " has " + std::to_string(c.lay.T) +
                " terms, more than 2^40 (2^24 wave-chunks of 64 lanes x 2^10 steps)");
      return SUP_EUNSUPPORTED;
    }
    double osum = 0.0;
    for (int w = 0; w < T; ++w) hi.terms += sum[w], osum += ops[w];
    hi.ops = hi.terms ? osum / (double)hi.terms : 0.0;
  }
  uint64_t slab_max = ~0ull;
  if (const char* e = std::getenv("SUP_HAFNIAN_SLAB")) {
    const long long v = std::atoll(e);
    if (v > 0) slab_max = (uint64_t)v;
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
    G = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)std::max(1, std::min(o.gpu_num, ndev - o.device_id)), L));
  }
  // one coefficient row per distinct order of the call: row n holds
  // 1 / (j! (n - 2j)!), j <= n / 2, hafnian_complex's values
  double fact[SUP_MAX_N + 1];
  fact[0] = 1.0;
  for (int i = 1; i <= SUP_MAX_N; ++i) fact[i] = fact[i - 1] * (double)i;
  std::vector<double> coef;
  uint32_t coef_at[SUP_MAX_N + 1];
  {
    bool seen[SUP_MAX_N + 1] = {false};
    for (uint64_t i = 0; i < L; ++i) seen[in.n[live[i]]] = true;
    for (int n = 1; n <= SUP_MAX_N; ++n) {
      coef_at[n] = (uint32_t)coef.size();
      if (seen[n])
        for (int j = 0; j <= n / 2; ++j) coef.push_back(1.0 / (fact[j] * fact[n - 2 * j]));
    }
  }
  std::vector<int> drc(G, SUP_OK), dgrid(G, 0);
  std::vector<double> dms(G, 0.0);
  std::vector<std::string> derr(G);
  // live items [a, b) in slabs under hafnian_complex's caps; orders mix freely
  auto work = [&](int g) {
    const uint64_t a = L * (uint64_t)g / (uint64_t)G, b = L * (uint64_t)(g + 1) / (uint64_t)G;
    try {
      std::vector<double> res;
      for (uint64_t i = a; i < b && !drc[g];) {
        HafSlab S;
        S.each = true;
        S.loop = true;
        S.coef = coef;
        S.div = 1.0;
        HafProgs progs;
        size_t bytes = 0;
        const uint64_t i0 = i;
        int64_t lo = row_of(live[i]), hi_row = lo;
        for (; i < b && i - i0 < slab_max; ++i) {
          const uint64_t k = live[i];
          const HafChoice c = haf_choose(list_of(k), in.n[k]);
          const size_t add = haf_bytes(c, 16);
          const uint64_t chunks = (c.lay.H + 63) / 64;
          if (i > i0 && (bytes + add > kHafSlabCapBytes || S.chunks.size() + chunks > 0x7fffffffull)) break;
          const int64_t row = row_of(k);
          haf_append(S, hin, c, progs, on_cpu, in.mu + 2 * (uint64_t)in.M * (uint64_t)row,
                     (uint32_t)in.n[k] | coef_at[in.n[k]] << 8);
          S.mu_row.push_back((int32_t)row);
          lo = std::min(lo, row), hi_row = std::max(hi_row, row);
          bytes += add;
        }
        // the device takes rows [lo, hi_row] of mu alone
        S.mu_lo = lo, S.mu_rows = hi_row - lo + 1;
        for (int32_t& r : S.mu_row) r -= (int32_t)lo;
        res.assign(2 * (i - i0), 0.0);
        if (on_cpu) {
          haf_cpu(S, std::max(o.threads, 1), res.data());
        } else {
          double ms = 0.0;
          drc[g] = run_hafnian(o.device_id + g, S, hin, res.data(), &ms, &dgrid[g]);
          if (drc[g]) derr[g] = last_error();
          dms[g] += ms;
        }
        if (!drc[g])
          for (uint64_t q = i0; q < i; ++q) out[2 * live[q]] = res[2 * (q - i0)], out[2 * live[q] + 1] = res[2 * (q - i0) + 1];
      }
    } catch (const std::bad_alloc&) {
      derr[g] = "out of host memory for a slab's tables and partials";
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
    hi.kernel_ms = *std::max_element(dms.begin(), dms.end());
    hi.grid = dgrid[0];
    hi.devices = G;
  }
  if (info) *info = hi;
  return SUP_OK;
}

}  // namespace sup
