// hafnian_quad.cpp — hafnians and loop hafnians in complex double-double:
// sup_hafnian_complex_quad and sup_loop_hafnian_complex_quad.
//
// The sum, the grouping, the layout, the slabs and the split over devices are
// hafnian.cpp's (haf_check_request, haf_fill_slab); hafdd_slab below turns a
// slab into what walk_hafdd.hip reads: the dd table's offsets, the step
// program with every weight converted from the exact integer, the dd weight
// triangle and the dd coefficients.  The host twin reads the same arrays and
// runs hafdd.hpp's operations in walk_hafdd.hip's order: chunk partials of four
// doubles, hafdd_fold_tree per matrix, hafdd_finish.  Result k is a function of
// (A, mu, idx[k]) only.
#include "hafnian_quad.hpp"

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <new>
#include <string>
#include <thread>

#include "cplx_fock_build.hpp"
#include "engine.hpp"

namespace sup {

namespace {

typedef unsigned __int128 u128;

inline uint32_t wt_row(int t) { return (uint32_t)(t * (t + 1) / 2); }

// The integer x < 2^106 (negated when neg) as a dd: hi = x rounded, lo = the
// exact remainder.
dd dd_from_u128(u128 x, bool neg) {
  const double hi = (double)x;
  const __int128 rem = (__int128)x - (__int128)hi;
  const double lo = (double)rem;
  return neg ? dd{-hi, -lo} : dd{hi, lo};
}

// Pascal's triangle in 64-bit integers: C(63, 31) < 2^63.
const std::vector<uint64_t>& binomials() {
  static const std::vector<uint64_t> b = [] {
    std::vector<uint64_t> t(wt_row(64), 0);
    std::vector<uint64_t> row{1};
    for (int n = 0; n < 64; ++n) {
      for (int v = 0; v <= n; ++v) t[wt_row(n) + v] = row[v];
      std::vector<uint64_t> next(n + 2, 1);
      for (int v = 1; v <= n; ++v) next[v] = row[v - 1] + row[v];
      row.swap(next);
    }
    return t;
  }();
  return b;
}

// n! as a dd, n <= 64: exact while n! has at most 106 significant bits (n <=
// 32 and beyond: 32! needs 87), dd_mul_d-rounded above.
void factorials(dd (&f)[SUP_MAX_N + 1]) {
  f[0] = dd{1.0, 0.0};
  for (int i = 1; i <= SUP_MAX_N; ++i) f[i] = dd_mul_d(f[i - 1], (double)i);
}

// The dd program of the walk-digit radix list `radix` from the fp64 program's
// entries src[0 .. Tw] (row and digit; Tw + 1 entries, the last the padding):
// the digits are replayed and each weight is the exact product of binomials.
void hafdd_program(const HafStep* src, const uint32_t* radix, int W, uint32_t Tw, HafddStep* dst) {
  const std::vector<uint64_t>& bin = binomials();
  uint32_t g[SUP_MAX_N] = {0};
  for (uint32_t t = 0; t <= Tw; ++t) {
    HafddStep s{};
    s.dsg = src[t].dsg;
    s.row = hafdd_row_bytes(s.dsg);
    if (t == Tw) {  // padding: the walk asks for entry t + 1 ahead
      s.row = hafdd_row_bytes(0u);
      dst[t] = s;
      break;
    }
    if (t > 0) {
      if (s.dsg & 1u) --g[s.dsg >> 1];
      else ++g[s.dsg >> 1];
    }
    u128 w = 1;  // prod C(s'_k, v_k) <= 2^(sum s'_k) < 2^64
    uint32_t par = 0;
    for (int i = 0; i < W; ++i) w *= bin[wt_row((int)radix[i] - 1) + g[i]], par += g[i];
    const dd wd = dd_from_u128(w, par & 1u);
    s.w_hi = wd.hi, s.w_lo = wd.lo;
    dst[t] = s;
  }
}

// The dd slab of the matrices [k0, k1) of in.idx from their fp64 slab F.
void hafdd_slab(HafddSlab& S, const HafSlab& F, const HafIn& in, int n, uint64_t k0, bool host_tables) {
  S.dig = F.dig;
  S.grp = F.grp;
  S.chunks = F.chunks;
  S.mats = F.mats;
  S.prog.assign(F.prog.size(), HafddStep{});
  std::vector<bool> built(F.prog.size(), false);
  for (size_t i = 0; i < S.mats.size(); ++i) {
    HafMat& M = S.mats[i];
    M.pairs = hafdd_pairs((int)M.W, (int)M.ndig);
    M.tab = S.tab_doubles;
    S.tab_doubles += (2 * (uint64_t)M.pairs + 7) / 8 * 8;  // tables start on 64 bytes
    if (!built[M.prog]) {
      const FockLayout l = fock_layout(fock_group_of(in.idx + (k0 + i) * (uint64_t)n, n));
      hafdd_program(F.prog.data() + M.prog, l.radix, l.nwalk, M.Tw, S.prog.data() + M.prog);
      built[M.prog] = true;
    }
  }
  if (host_tables) {
    S.tabs.assign(S.tab_doubles, 0.0);
    for (const HafMat& M : S.mats) {
      double* t = S.tabs.data() + M.tab;
      const int32_t* g = S.grp.data() + M.grp;
      for (uint32_t e = 0; e < M.pairs; ++e) {
        const cx v = hafdd_entry(in.A, in.M, in.loop ? in.mu : nullptr, g, (int)M.K, (int)M.W, (int)M.ndig, e);
        t[2 * (size_t)e] = v.re, t[2 * (size_t)e + 1] = v.im;
      }
    }
  }
}

// One wave-chunk of the slab's queue, every lane, then the 64-lane xor
// butterfly (walk_hafdd.hip's order).
cxdd hafdd_chunk(const HafddSlab& S, uint64_t a) {
  const cxdd zero{dd{0.0, 0.0}, dd{0.0, 0.0}};
  const FockChunk ck = S.chunks[a];
  const HafMat& M = S.mats[ck.mat];
  const std::vector<double>& wts = hafdd_weights();
  const double* tab = S.tabs.data() + M.tab;
  auto ld = [&](size_t pair) { return cx{tab[2 * pair], tab[2 * pair + 1]}; };
  auto ld4 = [&](size_t pair) { return cxdd{dd{tab[2 * pair], tab[2 * pair + 1]}, dd{tab[2 * pair + 2], tab[2 * pair + 3]}}; };
  const HafddStep* prog = S.prog.data() + M.prog;
  const uint32_t n = (uint32_t)S.n, m = n >> 1;
  const double* coef = S.coef.data();
  const size_t hs = (size_t)kHafddHigh + M.ndig, high0 = (size_t)kHafddStart + 2 * (size_t)M.W * kHafRow;
  const int ge = M.W > 4u ? kHafWalkDigits : 4;  // the G entries the walk updates
  auto term = [&](cxdd Q, cxdd r) { return S.loop ? hafdd_loop_poly(Q, r, coef, n) : hafdd_pow(Q, m); };
  cxdd v[64];
  for (uint32_t lane = 0; lane < 64; ++lane) {
    const uint32_t h = 64u * ck.local + lane;
    if (h >= M.H) {  // the device walks such a lane at h = 0 and drops its value
      v[lane] = zero;
      continue;
    }
    cxdd Q = ld4(0), r = ld4(2), G[kHafWalkDigits];
    for (int e = 0; e < kHafWalkDigits; ++e) G[e] = ld4(4 + 2 * (size_t)e);
    double dv[kHafHighDigits];
    uint32_t rem = h;
    dd hw{1.0, 0.0};
    for (uint32_t d = 0; d < M.ndig; ++d) {
      const HafDigit& D = S.dig[M.dig + d];
      const uint32_t qd = rem / D.radix, vd = rem - qd * D.radix;
      rem = qd;
      hw = dd_mul(hw, dd{wts[2 * (size_t)(D.wt_off + vd)], wts[2 * (size_t)(D.wt_off + vd) + 1]});
      const double dvd = -(double)vd;
      const size_t row = high0 + d * hs;
      cxdd t = ld4(row);
      for (uint32_t e = 0; e < d; ++e) {
        const cx b = ld(row + kHafddHigh + e);
        t = hafdd_mad(t, dv[e], b.re, b.im);
      }
      const double d2 = dvd + dvd, dsq = dvd * dvd;
      const cx bjj = ld(row + 2);
      Q = hafdd_mad_dd(Q, d2, t);
      Q = hafdd_mad(Q, dsq, bjj.re, bjj.im);
      if (S.loop) {
        const cx u = ld(row + 3);
        r = hafdd_mad(r, dvd, u.re, u.im);
      }
      for (int e = 0; e < ge; ++e) {
        const cx b = ld(row + 4 + (size_t)e);
        G[e] = hafdd_mad(G[e], dvd, b.re, b.im);
      }
      dv[d] = dvd;
    }
    cxdd acc = term(Q, r);
    for (uint32_t t = 1; t < M.Tw; ++t) {
      const size_t row = prog[t].row / 16;
      const double m2 = (prog[t].dsg & 1u) ? 2.0 : -2.0;
      const cx bdd = ld(row + kHafWalkDigits);
      Q = hafdd_step_q(Q, G[prog[t].dsg >> 1], m2, bdd.re, bdd.im);
      for (int e = 0; e < ge; ++e) {
        const cx c = ld(row + (size_t)e);
        G[e] = cxdd_add_d2(G[e], c.re, c.im);
      }
      if (S.loop) {
        const cx c = ld(row + kHafWalkDigits + 1);
        r = cxdd_add_d2(r, c.re, c.im);
      }
      acc = hafdd_accum(acc, dd{prog[t].w_hi, prog[t].w_lo}, term(Q, r));
    }
    v[lane] = hafdd_scale(acc, hw);
  }
  for (int off = 1; off <= 32; off <<= 1) {
    cxdd w[64];
    for (int l = 0; l < 64; ++l) w[l] = cxdd_add(v[l], v[l ^ off]);
    std::copy(w, w + 64, v);
  }
  return v[0];
}

// The host twin on a slab: `threads` threads share the queue's chunks, then
// each matrix's partials are folded.
void hafdd_cpu(const HafddSlab& S, int threads, double* out) {
  const uint64_t count = S.chunks.size();
  std::vector<double> parts(4 * (size_t)count, 0.0);
  const int nt = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)std::max(threads, 1), count));
  auto work = [&](int w) {
    for (uint64_t a = (uint64_t)w; a < count; a += (uint64_t)nt) {
      const cxdd v = hafdd_chunk(S, a);
      double* p = parts.data() + 4 * a;
      p[0] = v.re.hi, p[1] = v.re.lo, p[2] = v.im.hi, p[3] = v.im.lo;
    }
  };
  std::vector<std::thread> th;
  for (int w = 1; w < nt; ++w) th.emplace_back(work, w);
  work(0);
  for (auto& t : th) t.join();
  for (size_t k = 0; k < S.mats.size(); ++k) {
    const cxdd v =
        hafdd_finish(hafdd_fold_tree(parts.data() + 4 * (size_t)S.mats[k].chunk0, S.mats[k].chunks), S.div, S.loop);
    out[4 * k] = v.re.hi, out[4 * k + 1] = v.re.lo, out[4 * k + 2] = v.im.hi, out[4 * k + 3] = v.im.lo;
  }
}

}  // namespace

const std::vector<double>& hafdd_weights() {
  static const std::vector<double> w = [] {
    const std::vector<uint64_t>& b = binomials();
    std::vector<double> t(2 * b.size(), 0.0);
    for (int n = 0; n < 64; ++n)
      for (int v = 0; v <= n; ++v) {
        const dd x = dd_from_u128((u128)b[wt_row(n) + v], v & 1);
        t[2 * (size_t)(wt_row(n) + v)] = x.hi, t[2 * (size_t)(wt_row(n) + v) + 1] = x.lo;
      }
    return t;
  }();
  return w;
}

int hafnian_quad(const HafIn& in, int n, uint64_t count, const sup_opts& o, bool on_cpu, double* out, HafInfo* info) {
  const std::string who = in.loop ? "sup_loop_hafnian_complex_quad" : "sup_hafnian_complex_quad";
  if (!out || !in.A || !in.idx || (in.loop && !in.mu)) {
    set_error(who + ": null pointer");
    return SUP_EINVAL;
  }
  if (int rc = haf_check_request(in, n, count, who)) return rc;
  if (!on_cpu && n > SUP_HAFNIAN_QUAD_MAX_DEVICE_N) {  // before the device is looked for: the same answer on any machine
    set_error(who + ": n = " + std::to_string(n) + " is above SUP_HAFNIAN_QUAD_MAX_DEVICE_N = " +
              std::to_string(SUP_HAFNIAN_QUAD_MAX_DEVICE_N) + " (on_cpu = 1 runs host threads)");
    return SUP_EUNSUPPORTED;
  }
  HafInfo hi;
  if (info) *info = hi;
  if (count == 0) return SUP_OK;
  if (!in.loop && (n & 1)) {  // no perfect matching: exactly zero, nothing walked
    std::fill(out, out + 4 * count, 0.0);
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
        const FockLayout l = fock_layout(fock_group_of(in.idx + k * n, n));
        if ((l.H + 63) / 64 > kFockMaxChunks) bad[w] = std::min(bad[w], k);
        sum[w] += l.T;
        ops[w] += (double)l.T * hafdd_ops(l.nwalk, n, in.loop);
      }
    });
    const uint64_t k = *std::min_element(bad.begin(), bad.end());
    if (k != ~0ull) {
      const FockLayout l = fock_layout(fock_group_of(in.idx + k * n, n));
      set_error(who + ": matrix k = " + std::to_string(k) + " has " + std::to_string(l.T) +
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
  dd fact[SUP_MAX_N + 1];
  factorials(fact);
  std::vector<double> coef;  // 1 / (j! (n - 2j)!) by dd_div of 1 by the dd product
  if (in.loop)
    for (int j = 0; j <= n / 2; ++j) {
      const dd c = dd_div(dd{1.0, 0.0}, dd_mul(fact[j], fact[n - 2 * j]));
      coef.push_back(c.hi), coef.push_back(c.lo);
    }
  std::vector<int> drc(G, SUP_OK), dgrid(G, 0);
  std::vector<double> dms(G, 0.0);
  std::vector<std::string> derr(G);  // g_err is thread_local: carry worker messages back
  // matrices [a, b) in slabs, as hafnian_complex cuts them (32 bytes of partials per wave-chunk)
  auto work = [&](int g) {
    const uint64_t a = count * (uint64_t)g / (uint64_t)G, b = count * (uint64_t)(g + 1) / (uint64_t)G;
    try {
      for (uint64_t k = a; k < b && !drc[g];) {
        HafSlab F;
        F.n = n;
        F.loop = in.loop;
        const uint64_t k0 = k;
        k = haf_fill_slab(F, in, n, k, b, slab_max, 32, false);
        HafddSlab S;
        S.n = n;
        S.loop = in.loop;
        S.coef = coef;
        S.div = fact[n / 2];
        hafdd_slab(S, F, in, n, k0, on_cpu);
        if (on_cpu) {
          hafdd_cpu(S, std::max(o.threads, 1), out + 4 * k0);
        } else {
          double ms = 0.0;
          drc[g] = run_hafnian_quad(o.device_id + g, S, in, out + 4 * k0, &ms, &dgrid[g]);
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

}  // namespace sup
