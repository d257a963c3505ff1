// hafnian_exact.cpp — exact hafnians and loop hafnians of Gaussian-integer
// matrices gathered by index lists that may repeat: sup_hafnian_complex_exact
// (DESIGN.md §8k), the integer truth the floating hafnian entries (hafnian.cpp,
// hafnian_pt.cpp) are judged against.
//
// The sum is hafnian.cpp's over the same multiplicity vectors, layout and Gray
// order, on the integers q', r' of hafexact.hpp; the slabs are built by
// hafnian.cpp's builder.  Here: the input limits, the bound and the primes
// (exact.cpp's exact_take_primes below 2^25), the per-prime tables (c_j, the
// signed binomials and the weight of every step-program entry, all reduced on
// the host), the host twin, and per matrix and part the CRT with the division
// by m! 8^m or n! 2^(n+m) and its self-check (exact.cpp's exact_crt_div).
// The host twin runs walk_hafexact.hip's residue operations through the same
// header functions; all are exact, so the residues agree one for one.
#include "hafnian_exact.hpp"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <new>
#include <thread>

#include "cplx_fock_build.hpp"
#include "engine.hpp"

namespace sup {

namespace {

using u128 = unsigned __int128;
inline uint64_t mulmod(uint64_t a, uint64_t b, uint64_t m) { return (uint64_t)((u128)a * b % m); }
inline uint32_t wt_row(int t) { return (uint32_t)(t * (t + 1) / 2); }

// An exact integer-valued |v| < 2^53 as a residue in [0, p).
inline uint64_t to_res(double v, uint64_t p) {
  const int64_t i = (int64_t)v % (int64_t)p;
  return (uint64_t)(i < 0 ? i + (int64_t)p : i);
}

// The slab-independent constants of prime p (hafexact.hpp: p, 1 / p, c_j and
// the signed binomials, in [0, p)) into pc[0 .. kHafxStepW).
void hafx_prime_consts(double* pc, uint64_t p, int n, bool loop) {
  std::fill(pc, pc + kHafxStepW, 0.0);
  pc[0] = (double)p;
  pc[1] = 1.0 / (double)p;
  // Pascal's triangle modulo p, rows 0..64
  std::vector<uint64_t> C(65 * 65, 0);
  for (int t = 0; t <= 64; ++t) {
    C[t * 65] = 1 % p;
    for (int v = 1; v <= t; ++v) C[t * 65 + v] = (C[(t - 1) * 65 + v - 1] + (v <= t - 1 ? C[(t - 1) * 65 + v] : 0)) % p;
  }
  for (int t = 0; t < 64; ++t)
    for (int v = 0; v <= t; ++v) {
      const uint64_t c = C[t * 65 + v];
      pc[kHafxBinom + wt_row(t) + v] = (double)((v & 1) ? (p - c) % p : c);
    }
  if (loop) {
    // c_j = n! / (j! (n-2j)!) 2^(m-j) = C(n, 2j) (j+1)(j+2)..(2j) 2^(m-j)
    const int m = n / 2;
    for (int j = 0; j <= m; ++j) {
      uint64_t c = C[n * 65 + 2 * j];
      for (int i = j + 1; i <= 2 * j; ++i) c = mulmod(c, (uint64_t)i, p);
      for (int i = 0; i < m - j; ++i) c = mulmod(c, 2, p);
      pc[kHafxCoef + j] = (double)c;
    }
  }
}

// ptab of a slab: per prime the constants of `base` and the weight of every
// entry of S.prog modulo p (the product over the walk digits of the signed
// binomials of the state the entry reaches; the padding entries stay 0).
void hafx_slab_ptab(const HafSlab& S, const std::vector<double>& base, int np, std::vector<double>& ptab) {
  const uint64_t stride = hafx_stride(S.prog.size());
  ptab.assign((size_t)np * stride, 0.0);
  for (int q = 0; q < np; ++q)
    std::copy(base.begin() + (size_t)q * kHafxStepW, base.begin() + (size_t)(q + 1) * kHafxStepW,
              ptab.begin() + (size_t)q * stride);
  std::vector<char> seen(S.prog.size(), 0);
  for (const HafMat& M : S.mats) {
    if (seen[M.prog]) continue;
    seen[M.prog] = 1;
    // the walk digits' radices: the layout is a function of the multiplicity vector
    FockGroups g;
    g.K = (int)M.K;
    for (int k = 0; k < g.K; ++k) g.val[k] = S.grp[M.grp + 2 * k], g.mult[k] = S.grp[M.grp + 2 * k + 1];
    const FockLayout l = fock_layout(g);
    uint32_t v[kHafWalkDigits] = {0};
    for (uint32_t t = 0; t < M.Tw; ++t) {
      if (t) {
        const uint32_t dsg = S.prog[M.prog + t].dsg;
        if (dsg & 1u) --v[dsg >> 1];
        else ++v[dsg >> 1];
      }
      for (int q = 0; q < np; ++q) {
        const double* pc = ptab.data() + (size_t)q * stride;
        const uint64_t p = (uint64_t)pc[0];
        uint64_t w = 1;
        for (uint32_t i = 0; i < M.W; ++i) w = mulmod(w, (uint64_t)pc[kHafxBinom + wt_row((int)l.radix[i] - 1) + v[i]], p);
        ptab[(size_t)q * stride + kHafxStepW + M.prog + t] = (double)w;
      }
    }
  }
}

// One wave-chunk of the slab's queue on the host: every valid lane's walk
// (walk_hafexact.hip's operations), its residues added modulo p into
// out[2 q], out[2 q + 1].
void hafx_chunk(const HafSlab& S, const std::vector<double>& tabs, const std::vector<double>& ptab, int np, uint64_t a,
                uint64_t* out) {
  const uint64_t stride = hafx_stride(S.prog.size());
  const FockChunk ck = S.chunks[a];
  const HafMat& M = S.mats[ck.mat];
  const double* tab = tabs.data() + M.tab;
  auto ld = [&](size_t pair) { return cx{tab[2 * pair], tab[2 * pair + 1]}; };
  auto fma_cx = [](double s, cx b, cx x) { return cx{__builtin_fma(s, b.re, x.re), __builtin_fma(s, b.im, x.im)}; };
  const HafStep* prog = S.prog.data() + M.prog;
  const uint32_t n = (uint32_t)S.n, m = n >> 1;
  const size_t hs = (size_t)kHafHigh + M.ndig, high0 = (size_t)kHafStart + 2 * (size_t)M.W * kHafRow;
  const int ge = M.W > 4u ? kHafWalkDigits : 4;
  std::vector<cx> acc(np);
  std::vector<double> hw(np);
  auto term = [&](cx Q, cx r, const double* pc) {
    const double p = pc[0], pinv = pc[1];
    const cx Qr = cxe_red2(Q, p, pinv);
    return S.loop ? hafx_loop_poly(Qr, cxe_red2(r, p, pinv), pc + kHafxCoef, n, p, pinv) : hafx_pow(Qr, m, p, pinv);
  };
  for (int q = 0; q < np; ++q) out[2 * q] = out[2 * q + 1] = 0;
  for (uint32_t lane = 0; lane < 64; ++lane) {
    const uint32_t h = 64u * ck.local + lane;
    if (h >= M.H) break;
    cx Q = ld(0), r = ld(1), G[kHafWalkDigits];
    for (int e = 0; e < kHafWalkDigits; ++e) G[e] = ld(2 + (size_t)e);
    std::fill(hw.begin(), hw.end(), 1.0);
    double dv[kHafHighDigits];
    uint32_t rem = h;
    for (uint32_t d = 0; d < M.ndig; ++d) {
      const HafDigit& D = S.dig[M.dig + d];
      const uint32_t qd = rem / D.radix, vd = rem - qd * D.radix;
      rem = qd;
      for (int q = 0; q < np; ++q) {
        const double* pc = ptab.data() + (size_t)q * stride;
        hw[q] = cxe_red(hw[q] * pc[kHafxBinom + D.wt_off + vd], pc[0], pc[1]);
      }
      const double dvd = -(double)vd;
      const size_t row = high0 + d * hs;
      cx t = ld(row);
      for (uint32_t e = 0; e < d; ++e) t = fma_cx(dv[e], ld(row + kHafHigh + e), t);
      Q = fma_cx(4.0 * dvd, t, Q);
      Q = fma_cx(dvd * dvd, ld(row + 1), Q);
      if (S.loop) r = fma_cx(dvd, ld(row + 2), r);
      for (int e = 0; e < ge; ++e) G[e] = fma_cx(dvd, ld(row + 3 + (size_t)e), G[e]);
      dv[d] = dvd;
    }
    for (int q = 0; q < np; ++q) acc[q] = term(Q, r, ptab.data() + (size_t)q * stride);
    for (uint32_t t = 1; t < M.Tw; ++t) {
      const size_t row = prog[t].row / 16;
      const double m4 = (prog[t].dsg & 1u) ? 4.0 : -4.0;
      Q = fma_cx(m4, G[prog[t].dsg >> 1], Q);
      Q = cx_add(Q, ld(row + kHafWalkDigits));
      for (int e = 0; e < ge; ++e) G[e] = cx_add(G[e], ld(row + (size_t)e));
      if (S.loop) r = cx_add(r, ld(row + kHafWalkDigits + 1));
      for (int q = 0; q < np; ++q) {
        const double* pc = ptab.data() + (size_t)q * stride;
        const double p = pc[0], pinv = pc[1];
        acc[q] = cx_add(acc[q], hafx_weigh(term(Q, r, pc), pc[kHafxStepW + M.prog + t], p, pinv));
        if ((t & 255u) == 0u) acc[q] = cxe_red2(acc[q], p, pinv);
      }
    }
    for (int q = 0; q < np; ++q) {
      const double* pc = ptab.data() + (size_t)q * stride;
      const double p = pc[0], pinv = pc[1];
      const cx s = hafx_weigh(cxe_red2(acc[q], p, pinv), hw[q], p, pinv);
      const uint64_t pq = (uint64_t)p;
      out[2 * q] = (out[2 * q] + to_res(s.re, pq)) % pq;
      out[2 * q + 1] = (out[2 * q + 1] + to_res(s.im, pq)) % pq;
    }
  }
}

// The host twin on a slab: `threads` threads share the queue's chunks, then
// each matrix's chunk residues add modulo p.  res as run_hafnian_exact's.
void hafx_cpu(const HafSlab& S, const HafIn& in, const std::vector<double>& ptab, int np, int threads, uint64_t* res) {
  std::vector<double> tabs((size_t)S.tab_doubles, 0.0);
  for (const HafMat& M : S.mats) {
    double* t = tabs.data() + M.tab;
    const int32_t* g = S.grp.data() + M.grp;
    for (uint32_t e = 0; e < M.pairs; ++e) {
      const cx v = hafx_entry(in.A, in.M, in.mu, g, (int)M.K, (int)M.W, (int)M.ndig, e);
      t[2 * (size_t)e] = v.re, t[2 * (size_t)e + 1] = v.im;
    }
  }
  const uint64_t count = S.chunks.size();
  std::vector<uint64_t> parts((size_t)count * 2 * (size_t)np, 0);
  const int nt = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)std::max(threads, 1), count));
  auto work = [&](int w) {
    for (uint64_t a = (uint64_t)w; a < count; a += (uint64_t)nt) hafx_chunk(S, tabs, ptab, np, a, &parts[a * 2 * np]);
  };
  std::vector<std::thread> th;
  for (int w = 1; w < nt; ++w) th.emplace_back(work, w);
  work(0);
  for (auto& t : th) t.join();
  const uint64_t stride = hafx_stride(S.prog.size());
  for (size_t k = 0; k < S.mats.size(); ++k)
    for (int q = 0; q < np; ++q) {
      const uint64_t pq = (uint64_t)ptab[(size_t)q * stride];
      uint64_t sr = 0, si = 0;
      for (uint32_t c = 0; c < S.mats[k].chunks; ++c) {
        const uint64_t* v = &parts[((size_t)S.mats[k].chunk0 + c) * 2 * np + 2 * q];
        sr = (sr + v[0]) % pq, si = (si + v[1]) % pq;
      }
      res[(k * np + q) * 2] = sr, res[(k * np + q) * 2 + 1] = si;
    }
}

// log2 of n! / (j! (n-2j)!) 2^(m-j)
double log2_cj(int n, int j) {
  const int m = n / 2;
  return (std::lgamma(n + 1.0) - std::lgamma(j + 1.0) - std::lgamma(n - 2 * j + 1.0)) / std::log(2.0) + (m - j);
}

// log2 of the bound on |Re|, |Im| of T (plain) or L (loop) of one list:
// 2^(n-1) R^m or 2^(n-1) sum_j c_j R^j R_mu^(n-2j), R and R_mu the sums of
// |Re| + |Im| over the gathered matrix and mu (0 for a sum that is 0).
double hafx_bound_bits(const HafIn& in, const int32_t* idx, int n) {
  double R = 0.0, Rmu = 0.0;  // exact: at most 2 x 4096 integers below 2^31
  for (int i = 0; i < n; ++i) {
    for (int j = 0; j < n; ++j) {
      const double* p = in.A + 2 * ((size_t)idx[i] * in.M + idx[j]);
      R += std::fabs(p[0]) + std::fabs(p[1]);
    }
    if (in.mu) Rmu += std::fabs(in.mu[2 * (size_t)idx[i]]) + std::fabs(in.mu[2 * (size_t)idx[i] + 1]);
  }
  const int m = n / 2;
  if (!in.mu) return R > 0.0 ? (n - 1) + m * std::log2(R) : 0.0;
  double best = -1.0, lt[SUP_MAX_N / 2 + 1];
  for (int j = 0; j <= m; ++j) {
    lt[j] = -1.0;
    if ((j > 0 && R == 0.0) || (n - 2 * j > 0 && Rmu == 0.0)) continue;
    lt[j] = log2_cj(n, j) + (j ? j * std::log2(R) : 0.0) + (n - 2 * j ? (n - 2 * j) * std::log2(Rmu) : 0.0);
    best = std::max(best, lt[j]);
  }
  if (best < 0.0) return 0.0;
  double s = 0.0;
  for (int j = 0; j <= m; ++j)
    if (lt[j] >= 0.0) s += std::exp2(lt[j] - best);
  return (n - 1) + best + std::log2(s);
}

int check_integer_part(double v, const std::string& who, const std::string& where) {
  if (!std::isfinite(v) || v != std::floor(v)) {
    set_error(who + ": " + where + " is not an integer (parts must be integers with |part| < 2^31)");
    return SUP_EINVAL;
  }
  if (std::fabs(v) >= 2147483648.0) {
    set_error(who + ": " + where + " is out of range (parts must be integers with |part| < 2^31)");
    return SUP_EINVAL;
  }
  return SUP_OK;
}

}  // namespace

int hafnian_exact(const HafIn& in0, int n, uint64_t count, const sup_opts& o, bool on_cpu,
                  std::vector<std::string>& re, std::vector<std::string>& im, HafxInfo* info) {
  const std::string who = "sup_hafnian_complex_exact";
  HafIn in = in0;
  in.loop = in.mu != nullptr;
  if (!in.A || !in.idx) {
    set_error(who + ": null pointer");
    return SUP_EINVAL;
  }
  if (int rc = haf_check_request(in, n, count, who)) return rc;
  for (int i = 0; i < in.M; ++i)
    for (int j = 0; j < in.M; ++j)
      for (int part = 0; part < 2; ++part)
        if (int rc = check_integer_part(in.A[2 * ((size_t)i * in.M + j) + part], who,
                                        "A entry (row " + std::to_string(i) + ", column " + std::to_string(j) + ", " +
                                            (part ? "Im" : "Re") + " part)"))
          return rc;
  if (in.mu)
    for (int i = 0; i < in.M; ++i)
      for (int part = 0; part < 2; ++part)
        if (int rc = check_integer_part(in.mu[2 * (size_t)i + part], who,
                                        "mu entry (index " + std::to_string(i) + ", " + (part ? "Im" : "Re") + " part)"))
          return rc;
  HafxInfo hi;
  if (info) *info = hi;
  re.assign(count, "0"), im.assign(count, "0");
  if (count == 0) return SUP_OK;
  if (!in.loop && (n & 1)) return SUP_OK;  // no perfect matching: exactly zero, nothing walked
  // every matrix's terms, census weight and bound before any work
  const int T = std::max(o.threads, 1);
  double bits = 0.0;
  double shared_sum = 0.0;  // sum over the matrices of T x hafx_ops_shared
  {
    std::vector<uint64_t> sum(T, 0), bad(T, ~0ull);
    std::vector<double> shared(T, 0.0), mb(T, 0.0);
    std::atomic<int> next{0};
    fock_parallel(count, T, [&](uint64_t a, uint64_t b) {
      const int w = next.fetch_add(1);
      for (uint64_t k = a; k < b; ++k) {
        const FockLayout l = fock_layout(fock_group_of(in.idx + k * n, n));
        if ((l.H + 63) / 64 > kFockMaxChunks) bad[w] = std::min(bad[w], k);
        sum[w] += l.T;
        shared[w] += (double)l.T * hafx_ops_shared(l.nwalk, in.loop);
        mb[w] = std::max(mb[w], hafx_bound_bits(in, in.idx + k * n, n));
      }
    });
    const uint64_t k = *std::min_element(bad.begin(), bad.end());
    if (k != ~0ull) {
      const FockLayout l = fock_layout(fock_group_of(in.idx + k * n, n));
      set_error(who + ": matrix k = " + std::to_string(k) + " has " + std::to_string(l.T) +
                " terms, more than 2^40 (2^24 wave-chunks of 64 lanes x 2^10 steps)");
      return SUP_EUNSUPPORTED;
    }
    for (int w = 0; w < T; ++w) hi.terms += sum[w], shared_sum += shared[w], bits = std::max(bits, mb[w]);
  }
  std::vector<double> primes;
  exact_take_primes(kHafxPrimeBits, bits + 3.0, primes);  // product > 8 x the bound
  const int np = (int)primes.size();
  hi.primes = np;
  hi.launches = (np + kHafxPrimes - 1) / kHafxPrimes;
  hi.ops = hi.terms ? (double)hi.launches * shared_sum / (double)hi.terms + (double)np * hafx_ops_prime(n, in.loop) : 0.0;
  std::vector<double> base((size_t)np * kHafxStepW);
  for (int q = 0; q < np; ++q) hafx_prime_consts(base.data() + (size_t)q * kHafxStepW, (uint64_t)primes[q], n, in.loop);
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
  // 2T / (m! 8^m) or 2L / (n! 2^(n+m)); SUP_HAFNIAN_EXACT_TEST_MUL (tests of the
  // self-check only) replaces the factor 2
  const int m = n / 2;
  ExactDivisor div;
  div.mul = 2;
  div.shift = in.loop ? n + m : 3 * m;
  div.fact = in.loop ? n : m;
  if (const char* e = std::getenv("SUP_HAFNIAN_EXACT_TEST_MUL")) div.mul = (uint32_t)std::max(1, std::atoi(e));
  const char* what = in.loop ? "2L not divisible by n! 2^(n+m)" : "2T not divisible by m! 8^m";
  std::vector<int> drc(G, SUP_OK), dgrid(G, 0);
  std::vector<double> dms(G, 0.0);
  std::vector<std::string> derr(G);  // g_err is thread_local: carry worker messages back
  // the step weights of a slab's programs are per prime: keep its program pool small
  constexpr size_t kHafxMaxProg = (size_t)1 << 20;
  auto work = [&](int g) {
    const uint64_t a = count * (uint64_t)g / (uint64_t)G, b = count * (uint64_t)(g + 1) / (uint64_t)G;
    try {
      for (uint64_t k = a; k < b && !drc[g];) {
        const uint64_t k0 = k;
        HafSlab S;
        uint64_t lim = slab_max;
        for (;;) {
          S = HafSlab{};
          S.n = n;
          S.loop = in.loop;
          k = haf_fill_slab(S, in, n, k0, b, lim, 16 * (size_t)kHafxPrimes, false);
          if (S.prog.size() <= kHafxMaxProg || k - k0 <= 1) break;
          lim = (k - k0) / 2;
        }
        const uint64_t K = k - k0;
        std::vector<double> ptab;
        hafx_slab_ptab(S, base, np, ptab);
        std::vector<uint64_t> res((size_t)K * np * 2, 0);
        if (on_cpu) {
          hafx_cpu(S, in, ptab, np, std::max(o.threads, 1), res.data());
        } else {
          double ms = 0.0;
          int launches = 0;
          drc[g] = run_hafnian_exact(o.device_id + g, S, in, primes, ptab, res.data(), &ms, &dgrid[g], &launches);
          if (drc[g]) {
            derr[g] = last_error();
            break;
          }
          dms[g] += ms;
        }
        std::vector<uint64_t> rr(np), ri(np);
        for (uint64_t i = 0; i < K && !drc[g]; ++i) {
          for (int q = 0; q < np; ++q) rr[q] = res[(i * np + q) * 2], ri[q] = res[(i * np + q) * 2 + 1];
          if ((drc[g] = exact_crt_div(primes, rr, div, (who + " (Re)").c_str(), what, re[k0 + i])) ||
              (drc[g] = exact_crt_div(primes, ri, div, (who + " (Im)").c_str(), what, im[k0 + i])))
            derr[g] = last_error();
        }
      }
    } catch (const std::bad_alloc&) {
      derr[g] = "out of host memory for a slab's tables and residues";
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
