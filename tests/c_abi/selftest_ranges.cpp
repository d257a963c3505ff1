// selftest_ranges.cpp — host-code self test of the exact and double-double
// range entries for the sanitizer builds (make -C superman_amd/csrc
// sanitize-ranges: AddressSanitizer + UndefinedBehaviorSanitizer, and
// ThreadSanitizer).  No GPU is needed.  It drives
//   - sup_perman_exact_range and sup_perman_quad_range with on_cpu = 1 at
//     n = 1, 7, 12 and 33 on 1 and 8 host threads, every form and group the
//     entry accepts (n = 33: eight chunks of a short walk): the thread count
//     changes no bit, two pieces of a range add up modulo p, the whole range
//     is sup_perman_exact's integer (n <= 12, a CRT over the returned residues
//     in __int128) and, scaled, sup_perman_quad's bits and reported walk;
//   - every refusal: null pointers, n, walk_log2, form, group, the infeasible
//     group, form 2 without walk bits, bad ranges, cap too small.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../include/superman.h"

static int failures = 0;
#define CHECK(c)                                                          \
  do {                                                                    \
    if (!(c)) {                                                           \
      std::fprintf(stderr, "CHECK failed %s:%d: %s (%s)\n", __FILE__,     \
                   __LINE__, #c, sup_last_error());                       \
      ++failures;                                                         \
    }                                                                     \
  } while (0)

typedef unsigned __int128 u128;
static const int kCap = 128;

// density ~0.4, entries in {-1, 1, 2}, a full diagonal
static std::vector<int32_t> int_matrix(int n, unsigned seed) {
  std::mt19937_64 g(seed);
  std::vector<int32_t> a((size_t)n * n, 0);
  const int32_t vals[3] = {-1, 1, 2};
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j)
      if (i == j || g() % 5 < 2) a[(size_t)i * n + j] = vals[g() % 3];
  return a;
}

static uint64_t mulmod(uint64_t a, uint64_t b, uint64_t m) { return (uint64_t)((u128)a * b % m); }
static uint64_t powmod(uint64_t a, uint64_t e, uint64_t m) {
  uint64_t r = 1 % m;
  for (a %= m; e; e >>= 1, a = mulmod(a, a, m))
    if (e & 1) r = mulmod(r, a, m);
  return r;
}
// The signed integer below 2^125 in absolute value with these residues (Garner over at most 3 primes).
static __int128 crt_signed(const uint64_t* res, const uint64_t* p, int np) {
  u128 x = 0, M = 1;
  for (int i = 0; i < np; ++i) {
    const uint64_t xm = (uint64_t)(x % p[i]), Mm = (uint64_t)(M % p[i]);
    const uint64_t d = mulmod((res[i] + p[i] - xm) % p[i], powmod(Mm, p[i] - 2, p[i]), p[i]);
    x += M * d;
    M *= p[i];
  }
  return x > M / 2 ? -(__int128)(M - x) : (__int128)x;
}

struct ExactOut {
  uint64_t primes[kCap], res[kCap];
  int np = 0;
  std::vector<int> colmap;
  sup_stats st;
};

static int exact_range(const std::vector<int32_t>& a, int n, uint64_t c0, uint64_t c1, int threads, int wl, int form,
                       int group, ExactOut& out) {
  sup_opts o;
  sup_opts_init(&o);
  o.threads = threads;
  o.walk_log2 = wl;
  out.colmap.assign(n > 1 ? n - 1 : 1, -1);
  return sup_perman_exact_range(a.data(), SUP_INT32, n, c0, c1, &o, 1, form, group, out.primes, out.res, kCap,
                                &out.np, out.colmap.data(), &out.st);
}

static void test_exact() {
  for (int n : {1, 7, 12, 33}) {
    const std::vector<int32_t> a = int_matrix(n, 500u + (unsigned)n);
    const int wl = n == 33 ? 6 : 0;  // n = 33: eight of the 2^20 chunks of a 6-bit walk
    for (int form : {0, 1, 2})
      for (int group : {0, 1, 2, 4}) {
        ExactOut w[2];
        const int rc = exact_range(a, n, 0, 0, 1, wl, form, group, w[0]);  // an empty range: the plan
        if (form == 2 && n <= 7) {
          CHECK(rc == SUP_EINVAL);
          continue;
        }
        CHECK(rc == SUP_OK);
        const uint64_t chunks = 1ull << (n - 1 - w[0].st.lane_bits - w[0].st.walk_bits);
        const uint64_t c0 = n == 33 ? 5 : 0, c1 = n == 33 ? 13 : chunks;
        int k = 0;
        for (int threads : {1, 8}) CHECK(exact_range(a, n, c0, c1, threads, wl, form, group, w[k++]) == SUP_OK);
        CHECK(w[0].np == w[1].np && w[0].np >= 1 && w[0].np <= kCap);
        CHECK(std::memcmp(w[0].primes, w[1].primes, sizeof(uint64_t) * w[0].np) == 0);
        CHECK(std::memcmp(w[0].res, w[1].res, sizeof(uint64_t) * w[0].np) == 0);
        CHECK(w[0].colmap == w[1].colmap);
        CHECK(w[0].st.devices_used == 0 && w[0].st.leaves == 1);
        CHECK(group == 0 || w[0].st.seg_pair_bits == group);
        CHECK(form == 0 || w[0].st.walk_kind == form - 1);
        CHECK(w[0].st.gray_steps == (c1 - c0) << (w[0].st.lane_bits + w[0].st.walk_bits));
        for (int q = 0; q < w[0].np; ++q) CHECK(w[0].res[q] < w[0].primes[q]);
        if (c1 - c0 >= 2) {  // two pieces add up modulo p
          const uint64_t mid = c0 + (c1 - c0) / 2;
          ExactOut h0, h1;
          CHECK(exact_range(a, n, c0, mid, 8, wl, form, group, h0) == SUP_OK);
          CHECK(exact_range(a, n, mid, c1, 1, wl, form, group, h1) == SUP_OK);
          for (int q = 0; q < w[0].np; ++q) CHECK((h0.res[q] + h1.res[q]) % w[0].primes[q] == w[0].res[q]);
        }
        if (n != 33 && w[0].np <= 3) {  // the whole range is the permanent: (n odd: +) T / 2^(n-1)
          char buf[600];
          CHECK(sup_perman_exact(a.data(), SUP_INT32, n, nullptr, 1, buf, sizeof buf, nullptr) == SUP_OK);
          const __int128 T = crt_signed(w[0].res, w[0].primes, w[0].np);
          const __int128 want = (__int128)std::strtoll(buf, nullptr, 10) * ((n & 1) ? 1 : -1) * ((__int128)1 << (n - 1));
          CHECK(T == want);
        }
      }
  }
}

static void test_quad() {
  for (int n : {1, 7, 12, 33}) {
    const std::vector<int32_t> ai = int_matrix(n, 600u + (unsigned)n);
    std::vector<double> a(ai.begin(), ai.end());
    for (int c = 0; c < n; ++c) a[(size_t)(n / 2) * n + c] *= 0.1;
    for (int form : {0, 1, 2}) {
      sup_opts o;
      sup_opts_init(&o);
      o.walk_log2 = n == 33 ? 10 : 0;
      double hi[2] = {0, 0}, lo[2] = {0, 0};
      sup_stats st;
      std::vector<int> colmap(n > 1 ? n - 1 : 1, -1);
      int rc = sup_perman_quad_range(a.data(), SUP_FLOAT64, n, 0, 0, &o, 1, form, &hi[0], &lo[0], colmap.data(), &st);
      if (form == 2 && n <= 7) {
        CHECK(rc == SUP_EINVAL);
        continue;
      }
      CHECK(rc == SUP_OK && hi[0] == 0.0 && lo[0] == 0.0);
      const uint64_t chunks = 1ull << (n - 1 - st.lane_bits - st.walk_bits);
      const uint64_t c1 = n == 33 ? 2 : chunks;
      int k = 0;
      for (int threads : {1, 8}) {
        o.threads = threads;
        CHECK(sup_perman_quad_range(a.data(), SUP_FLOAT64, n, 0, c1, &o, 1, form, &hi[k], &lo[k], colmap.data(), &st) ==
              SUP_OK);
        ++k;
      }
      CHECK(hi[0] == hi[1] && lo[0] == lo[1] && std::isfinite(hi[0]));
      CHECK(st.devices_used == 0 && st.gray_steps == c1 << (st.lane_bits + st.walk_bits));
      CHECK(form == 0 || st.walk_kind == form - 1);
      for (int e = 0; e + 1 < n; ++e) CHECK(colmap[e] >= 0 && colmap[e] < n - 1);
      if (n == 33 || form != 0) continue;
      // form 0, default layout, whole range, scaled: sup_perman_quad's bits and its reported walk
      double qh = 0, ql = 0;
      sup_stats qs;
      CHECK(sup_perman_quad(a.data(), SUP_FLOAT64, n, nullptr, 1, &qh, &ql, &qs) == SUP_OK);
      const double f = 4.0 * (n & 1) - 2.0;
      CHECK(f * hi[0] == qh && f * lo[0] == ql);
      CHECK(qs.walk_kind == st.walk_kind && qs.est_ops_per_step == st.est_ops_per_step);
    }
  }
}

static void test_arguments() {
  const std::vector<int32_t> a = int_matrix(9, 5);
  const std::vector<double> d(a.begin(), a.end());
  uint64_t pr[kCap], rs[kCap];
  int np = 0;
  double hi = 0, lo = 0;
  auto ex = [&](const void* m, int n, uint64_t c0, uint64_t c1, const sup_opts* o, int form, int group, uint64_t* p,
                uint64_t* r, int cap, int* npp) {
    return sup_perman_exact_range(m, SUP_INT32, n, c0, c1, o, 1, form, group, p, r, cap, npp, nullptr, nullptr);
  };
  auto qd = [&](const void* m, int n, uint64_t c0, uint64_t c1, const sup_opts* o, int form, double* h, double* l) {
    return sup_perman_quad_range(m, SUP_FLOAT64, n, c0, c1, o, 1, form, h, l, nullptr, nullptr);
  };
  CHECK(ex(a.data(), 9, 0, 1, nullptr, 0, 0, pr, rs, kCap, &np) == SUP_OK && np >= 1);
  CHECK(ex(nullptr, 9, 0, 1, nullptr, 0, 0, pr, rs, kCap, &np) == SUP_EINVAL);
  CHECK(ex(a.data(), 9, 0, 1, nullptr, 0, 0, nullptr, rs, kCap, &np) == SUP_EINVAL);
  CHECK(ex(a.data(), 9, 0, 1, nullptr, 0, 0, pr, nullptr, kCap, &np) == SUP_EINVAL);
  CHECK(ex(a.data(), 9, 0, 1, nullptr, 0, 0, pr, rs, kCap, nullptr) == SUP_EINVAL);
  CHECK(ex(a.data(), 0, 0, 1, nullptr, 0, 0, pr, rs, kCap, &np) == SUP_EINVAL);
  CHECK(ex(a.data(), 65, 0, 1, nullptr, 0, 0, pr, rs, kCap, &np) == SUP_EINVAL);
  CHECK(ex(a.data(), 9, 1, 0, nullptr, 0, 0, pr, rs, kCap, &np) == SUP_EINVAL);
  CHECK(ex(a.data(), 9, 0, 2, nullptr, 0, 0, pr, rs, kCap, &np) == SUP_EINVAL);  // one chunk
  CHECK(ex(a.data(), 9, 0, 1, nullptr, 3, 0, pr, rs, kCap, &np) == SUP_EINVAL);
  CHECK(ex(a.data(), 9, 0, 1, nullptr, -1, 0, pr, rs, kCap, &np) == SUP_EINVAL);
  CHECK(ex(a.data(), 9, 0, 1, nullptr, 0, 3, pr, rs, kCap, &np) == SUP_EINVAL);
  CHECK(ex(a.data(), 9, 0, 1, nullptr, 0, 0, pr, rs, 0, &np) == SUP_EINVAL);
  CHECK(ex(a.data(), 9, 0, 1, nullptr, 0, 0, pr, rs, -1, &np) == SUP_EINVAL);
  CHECK(ex(a.data(), 7, 0, 1, nullptr, 2, 0, pr, rs, kCap, &np) == SUP_EINVAL);  // no walk bits
  CHECK(ex(a.data(), 9, 1, 1, nullptr, 0, 0, pr, rs, kCap, &np) == SUP_OK && np >= 1 && rs[0] == 0);
  sup_opts o;
  sup_opts_init(&o);
  o.walk_log2 = 32;
  CHECK(ex(a.data(), 9, 0, 1, &o, 0, 0, pr, rs, kCap, &np) == SUP_EINVAL);
  CHECK(qd(d.data(), 9, 0, 1, &o, 0, &hi, &lo) == SUP_EINVAL);
  o.walk_log2 = -1;
  CHECK(ex(a.data(), 9, 0, 1, &o, 0, 0, pr, rs, kCap, &np) == SUP_EINVAL);
  // an infeasible group: row sums of 2^16 - 1 leave G = 2 primes of 19 bits; three 35-bit primes with G = 1
  std::vector<int32_t> big(16, (1 << 14) - 1);
  big[0] += 3;
  CHECK(ex(big.data(), 4, 0, 1, nullptr, 0, 2, pr, rs, kCap, &np) == SUP_EINVAL);
  CHECK(std::strstr(sup_last_error(), "xbits = 16") != nullptr);
  CHECK(ex(big.data(), 4, 0, 1, nullptr, 0, 4, pr, rs, kCap, &np) == SUP_EINVAL);
  CHECK(ex(big.data(), 4, 0, 1, nullptr, 0, 1, pr, rs, kCap, &np) == SUP_OK && np >= 2);
  const int need = np;
  CHECK(ex(big.data(), 4, 0, 1, nullptr, 0, 1, pr, rs, need - 1, &np) == SUP_EINVAL);
  CHECK(ex(big.data(), 4, 0, 1, nullptr, 0, 1, pr, rs, need, &np) == SUP_OK);
  const std::vector<double> half(81, 0.5);  // not integers
  CHECK(sup_perman_exact_range(half.data(), SUP_FLOAT64, 9, 0, 1, nullptr, 1, 0, 0, pr, rs, kCap, &np, nullptr,
                               nullptr) == SUP_EINVAL);

  CHECK(qd(d.data(), 9, 0, 1, nullptr, 0, &hi, &lo) == SUP_OK);
  CHECK(qd(nullptr, 9, 0, 1, nullptr, 0, &hi, &lo) == SUP_EINVAL);
  CHECK(qd(d.data(), 9, 0, 1, nullptr, 0, nullptr, &lo) == SUP_EINVAL);
  CHECK(qd(d.data(), 9, 0, 1, nullptr, 0, &hi, nullptr) == SUP_EINVAL);
  CHECK(qd(d.data(), 0, 0, 1, nullptr, 0, &hi, &lo) == SUP_EINVAL);
  CHECK(qd(d.data(), 65, 0, 1, nullptr, 0, &hi, &lo) == SUP_EINVAL);
  CHECK(qd(d.data(), 9, 1, 0, nullptr, 0, &hi, &lo) == SUP_EINVAL);
  CHECK(qd(d.data(), 9, 0, 2, nullptr, 0, &hi, &lo) == SUP_EINVAL);
  CHECK(qd(d.data(), 9, 0, 1, nullptr, 3, &hi, &lo) == SUP_EINVAL);
  CHECK(qd(d.data(), 7, 0, 1, nullptr, 2, &hi, &lo) == SUP_EINVAL);
  CHECK(qd(d.data(), 9, 1, 1, nullptr, 0, &hi, &lo) == SUP_OK && hi == 0.0 && lo == 0.0);
}

int main() {
  test_exact();
  test_quad();
  test_arguments();
  std::printf("selftest_ranges: %s (%d failed checks)\n", failures ? "FAILED" : "ok", failures);
  return failures ? 1 : 0;
}
