// selftest_complex_exact.cpp — host-code self test of the exact complex entry
// points for the sanitizer builds (make -C superman_amd/csrc
// sanitize-complex-exact: AddressSanitizer + UndefinedBehaviorSanitizer, and
// ThreadSanitizer).  No GPU is needed.  It drives
//   - sup_perman_complex_exact and sup_perman_complex_exact_range with
//     on_cpu = 1 at n = 1, 2, 7, 12 on 1 and 8 host threads: the thread count
//     changes no residue and no digit, c J_n gives c^n n!, both G give the same
//     integer through a CRT of the range entry's residues, and aligned ranges
//     add modulo p to the whole;
//   - the several-pass prime case (parts of about 2^20 at n = 12);
//   - every argument check and input limit, the zero row, the empty range, the
//     short output buffer, and on_cpu = 0: n above
//     SUP_CPLX_EXACT_MAX_DEVICE_N is SUP_EUNSUPPORTED before any device is
//     looked for, and below it a machine without a device answers SUP_ENODEV.
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
typedef __int128 i128;

static std::vector<double> random_gauss(int n, unsigned seed, int lim) {
  std::mt19937_64 g(seed);
  std::uniform_int_distribution<int> d(-lim, lim);
  std::vector<double> a((size_t)2 * n * n);
  for (auto& v : a) v = (double)d(g);
  return a;
}

static bool has(const char* word) { return std::strstr(sup_last_error(), word) != nullptr; }

// residues -> the integer in (-M/2, M/2], for M below 2^126 (three primes of 42 bits)
static i128 crt_signed(const uint64_t* res, const uint64_t* p, int k) {
  u128 x = 0, M = 1;
  for (int i = 0; i < k; ++i) {
    // x += M * ((res - x) / M mod p)
    const uint64_t xm = (uint64_t)(x % p[i]), mm = (uint64_t)(M % p[i]);
    uint64_t inv = 1, b = mm, e = p[i] - 2;
    for (; e; e >>= 1, b = (uint64_t)((u128)b * b % p[i]))
      if (e & 1) inv = (uint64_t)((u128)inv * b % p[i]);
    const uint64_t d = (uint64_t)((u128)((res[i] + p[i] - xm) % p[i]) * inv % p[i]);
    x += M * d;
    M *= p[i];
  }
  return 2 * x > M ? (i128)x - (i128)M : (i128)x;
}

static void test_perman() {
  char re[2][640], im[2][640];
  for (int n : {1, 2, 7, 12}) {
    const std::vector<double> a = random_gauss(n, 300u + (unsigned)n, 3);
    sup_stats st;
    int k = 0;
    for (int threads : {1, 8}) {
      sup_opts o;
      sup_opts_init(&o);
      o.threads = threads;
      CHECK(sup_perman_complex_exact(a.data(), n, &o, 1, re[k], im[k], 640, &st) == SUP_OK);
      CHECK(st.devices_used == 0 && st.gray_steps == (1ull << (n - 1)) && st.leaves == 1);
      CHECK(st.seg_pair_bits == 1 || st.seg_pair_bits == 2);
      ++k;
    }
    CHECK(std::strcmp(re[0], re[1]) == 0 && std::strcmp(im[0], im[1]) == 0);
    // both G through the range entry: the whole range is T, perm = (4(n&1) - 2) T / 2^n
    for (int G : {1, 2})
      for (int wl : {0, 2}) {
        uint64_t p[2][16], rr[2][16], ri[2][16];
        int np[2] = {0, 0};
        sup_stats rs;
        uint64_t C = 0;
        for (int t = 0; t < 2; ++t) {
          sup_opts o;
          sup_opts_init(&o);
          o.threads = t ? 8 : 1;
          o.walk_log2 = wl;
          // the plan's chunk count: probe it with an empty range
          CHECK(sup_perman_complex_exact_range(a.data(), n, 0, 0, &o, 1, G, p[t], rr[t], ri[t], 16, &np[t], &rs) ==
                SUP_OK);
          C = 1ull << (n - 1 - rs.lane_bits - rs.walk_bits);
          CHECK(sup_perman_complex_exact_range(a.data(), n, 0, C, &o, 1, G, p[t], rr[t], ri[t], 16, &np[t], &rs) ==
                SUP_OK);
          CHECK(rs.seg_pair_bits == G && rs.gray_steps == (C << (rs.lane_bits + rs.walk_bits)) && rs.devices_used == 0);
        }
        CHECK(np[0] == np[1] && np[0] >= 1 && np[0] <= 3);
        CHECK(std::memcmp(p[0], p[1], sizeof(uint64_t) * np[0]) == 0);
        CHECK(std::memcmp(rr[0], rr[1], sizeof(uint64_t) * np[0]) == 0);
        CHECK(std::memcmp(ri[0], ri[1], sizeof(uint64_t) * np[0]) == 0);
        const i128 sgn = (n & 1) ? 1 : -1, Tr = crt_signed(rr[0], p[0], np[0]), Ti = crt_signed(ri[0], p[0], np[0]);
        CHECK(Tr % ((i128)1 << (n - 1)) == 0 && Ti % ((i128)1 << (n - 1)) == 0);
        CHECK((long long)(sgn * Tr / ((i128)1 << (n - 1))) == std::atoll(re[0]));
        CHECK((long long)(sgn * Ti / ((i128)1 << (n - 1))) == std::atoll(im[0]));
        // aligned halves and quarters add modulo p to the whole
        for (uint64_t pieces : {(uint64_t)2, (uint64_t)4}) {
          if (pieces > C) continue;
          std::vector<uint64_t> sr(np[0], 0), si(np[0], 0);
          for (uint64_t i = 0; i < pieces; ++i) {
            sup_opts o;
            sup_opts_init(&o);
            o.threads = i & 1 ? 8 : 1;
            o.walk_log2 = wl;
            uint64_t q[16], a_re[16], a_im[16];
            int nq = 0;
            CHECK(sup_perman_complex_exact_range(a.data(), n, i * (C / pieces), (i + 1) * (C / pieces), &o, 1, G, q, a_re,
                                                 a_im, 16, &nq, nullptr) == SUP_OK);
            CHECK(nq == np[0]);
            for (int j = 0; j < nq; ++j) sr[j] = (sr[j] + a_re[j]) % q[j], si[j] = (si[j] + a_im[j]) % q[j];
          }
          for (int j = 0; j < np[0]; ++j) CHECK(sr[j] == rr[0][j] && si[j] == ri[0][j]);
        }
      }
  }
  // closed forms: n = 1 the entry itself; (1+2i)(-3+i) + (2-i)(4i) = -1 + 3i; (1 - 2i)^7 7! for c J_7
  const double one[2] = {3.0, -2.0};
  CHECK(sup_perman_complex_exact(one, 1, nullptr, 1, re[0], im[0], 640, nullptr) == SUP_OK);
  CHECK(std::strcmp(re[0], "3") == 0 && std::strcmp(im[0], "-2") == 0);
  const double two[8] = {1.0, 2.0, 2.0, -1.0, 0.0, 4.0, -3.0, 1.0};
  CHECK(sup_perman_complex_exact(two, 2, nullptr, 1, re[0], im[0], 640, nullptr) == SUP_OK);
  CHECK(std::strcmp(re[0], "-1") == 0 && std::strcmp(im[0], "3") == 0);
  std::vector<double> cj((size_t)2 * 7 * 7);
  for (size_t i = 0; i < cj.size(); i += 2) cj[i] = 1.0, cj[i + 1] = -2.0;
  CHECK(sup_perman_complex_exact(cj.data(), 7, nullptr, 1, re[0], im[0], 640, nullptr) == SUP_OK);
  CHECK(std::atoll(re[0]) == 29LL * 5040 && std::atoll(im[0]) == -278LL * 5040);  // (1 - 2i)^7 = 29 - 278i
  // a zero row: "0", "0" without a walk
  std::vector<double> z = random_gauss(7, 9, 3);
  for (int c = 0; c < 14; ++c) z[(size_t)2 * 7 * 3 + c] = 0.0;
  sup_stats st;
  CHECK(sup_perman_complex_exact(z.data(), 7, nullptr, 1, re[0], im[0], 640, &st) == SUP_OK);
  CHECK(std::strcmp(re[0], "0") == 0 && std::strcmp(im[0], "0") == 0 && st.gray_steps == 0);
}

// Parts of about 2^20 at n = 12: a dozen primes of 26 bits, several passes of
// four on a device; here the same count through the host twin on 1 and 8
// threads, and a result too long for a short buffer.
static void test_many_primes() {
  const int n = 12;
  const std::vector<double> a = random_gauss(n, 77, 1 << 20);
  uint64_t p[32], rr[2][32], ri[2][32];
  int np = 0;
  for (int t = 0; t < 2; ++t) {
    sup_opts o;
    sup_opts_init(&o);
    o.threads = t ? 8 : 1;
    CHECK(sup_perman_complex_exact_range(a.data(), n, 0, 1, &o, 1, 0, p, rr[t], ri[t], 32, &np, nullptr) == SUP_OK);
  }
  CHECK(np >= 9 && np <= 32);
  CHECK(std::memcmp(rr[0], rr[1], sizeof(uint64_t) * np) == 0 && std::memcmp(ri[0], ri[1], sizeof(uint64_t) * np) == 0);
  CHECK(sup_perman_complex_exact_range(a.data(), n, 0, 1, nullptr, 1, 0, p, rr[0], ri[0], np - 1, &np, nullptr) ==
        SUP_EINVAL);
  CHECK(has("cap = "));
  char re[640], im[640];
  CHECK(sup_perman_complex_exact(a.data(), n, nullptr, 1, re, im, 640, nullptr) == SUP_OK);
  const size_t need = std::max(std::strlen(re), std::strlen(im)) + 1;
  CHECK(need > 60);
  char sre[640], sim[640];
  CHECK(sup_perman_complex_exact(a.data(), n, nullptr, 1, sre, sim, need - 1, nullptr) == SUP_EINVAL);
  CHECK(has(std::to_string(need).c_str()));
  CHECK(sup_perman_complex_exact(a.data(), n, nullptr, 1, sre, sim, need, nullptr) == SUP_OK);
  CHECK(std::strcmp(re, sre) == 0 && std::strcmp(im, sim) == 0);
}

static void test_arguments() {
  const std::vector<double> a = random_gauss(7, 5, 3);
  char re[640], im[640];
  uint64_t p[16], rr[16], ri[16];
  int np = 0;
  for (int on_cpu : {0, 1}) {  // the argument checks and input limits come before the cap and the device
    CHECK(sup_perman_complex_exact(nullptr, 7, nullptr, on_cpu, re, im, 640, nullptr) == SUP_EINVAL);
    CHECK(sup_perman_complex_exact(a.data(), 7, nullptr, on_cpu, nullptr, im, 640, nullptr) == SUP_EINVAL);
    CHECK(sup_perman_complex_exact(a.data(), 7, nullptr, on_cpu, re, nullptr, 640, nullptr) == SUP_EINVAL);
    for (int n : {0, -3, 65}) {
      CHECK(sup_perman_complex_exact(a.data(), n, nullptr, on_cpu, re, im, 640, nullptr) == SUP_EINVAL);
      CHECK(sup_perman_complex_exact_range(a.data(), n, 0, 1, nullptr, on_cpu, 0, p, rr, ri, 16, &np, nullptr) ==
            SUP_EINVAL);
    }
    CHECK(sup_perman_complex_exact_range(nullptr, 7, 0, 1, nullptr, on_cpu, 0, p, rr, ri, 16, &np, nullptr) == SUP_EINVAL);
    CHECK(sup_perman_complex_exact_range(a.data(), 7, 0, 1, nullptr, on_cpu, 0, nullptr, rr, ri, 16, &np, nullptr) ==
          SUP_EINVAL);
    CHECK(sup_perman_complex_exact_range(a.data(), 7, 0, 1, nullptr, on_cpu, 0, p, nullptr, ri, 16, &np, nullptr) ==
          SUP_EINVAL);
    CHECK(sup_perman_complex_exact_range(a.data(), 7, 0, 1, nullptr, on_cpu, 0, p, rr, nullptr, 16, &np, nullptr) ==
          SUP_EINVAL);
    CHECK(sup_perman_complex_exact_range(a.data(), 7, 0, 1, nullptr, on_cpu, 0, p, rr, ri, 16, nullptr, nullptr) ==
          SUP_EINVAL);
    for (int wl : {32, -1}) {
      sup_opts o;
      sup_opts_init(&o);
      o.walk_log2 = wl;
      CHECK(sup_perman_complex_exact(a.data(), 7, &o, on_cpu, re, im, 640, nullptr) == SUP_EINVAL);
      CHECK(sup_perman_complex_exact_range(a.data(), 7, 0, 1, &o, on_cpu, 0, p, rr, ri, 16, &np, nullptr) == SUP_EINVAL);
    }
    for (int g : {3, 4, -1}) {
      CHECK(sup_perman_complex_exact_range(a.data(), 7, 0, 1, nullptr, on_cpu, g, p, rr, ri, 16, &np, nullptr) ==
            SUP_EINVAL);
      CHECK(has("group = "));
    }
    // the input limits, each with its place in the message
    std::vector<double> b = a;
    b[2 * (1 * 7 + 2) + 1] = 0.5;
    CHECK(sup_perman_complex_exact(b.data(), 7, nullptr, on_cpu, re, im, 640, nullptr) == SUP_EINVAL);
    CHECK(has("row 1, column 2, Im part") && has("not an integer"));
    b = a;
    b[2 * (3 * 7 + 0)] = std::nan("");
    CHECK(sup_perman_complex_exact_range(b.data(), 7, 0, 1, nullptr, on_cpu, 0, p, rr, ri, 16, &np, nullptr) == SUP_EINVAL);
    CHECK(has("row 3, column 0, Re part") && has("not an integer"));
    b[2 * (3 * 7 + 0)] = INFINITY;
    CHECK(sup_perman_complex_exact(b.data(), 7, nullptr, on_cpu, re, im, 640, nullptr) == SUP_EINVAL);
    b = a;
    b[2 * (2 * 7 + 2)] = -2147483648.0;
    CHECK(sup_perman_complex_exact(b.data(), 7, nullptr, on_cpu, re, im, 640, nullptr) == SUP_EINVAL);
    CHECK(has("row 2, column 2, Re part") && has("out of range"));
    b[2 * (2 * 7 + 2)] = 2147483647.0;
    b[2 * (2 * 7 + 3) + 1] = -1.0;
    CHECK(sup_perman_complex_exact(b.data(), 7, nullptr, on_cpu, re, im, 640, nullptr) == SUP_EINVAL);
    CHECK(has("row 2") && has(">= 2^31"));
  }
  // G = 2 where its primes would fall below 20 bits: row bounds of 17 bits
  std::vector<double> w((size_t)2 * 6 * 6, 8191.0);
  CHECK(sup_perman_complex_exact_range(w.data(), 6, 0, 1, nullptr, 1, 2, p, rr, ri, 16, &np, nullptr) == SUP_EINVAL);
  CHECK(has("xbits = 17"));
  CHECK(sup_perman_complex_exact_range(w.data(), 6, 0, 1, nullptr, 1, 1, p, rr, ri, 16, &np, nullptr) == SUP_OK);
  CHECK(sup_perman_complex_exact_range(a.data(), 7, 0, 2, nullptr, 1, 0, p, rr, ri, 16, &np, nullptr) == SUP_EINVAL);  // one chunk
  CHECK(sup_perman_complex_exact_range(a.data(), 7, 1, 0, nullptr, 1, 0, p, rr, ri, 16, &np, nullptr) == SUP_EINVAL);
  rr[0] = ri[0] = 9;
  CHECK(sup_perman_complex_exact_range(a.data(), 7, 1, 1, nullptr, 1, 0, p, rr, ri, 16, &np, nullptr) == SUP_OK);
  CHECK(np >= 1 && rr[0] == 0 && ri[0] == 0);
  // on_cpu = 0: above the cap SUP_EUNSUPPORTED with the cap in the message, on any machine
  if (SUP_CPLX_EXACT_MAX_DEVICE_N < 64) {
    const int big = SUP_CPLX_EXACT_MAX_DEVICE_N + 1;
    const std::vector<double> b = random_gauss(big, 7, 3);
    CHECK(sup_perman_complex_exact(b.data(), big, nullptr, 0, re, im, 640, nullptr) == SUP_EUNSUPPORTED);
    CHECK(has(std::to_string(SUP_CPLX_EXACT_MAX_DEVICE_N).c_str()));
    CHECK(sup_perman_complex_exact_range(b.data(), big, 0, 1, nullptr, 0, 0, p, rr, ri, 16, &np, nullptr) ==
          SUP_EUNSUPPORTED);
    // the host twin serves it (two chunks of 2^7 subsets)
    sup_opts o;
    sup_opts_init(&o);
    o.walk_log2 = 1;
    o.threads = 8;
    uint64_t bp[64], br[64], bi[64];
    CHECK(sup_perman_complex_exact_range(b.data(), big, 5, 7, &o, 1, 0, bp, br, bi, 64, &np, nullptr) == SUP_OK);
  }
  // at or below the cap a machine without a device answers SUP_ENODEV (no CPU fallback)
  int ndev = 0;
  if (sup_device_count(&ndev) != SUP_OK || ndev == 0) {
    CHECK(sup_perman_complex_exact(a.data(), 7, nullptr, 0, re, im, 640, nullptr) == SUP_ENODEV);
    CHECK(sup_perman_complex_exact_range(a.data(), 7, 0, 1, nullptr, 0, 0, p, rr, ri, 16, &np, nullptr) == SUP_ENODEV);
  }
}

int main() {
  test_perman();
  test_many_primes();
  test_arguments();
  std::printf("selftest_complex_exact: %s (%d failed checks)\n", failures ? "FAILED" : "ok", failures);
  return failures ? 1 : 0;
}
