// selftest_hafnian_exact.cpp — host-code self test of sup_hafnian_complex_exact
// for the sanitizer builds (make -C superman_amd/csrc sanitize-hafnian-exact:
// AddressSanitizer + UndefinedBehaviorSanitizer, and ThreadSanitizer).  No GPU
// is needed.  It drives, with on_cpu = 1 on 1, 3 and 8 host threads,
//   - both forms at n = 1, 6, 9, 14 with count 0, 1 and 7 and index lists that
//     repeat a lot, a little and not at all: every result is the string of the
//     call on that matrix alone, whatever the thread count and the slab size,
//     and equals the recursive definition in 128-bit integers (n <= 9);
//   - closed forms with many primes: one mode 64 times (63!!), and entries of
//     2^31 - 1 at n = 12 (three launches' worth of primes in the loop form);
//   - the divisor's self-check made to fail (SUP_EHIP with the message);
//   - the argument, symmetry, index, integrality, range and buffer checks.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../include/superman.h"

typedef __int128 i128;
struct Gi {
  i128 re, im;
};
static Gi mul(Gi a, Gi b) { return Gi{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
static Gi add(Gi a, Gi b) { return Gi{a.re + b.re, a.im + b.im}; }

static int failures = 0;
#define CHECK(c)                                                          \
  do {                                                                    \
    if (!(c)) {                                                           \
      std::fprintf(stderr, "CHECK failed %s:%d: %s (%s)\n", __FILE__,     \
                   __LINE__, #c, sup_last_error());                       \
      ++failures;                                                         \
    }                                                                     \
  } while (0)

static const size_t kLen = 768;

static sup_opts opts(int threads) {
  sup_opts o;
  sup_opts_init(&o);
  o.threads = threads;
  return o;
}

static std::string dec(i128 v) {
  if (v == 0) return "0";
  const bool neg = v < 0;
  unsigned __int128 u = neg ? (unsigned __int128)(-(v + 1)) + 1 : (unsigned __int128)v;
  std::string s;
  while (u) s.insert(s.begin(), (char)('0' + (int)(u % 10))), u /= 10;
  return neg ? "-" + s : s;
}

// A symmetric M x M matrix (interleaved) and a vector mu with parts in [-3, 3].
static void make_matrix(int M, unsigned seed, std::vector<double>& A, std::vector<double>& mu) {
  std::mt19937_64 g(seed);
  auto draw = [&]() { return (double)((int)(g() % 7u) - 3); };
  A.assign((size_t)2 * M * M, 0.0);
  mu.assign((size_t)2 * M, 0.0);
  for (int i = 0; i < M; ++i) {
    for (int j = 0; j <= i; ++j)
      for (int p = 0; p < 2; ++p) A[2 * ((size_t)i * M + j) + p] = A[2 * ((size_t)j * M + i) + p] = draw();
    mu[2 * i] = draw(), mu[2 * i + 1] = draw();
  }
}

static std::vector<int32_t> make_lists(int n, uint64_t count, int M, unsigned seed) {
  const int mod[3] = {2, M, 4};
  std::mt19937 g(seed);
  std::vector<int32_t> idx((size_t)(count ? count : 1) * n, 0);
  for (uint64_t k = 0; k < count; ++k)
    for (int j = 0; j < n; ++j) idx[k * n + j] = (int32_t)(g() % (unsigned)mod[k % 3]);
  return idx;
}

// The recursive definition on the gather by ix (mu null: the plain hafnian).
static Gi rec(const std::vector<double>& A, int M, const double* mu, std::vector<int32_t> ix) {
  if (ix.empty()) return Gi{1, 0};
  if (!mu && (ix.size() & 1)) return Gi{0, 0};
  const int32_t a = ix[0];
  std::vector<int32_t> rest(ix.begin() + 1, ix.end());
  Gi s = mu ? mul(Gi{(i128)mu[2 * a], (i128)mu[2 * a + 1]}, rec(A, M, mu, rest)) : Gi{0, 0};
  for (size_t j = 0; j < rest.size(); ++j) {
    std::vector<int32_t> r2(rest);
    r2.erase(r2.begin() + (long)j);
    const double* e = &A[2 * ((size_t)a * M + rest[j])];
    s = add(s, mul(Gi{(i128)e[0], (i128)e[1]}, rec(A, M, mu, r2)));
  }
  return s;
}

struct Out {
  std::vector<char> re, im;
  explicit Out(uint64_t count) : re(kLen * (count ? count : 1), 'x'), im(kLen * (count ? count : 1), 'x') {}
  std::string r(uint64_t k) const { return std::string(&re[k * kLen]); }
  std::string i(uint64_t k) const { return std::string(&im[k * kLen]); }
};

static void test_values_and_splits() {
  const int M = 9;
  std::vector<double> A, mu;
  make_matrix(M, 11, A, mu);
  for (int n : {1, 6, 9, 14})
    for (uint64_t count : {(uint64_t)0, (uint64_t)1, (uint64_t)7}) {
      const std::vector<int32_t> idx = make_lists(n, count, M, 100u + (unsigned)n);
      for (int loop = 0; loop < 2; ++loop) {
        const double* m = loop ? mu.data() : nullptr;
        sup_opts o1 = opts(1);
        Out ref(count);
        sup_stats st;
        CHECK(sup_hafnian_complex_exact(A.data(), M, m, idx.data(), n, count, &o1, 1, ref.re.data(), ref.im.data(), kLen,
                                        &st) == SUP_OK);
        CHECK(st.leaves == (int)count);
        for (uint64_t k = 0; k < count; ++k) {
          Out one(1);
          CHECK(sup_hafnian_complex_exact(A.data(), M, m, idx.data() + k * n, n, 1, &o1, 1, one.re.data(),
                                          one.im.data(), kLen, nullptr) == SUP_OK);
          CHECK(one.r(0) == ref.r(k) && one.i(0) == ref.i(k));
          if (n <= 9) {  // the recursion takes too long at n = 14
            const Gi t = rec(A, M, m, std::vector<int32_t>(idx.begin() + (long)(k * n), idx.begin() + (long)((k + 1) * n)));
            CHECK(ref.r(k) == dec(t.re) && ref.i(k) == dec(t.im));
          }
        }
        for (int threads : {3, 8})
          for (const char* slab : {"", "1", "3"}) {
            if (*slab) setenv("SUP_HAFNIAN_SLAB", slab, 1);
            sup_opts o = opts(threads);
            Out got(count);
            CHECK(sup_hafnian_complex_exact(A.data(), M, m, idx.data(), n, count, &o, 1, got.re.data(), got.im.data(),
                                            kLen, nullptr) == SUP_OK);
            for (uint64_t k = 0; k < count; ++k) CHECK(got.r(k) == ref.r(k) && got.i(k) == ref.i(k));
            unsetenv("SUP_HAFNIAN_SLAB");
          }
      }
    }
}

static void test_many_primes() {
  // one mode 64 times: 63!! = 3 x 5 x ... x 63 (147 bits)
  const double one[2] = {1.0, 0.0};
  std::vector<int32_t> idx(64, 0);
  Out out(1);
  sup_opts o = opts(8);
  sup_stats st;
  CHECK(sup_hafnian_complex_exact(one, 1, nullptr, idx.data(), 64, 1, &o, 1, out.re.data(), out.im.data(), kLen, &st) ==
        SUP_OK);
  CHECK(out.r(0) == "112275575285571389562324404930670903477890625" && out.i(0) == "0");  // 63!!
  CHECK(st.visited_steps == 64 && st.seg_cached_bits >= 6);
  // +-(2^31 - 1)(1 + i) on (3, 3, 3, 3): 10 primes, 18 in the loop form; threads agree
  const int M = 4;
  std::vector<double> A((size_t)2 * M * M), mu((size_t)2 * M);
  std::mt19937 g(5);
  for (int i = 0; i < M; ++i)
    for (int j = 0; j <= i; ++j) {
      const double s = (g() & 1u) ? 2147483647.0 : -2147483647.0;
      for (int p = 0; p < 2; ++p) A[2 * ((size_t)i * M + j) + p] = A[2 * ((size_t)j * M + i) + p] = s;
    }
  for (int i = 0; i < M; ++i) mu[2 * i] = A[2 * ((size_t)i * M + i)], mu[2 * i + 1] = A[2 * ((size_t)i * M + i) + 1];
  const int32_t i12[12] = {0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3};
  for (int loop = 0; loop < 2; ++loop) {
    Out a(1), b(1);
    sup_opts o1 = opts(1);
    CHECK(sup_hafnian_complex_exact(A.data(), M, loop ? mu.data() : nullptr, i12, 12, 1, &o1, 1, a.re.data(),
                                    a.im.data(), kLen, &st) == SUP_OK);
    CHECK(st.seg_cached_bits == (loop ? 18 : 10) && st.seg_pair_bits == (loop ? 3 : 2));
    CHECK(sup_hafnian_complex_exact(A.data(), M, loop ? mu.data() : nullptr, i12, 12, 1, &o, 1, b.re.data(),
                                    b.im.data(), kLen, nullptr) == SUP_OK);
    CHECK(a.r(0) == b.r(0) && a.i(0) == b.i(0) && a.r(0).size() + a.i(0).size() > 60);
  }
}

static void test_self_check() {
  // haf J_4 = 3: with the factor 2 of 2T / (m! 8^m) replaced by 1 the division fails
  std::vector<double> J((size_t)2 * 16, 0.0), mu(8, 0.0);
  for (int i = 0; i < 16; ++i) J[2 * i] = 1.0;
  const int32_t idx[4] = {0, 1, 2, 3};
  Out out(1);
  CHECK(sup_hafnian_complex_exact(J.data(), 4, nullptr, idx, 4, 1, nullptr, 1, out.re.data(), out.im.data(), kLen,
                                  nullptr) == SUP_OK);
  CHECK(out.r(0) == "3" && out.i(0) == "0");
  setenv("SUP_HAFNIAN_EXACT_TEST_MUL", "1", 1);
  CHECK(sup_hafnian_complex_exact(J.data(), 4, nullptr, idx, 4, 1, nullptr, 1, out.re.data(), out.im.data(), kLen,
                                  nullptr) == SUP_EHIP);
  CHECK(std::strstr(sup_last_error(), "self-check failed (2T not divisible by m! 8^m)") != nullptr);
  unsetenv("SUP_HAFNIAN_EXACT_TEST_MUL");
}

static void test_arguments() {
  const int M = 6;
  std::vector<double> A, mu;
  make_matrix(M, 3, A, mu);
  int32_t idx[4] = {0, 1, 2, 3};
  Out out(2);
  char* re = out.re.data();
  char* im = out.im.data();
  CHECK(sup_hafnian_complex_exact(nullptr, M, nullptr, idx, 2, 2, nullptr, 1, re, im, kLen, nullptr) == SUP_EINVAL);
  CHECK(sup_hafnian_complex_exact(A.data(), M, nullptr, nullptr, 2, 2, nullptr, 1, re, im, kLen, nullptr) == SUP_EINVAL);
  CHECK(sup_hafnian_complex_exact(A.data(), M, nullptr, idx, 2, 2, nullptr, 1, nullptr, im, kLen, nullptr) == SUP_EINVAL);
  CHECK(sup_hafnian_complex_exact(A.data(), M, nullptr, idx, 2, 2, nullptr, 1, re, nullptr, kLen, nullptr) == SUP_EINVAL);
  CHECK(sup_hafnian_complex_exact(A.data(), M, nullptr, idx, 0, 2, nullptr, 1, re, im, kLen, nullptr) == SUP_EINVAL);
  CHECK(sup_hafnian_complex_exact(A.data(), M, nullptr, idx, 65, 2, nullptr, 1, re, im, kLen, nullptr) == SUP_EINVAL);
  CHECK(sup_hafnian_complex_exact(A.data(), 0, nullptr, idx, 2, 2, nullptr, 1, re, im, kLen, nullptr) == SUP_EINVAL);
  CHECK(sup_hafnian_complex_exact(A.data(), M, nullptr, idx, 2, 0, nullptr, 1, nullptr, nullptr, 0, nullptr) == SUP_OK);
  CHECK(sup_hafnian_complex_exact(A.data(), M, mu.data(), idx, 2, 2, nullptr, 1, re, im, 1, nullptr) == SUP_EINVAL);
  CHECK(std::strstr(sup_last_error(), "out_len = 1 but a result needs") != nullptr);
  idx[3] = M;
  CHECK(sup_hafnian_complex_exact(A.data(), M, nullptr, idx, 2, 2, nullptr, 1, re, im, kLen, nullptr) == SUP_EINVAL);
  CHECK(std::strstr(sup_last_error(), "idx[k = 1][position 1] = 6") != nullptr);
  idx[3] = 3;
  std::vector<int32_t> id(42);
  std::vector<double> B((size_t)2 * 42 * 42, 0.0);
  for (int j = 0; j < 42; ++j) id[j] = j;
  CHECK(sup_hafnian_complex_exact(B.data(), 42, nullptr, id.data(), 42, 1, nullptr, 1, re, im, kLen, nullptr) ==
        SUP_EUNSUPPORTED);
  std::vector<double> C = A;
  C[2 * (1 * M + 4)] = C[2 * (4 * M + 1)] = 0.5;
  CHECK(sup_hafnian_complex_exact(C.data(), M, nullptr, idx, 2, 2, nullptr, 1, re, im, kLen, nullptr) == SUP_EINVAL);
  CHECK(std::strstr(sup_last_error(), "A entry (row 1, column 4, Re part) is not an integer") != nullptr);
  C[2 * (1 * M + 4)] = C[2 * (4 * M + 1)] = 2147483648.0;
  CHECK(sup_hafnian_complex_exact(C.data(), M, nullptr, idx, 2, 2, nullptr, 1, re, im, kLen, nullptr) == SUP_EINVAL);
  CHECK(std::strstr(sup_last_error(), "is out of range") != nullptr);
  std::vector<double> m2 = mu;
  m2[2 * 5 + 1] = -0.25;
  CHECK(sup_hafnian_complex_exact(A.data(), M, m2.data(), idx, 2, 2, nullptr, 1, re, im, kLen, nullptr) == SUP_EINVAL);
  CHECK(std::strstr(sup_last_error(), "mu entry (index 5, Im part) is not an integer") != nullptr);
  A[2 * (2 * M + 5) + 1] += 1.0;
  CHECK(sup_hafnian_complex_exact(A.data(), M, nullptr, idx, 2, 2, nullptr, 1, re, im, kLen, nullptr) == SUP_EINVAL);
  CHECK(std::strstr(sup_last_error(), "A[2][5] and A[5][2] differ") != nullptr);
}

int main() {
  test_values_and_splits();
  test_many_primes();
  test_self_check();
  test_arguments();
  std::printf("selftest_hafnian_exact: %s (%d failed checks)\n", failures ? "FAILED" : "ok", failures);
  return failures ? 1 : 0;
}
