// selftest_torontonian.cpp — host-code self test of the torontonian entry
// points for the sanitizer builds (make -C superman_amd/csrc
// sanitize-torontonian: AddressSanitizer + UndefinedBehaviorSanitizer, and
// ThreadSanitizer).  No GPU is needed.  It drives, with on_cpu = 1 on 1 and 8
// host threads,
//   - sup_torontonian at n = 1, 3, 6, 9, 11 with count 0, 1 and 9 (lists and
//     chunks shared among the threads): every result has the bits of the call
//     on that list alone on one thread; the closed form 3^n with equality; a
//     direct restatement (a fresh complex Cholesky per subset) to rounding;
//   - the masked and the from-nothing forms of the twin (TOR_TWIN_TAIL);
//   - sup_torontonian_range: whole, split and empty ranges, and n = 32 at both
//     ends of the subsets;
//   - sup_torontonian_plan and the stats against it;
//   - the argument, mode and range checks, NaN for a matrix that is not
//     positive definite, and the device cap.
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../include/superman.h"

typedef std::complex<double> cplx;

static int failures = 0;
#define CHECK(c)                                                          \
  do {                                                                    \
    if (!(c)) {                                                           \
      std::fprintf(stderr, "CHECK failed %s:%d: %s (%s)\n", __FILE__,     \
                   __LINE__, #c, sup_last_error());                       \
      ++failures;                                                         \
    }                                                                     \
  } while (0)

static bool same_bits(const std::vector<double>& a, const std::vector<double>& b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0);
}

static sup_opts opts(int threads) {
  sup_opts o;
  sup_opts_init(&o);
  o.threads = threads;
  return o;
}

// A 2M x 2M Hermitian matrix (interleaved) with small off-diagonal entries and
// a diagonal near 0.4: I - O_z is positive definite for every z.
static std::vector<double> make_matrix(int M, unsigned seed) {
  const int N = 2 * M;
  std::mt19937_64 g(seed);
  std::uniform_real_distribution<double> d(-0.3 / N, 0.3 / N);
  std::vector<double> O((size_t)2 * N * N, 0.0);
  for (int i = 0; i < N; ++i) {
    for (int j = 0; j < i; ++j) {
      const double re = d(g), im = d(g);
      O[2 * ((size_t)i * N + j)] = O[2 * ((size_t)j * N + i)] = re;
      O[2 * ((size_t)i * N + j) + 1] = im, O[2 * ((size_t)j * N + i) + 1] = -im;
    }
    O[2 * ((size_t)i * N + i)] = 0.4 + d(g);
  }
  return O;
}

// Distinct modes: list k is a rotation of a shuffle of 0..M-1, cut to n.
static std::vector<int32_t> make_lists(int n, uint64_t count, int M, unsigned seed) {
  std::mt19937 g(seed);
  std::vector<int32_t> base(M);
  for (int i = 0; i < M; ++i) base[i] = i;
  for (int i = M - 1; i > 0; --i) std::swap(base[i], base[g() % (unsigned)(i + 1)]);
  std::vector<int32_t> modes((size_t)(count ? count : 1) * n, 0);
  for (uint64_t k = 0; k < count; ++k)
    for (int j = 0; j < n; ++j) modes[k * n + j] = base[(j + 3 * k) % M];
  return modes;
}

// The definition: a fresh factor per subset, std::complex arithmetic.
static double direct(const std::vector<double>& O, int M, const int32_t* s, int n, double* S) {
  const int N = 2 * M;
  double tor = 0.0;
  *S = 0.0;
  for (uint32_t z = 0; z < (1u << n); ++z) {
    std::vector<int> r;
    for (int b = n - 1; b >= 0; --b)
      if ((z >> b) & 1u) r.push_back(s[b]), r.push_back(s[b] + M);
    const int R = (int)r.size();
    std::vector<cplx> L((size_t)R * R);
    double f = 1.0;
    for (int i = 0; i < R; ++i)
      for (int c = 0; c <= i; ++c) {
        cplx acc = (i == c ? 1.0 : 0.0) - cplx(O[2 * ((size_t)r[i] * N + r[c])], i == c ? 0.0 : O[2 * ((size_t)r[i] * N + r[c]) + 1]);
        for (int l = 0; l < c; ++l) acc -= L[(size_t)i * R + l] * std::conj(L[(size_t)c * R + l]);
        if (c < i) L[(size_t)i * R + c] = acc / L[(size_t)c * R + c].real();
        else L[(size_t)i * R + i] = std::sqrt(acc.real()), f /= L[(size_t)i * R + i].real();
      }
    tor += ((n - __builtin_popcount(z)) & 1) ? -f : f;
    *S += f;
  }
  return tor;
}

static void test_values_and_bits() {
  const int M = 12;
  const std::vector<double> O = make_matrix(M, 41);
  for (int n : {1, 3, 6, 9, 11})
    for (uint64_t count : {(uint64_t)0, (uint64_t)1, (uint64_t)9}) {
      const std::vector<int32_t> modes = make_lists(n, count, M, 100 + n);
      std::vector<double> one(count ? count : 1, -1.0), many(count ? count : 1, -1.0);  // count 0 writes nothing
      sup_opts o1 = opts(1), o8 = opts(8);
      sup_stats st;
      CHECK(sup_torontonian(O.data(), M, modes.data(), n, count, &o1, 1, one.data(), &st) == SUP_OK);
      CHECK(sup_torontonian(O.data(), M, modes.data(), n, count, &o8, 1, many.data(), nullptr) == SUP_OK);
      CHECK(same_bits(one, many));
      if (count) CHECK(st.visited_steps == (count << n) && st.leaves == (int)count && st.gray_steps == (count << n));
      for (uint64_t k = 0; k < count; ++k) {
        double alone = 0.0, S = 0.0;
        CHECK(sup_torontonian(O.data(), M, modes.data() + k * n, n, 1, &o1, 1, &alone, nullptr) == SUP_OK);
        CHECK(std::memcmp(&alone, &one[k], sizeof(double)) == 0);
        const double want = direct(O, M, modes.data() + k * n, n, &S);
        CHECK(std::fabs(alone - want) <= 64.0 * n * 2.220446049250313e-16 * S);
        for (const char* tail : {"0", "4", "6"}) {
          double v = 0.0;
          setenv("TOR_TWIN_TAIL", tail, 1);
          CHECK(sup_torontonian(O.data(), M, modes.data() + k * n, n, 1, &o8, 1, &v, nullptr) == SUP_OK);
          unsetenv("TOR_TWIN_TAIL");
          CHECK(std::memcmp(&alone, &v, sizeof(double)) == 0);
        }
      }
    }
  for (int n : {1, 5, 8, 14}) {  // O = (3/4) I: every pivot a power of two
    std::vector<double> D((size_t)8 * n * n, 0.0);
    for (int i = 0; i < 2 * n; ++i) D[2 * ((size_t)i * 2 * n + i)] = 0.75;
    std::vector<int32_t> modes(n);
    for (int i = 0; i < n; ++i) modes[i] = i;
    double v = 0.0;
    sup_opts o8 = opts(8);
    CHECK(sup_torontonian(D.data(), n, modes.data(), n, 1, &o8, 1, &v, nullptr) == SUP_OK);
    CHECK(v == std::pow(3.0, n));
  }
}

static void test_ranges() {
  const int M = 32;
  const std::vector<double> O = make_matrix(M, 43);
  const std::vector<int32_t> all = make_lists(32, 1, M, 7);
  sup_opts o8 = opts(8);
  for (int n : {5, 11, 13}) {
    double whole = 0.0, full = 0.0, a = 0.0, b = 0.0, e = 1.0;
    sup_stats st;
    CHECK(sup_torontonian(O.data(), M, all.data(), n, 1, &o8, 1, &whole, nullptr) == SUP_OK);
    CHECK(sup_torontonian_range(O.data(), M, all.data(), n, 0, 1ull << n, &o8, 1, &full, &st) == SUP_OK);
    CHECK(std::memcmp(&whole, &full, sizeof(double)) == 0 && st.visited_steps == (1ull << n));
    CHECK(sup_torontonian_range(O.data(), M, all.data(), n, 0, 1ull << (n - 1), &o8, 1, &a, nullptr) == SUP_OK);
    CHECK(sup_torontonian_range(O.data(), M, all.data(), n, 1ull << (n - 1), 1ull << n, &o8, 1, &b, nullptr) == SUP_OK);
    if (n >= 11) {  // at least two chunks: the halves are subtrees of the fold
      const double sum = a + b;
      CHECK(std::memcmp(&whole, &sum, sizeof(double)) == 0);
    }
    CHECK(sup_torontonian_range(O.data(), M, all.data(), n, 9, 9, &o8, 1, &e, nullptr) == SUP_OK && e == 0.0);
  }
  for (int threads : {1, 8}) {  // n = 32: 2^17 subsets per wave-chunk, both ends
    sup_opts o = opts(threads);
    double lo = 0.0, hi = 0.0;
    sup_stats st;
    CHECK(sup_torontonian_range(O.data(), M, all.data(), 32, 0, 128, &o, 1, &lo, &st) == SUP_OK);
    CHECK(st.visited_steps == 128 && st.gray_steps == (1ull << 32));
    CHECK(sup_torontonian_range(O.data(), M, all.data(), 32, (1ull << 32) - 128, 1ull << 32, &o, 1, &hi, nullptr) == SUP_OK);
    CHECK(std::isfinite(lo) && std::isfinite(hi) && hi != 0.0);
  }
}

static void test_arguments() {
  const int M = 4;
  std::vector<double> O = make_matrix(M, 45);
  int32_t modes[3] = {0, 1, 2};
  double out[2] = {0.0, 0.0};
  sup_opts o = opts(2);
  CHECK(sup_torontonian(nullptr, M, modes, 3, 1, &o, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_torontonian(O.data(), M, nullptr, 3, 1, &o, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_torontonian(O.data(), M, modes, 3, 1, &o, 1, nullptr, nullptr) == SUP_EINVAL);
  CHECK(sup_torontonian(O.data(), M, modes, 0, 1, &o, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_torontonian(O.data(), M, modes, 33, 1, &o, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_torontonian(O.data(), 0, modes, 3, 1, &o, 1, out, nullptr) == SUP_EINVAL);
  int32_t bad[3] = {0, 4, 2}, neg[3] = {0, -1, 2}, twice[3] = {2, 1, 2};
  CHECK(sup_torontonian(O.data(), M, bad, 3, 1, &o, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_torontonian(O.data(), M, neg, 3, 1, &o, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_torontonian(O.data(), M, twice, 3, 1, &o, 1, out, nullptr) == SUP_EINVAL);
  CHECK(std::strstr(sup_last_error(), "distinct") != nullptr);
  CHECK(sup_torontonian_range(O.data(), M, modes, 3, 5, 4, &o, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_torontonian_range(O.data(), M, modes, 3, 0, 9, &o, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_torontonian(O.data(), M, modes, 3, 1, nullptr, 1, out, nullptr) == SUP_OK);  // default options
  // errors come before any device work, and without a device the call says so
  const int rc = sup_torontonian(O.data(), M, twice, 3, 1, &o, 0, out, nullptr);
  CHECK(rc == SUP_EINVAL);
  uint64_t subsets = 0;
  double ops = 0.0;
  CHECK(sup_torontonian_plan(12, &subsets, &ops) == SUP_OK && subsets == 4096 && ops > 0.0);
  CHECK(sup_torontonian_plan(12, nullptr, nullptr) == SUP_OK);
  CHECK(sup_torontonian_plan(0, &subsets, &ops) == SUP_EINVAL && sup_torontonian_plan(33, &subsets, &ops) == SUP_EINVAL);
  sup_stats st;
  int32_t twelve[4] = {3, 0, 2, 1};
  CHECK(sup_torontonian(O.data(), M, twelve, 4, 1, &o, 1, out, &st) == SUP_OK);
  double ops4 = 0.0;
  CHECK(sup_torontonian_plan(4, nullptr, &ops4) == SUP_OK && st.est_ops_per_step == ops4);
  static_assert(SUP_TORONTONIAN_MAX_DEVICE_N == 32, "the cap is every n the entry takes");
  // not positive definite: NaN, no error code
  O[2 * ((size_t)1 * 2 * M + 1)] = 1.5;
  CHECK(sup_torontonian(O.data(), M, modes, 3, 1, &o, 1, out, nullptr) == SUP_OK && std::isnan(out[0]));
  int32_t clean[2] = {0, 2};
  CHECK(sup_torontonian(O.data(), M, clean, 2, 1, &o, 1, out, nullptr) == SUP_OK && std::isfinite(out[0]));
}

int main() {
  test_values_and_bits();
  test_ranges();
  test_arguments();
  std::printf("selftest_torontonian: %s (%d failed checks)\n", failures ? "FAILED" : "ok", failures);
  return failures ? 1 : 0;
}
