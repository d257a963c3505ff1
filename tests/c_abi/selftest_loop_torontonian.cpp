// selftest_loop_torontonian.cpp — host-code self test of the loop torontonian
// entry points for the sanitizer builds (make -C superman_amd/csrc
// sanitize-loop-torontonian: AddressSanitizer + UndefinedBehaviorSanitizer, and
// ThreadSanitizer).  No GPU is needed.  It drives, with on_cpu = 1 on 1 and 8
// host threads,
//   - sup_loop_torontonian at n = 1, 3, 6, 9, 11 with count 0, 1 and 9 (lists
//     and chunks shared among the threads): every result has the bits of the
//     call on that list alone on one thread; gamma = 0 has sup_torontonian's
//     bits; a direct restatement (a fresh complex Cholesky and forward solve
//     per subset, std::exp) to rounding;
//   - the masked and the from-nothing forms of the twin (LTOR_TWIN_TAIL);
//   - sup_loop_torontonian_range: whole, split and empty ranges, and n = 32 at
//     both ends of the subsets;
//   - sup_loop_torontonian_plan and the stats against it;
//   - the argument, mode and range checks, NaN for a matrix that is not
//     positive definite, inf for an exponent beyond the range, the device cap;
//   - sup_ltor_exp at its edges and against std::exp, and
//     sup_ltor_exp_device's argument checks.
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
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
static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }

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

// 2M complex entries of size about `scale`.
static std::vector<double> make_gamma(int M, unsigned seed, double scale) {
  std::mt19937_64 g(seed);
  std::uniform_real_distribution<double> d(-scale, scale);
  std::vector<double> v((size_t)4 * M);
  for (double& x : v) x = d(g);
  return v;
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

// The definition: a fresh factor and forward solve per subset, std::complex
// arithmetic, std::exp.
static double direct(const std::vector<double>& O, const std::vector<double>& gm, int M, const int32_t* s, int n, double* S) {
  const int N = 2 * M;
  double ltor = 0.0;
  *S = 0.0;
  for (uint32_t z = 0; z < (1u << n); ++z) {
    std::vector<int> r;
    for (int b = n - 1; b >= 0; --b)
      if ((z >> b) & 1u) r.push_back(s[b]), r.push_back(s[b] + M);
    const int R = (int)r.size();
    std::vector<cplx> L((size_t)R * R), y(R);
    double f = 1.0, q = 0.0;
    for (int i = 0; i < R; ++i) {
      for (int c = 0; c <= i; ++c) {
        cplx acc = (i == c ? 1.0 : 0.0) - cplx(O[2 * ((size_t)r[i] * N + r[c])], i == c ? 0.0 : O[2 * ((size_t)r[i] * N + r[c]) + 1]);
        for (int l = 0; l < c; ++l) acc -= L[(size_t)i * R + l] * std::conj(L[(size_t)c * R + l]);
        if (c < i) L[(size_t)i * R + c] = acc / L[(size_t)c * R + c].real();
        else L[(size_t)i * R + i] = std::sqrt(acc.real()), f /= L[(size_t)i * R + i].real();
      }
      cplx acc(gm[2 * (size_t)r[i]], gm[2 * (size_t)r[i] + 1]);
      for (int l = 0; l < i; ++l) acc -= L[(size_t)i * R + l] * y[l];
      y[i] = acc / L[(size_t)i * R + i].real();
      q += std::norm(y[i]);
    }
    f *= std::exp(0.5 * q);
    ltor += ((n - __builtin_popcount(z)) & 1) ? -f : f;
    *S += f;
  }
  return ltor;
}

static void test_values_and_bits() {
  const int M = 12;
  const std::vector<double> O = make_matrix(M, 41);
  const std::vector<double> gm = make_gamma(M, 42, 0.4), zero((size_t)4 * M, 0.0);
  for (int n : {1, 3, 6, 9, 11})
    for (uint64_t count : {(uint64_t)0, (uint64_t)1, (uint64_t)9}) {
      const std::vector<int32_t> modes = make_lists(n, count, M, 100 + n);
      std::vector<double> one(count ? count : 1, -1.0), many(count ? count : 1, -1.0);  // count 0 writes nothing
      std::vector<double> lz(count ? count : 1, -1.0), tz(count ? count : 1, -1.0);
      sup_opts o1 = opts(1), o8 = opts(8);
      sup_stats st;
      CHECK(sup_loop_torontonian(O.data(), M, gm.data(), modes.data(), n, count, &o1, 1, one.data(), &st) == SUP_OK);
      CHECK(sup_loop_torontonian(O.data(), M, gm.data(), modes.data(), n, count, &o8, 1, many.data(), nullptr) == SUP_OK);
      CHECK(same_bits(one, many));
      CHECK(sup_loop_torontonian(O.data(), M, zero.data(), modes.data(), n, count, &o8, 1, lz.data(), nullptr) == SUP_OK);
      CHECK(sup_torontonian(O.data(), M, modes.data(), n, count, &o8, 1, tz.data(), nullptr) == SUP_OK);
      CHECK(same_bits(lz, tz));
      if (count) CHECK(st.visited_steps == (count << n) && st.leaves == (int)count && st.gray_steps == (count << n));
      for (uint64_t k = 0; k < count; ++k) {
        double alone = 0.0, S = 0.0;
        CHECK(sup_loop_torontonian(O.data(), M, gm.data(), modes.data() + k * n, n, 1, &o1, 1, &alone, nullptr) == SUP_OK);
        CHECK(same_bits(alone, one[k]));
        const double want = direct(O, gm, M, modes.data() + k * n, n, &S);
        CHECK(std::fabs(alone - want) <= 64.0 * n * 2.220446049250313e-16 * 8.0 * S);  // exponents below 7
        for (const char* tail : {"0", "4", "6"}) {
          double v = 0.0;
          setenv("LTOR_TWIN_TAIL", tail, 1);
          CHECK(sup_loop_torontonian(O.data(), M, gm.data(), modes.data() + k * n, n, 1, &o8, 1, &v, nullptr) == SUP_OK);
          unsetenv("LTOR_TWIN_TAIL");
          CHECK(same_bits(alone, v));
        }
      }
    }
}

static void test_ranges() {
  const int M = 32;
  const std::vector<double> O = make_matrix(M, 43);
  const std::vector<double> gm = make_gamma(M, 44, 0.2);
  const std::vector<int32_t> all = make_lists(32, 1, M, 7);
  sup_opts o8 = opts(8);
  for (int n : {5, 11, 13}) {
    double whole = 0.0, full = 0.0, a = 0.0, b = 0.0, e = 1.0;
    sup_stats st;
    CHECK(sup_loop_torontonian(O.data(), M, gm.data(), all.data(), n, 1, &o8, 1, &whole, nullptr) == SUP_OK);
    CHECK(sup_loop_torontonian_range(O.data(), M, gm.data(), all.data(), n, 0, 1ull << n, &o8, 1, &full, &st) == SUP_OK);
    CHECK(same_bits(whole, full) && st.visited_steps == (1ull << n));
    CHECK(sup_loop_torontonian_range(O.data(), M, gm.data(), all.data(), n, 0, 1ull << (n - 1), &o8, 1, &a, nullptr) == SUP_OK);
    CHECK(sup_loop_torontonian_range(O.data(), M, gm.data(), all.data(), n, 1ull << (n - 1), 1ull << n, &o8, 1, &b, nullptr) == SUP_OK);
    if (n >= 11) CHECK(same_bits(whole, a + b));  // at least two chunks: the halves are subtrees of the fold
    CHECK(sup_loop_torontonian_range(O.data(), M, gm.data(), all.data(), n, 9, 9, &o8, 1, &e, nullptr) == SUP_OK && e == 0.0);
  }
  for (int threads : {1, 8}) {  // n = 32: 2^17 subsets per wave-chunk, both ends
    sup_opts o = opts(threads);
    double lo = 0.0, hi = 0.0;
    sup_stats st;
    CHECK(sup_loop_torontonian_range(O.data(), M, gm.data(), all.data(), 32, 0, 128, &o, 1, &lo, &st) == SUP_OK);
    CHECK(st.visited_steps == 128 && st.gray_steps == (1ull << 32));
    CHECK(sup_loop_torontonian_range(O.data(), M, gm.data(), all.data(), 32, (1ull << 32) - 128, 1ull << 32, &o, 1, &hi, nullptr) == SUP_OK);
    CHECK(std::isfinite(lo) && std::isfinite(hi) && hi != 0.0);
  }
}

static void test_arguments() {
  const int M = 4;
  std::vector<double> O = make_matrix(M, 45);
  std::vector<double> gm = make_gamma(M, 46, 0.3);
  int32_t modes[3] = {0, 1, 2};
  double out[2] = {0.0, 0.0};
  sup_opts o = opts(2);
  CHECK(sup_loop_torontonian(nullptr, M, gm.data(), modes, 3, 1, &o, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_loop_torontonian(O.data(), M, nullptr, modes, 3, 1, &o, 1, out, nullptr) == SUP_EINVAL);
  CHECK(std::strstr(sup_last_error(), "null pointer") != nullptr);
  CHECK(sup_loop_torontonian(O.data(), M, gm.data(), nullptr, 3, 1, &o, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_loop_torontonian(O.data(), M, gm.data(), modes, 3, 1, &o, 1, nullptr, nullptr) == SUP_EINVAL);
  CHECK(sup_loop_torontonian(O.data(), M, gm.data(), modes, 0, 1, &o, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_loop_torontonian(O.data(), M, gm.data(), modes, 33, 1, &o, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_loop_torontonian(O.data(), 0, gm.data(), modes, 3, 1, &o, 1, out, nullptr) == SUP_EINVAL);
  int32_t bad[3] = {0, 4, 2}, neg[3] = {0, -1, 2}, twice[3] = {2, 1, 2};
  CHECK(sup_loop_torontonian(O.data(), M, gm.data(), bad, 3, 1, &o, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_loop_torontonian(O.data(), M, gm.data(), neg, 3, 1, &o, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_loop_torontonian(O.data(), M, gm.data(), twice, 3, 1, &o, 1, out, nullptr) == SUP_EINVAL);
  CHECK(std::strstr(sup_last_error(), "distinct") != nullptr);
  CHECK(sup_loop_torontonian_range(O.data(), M, gm.data(), modes, 3, 5, 4, &o, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_loop_torontonian_range(O.data(), M, gm.data(), modes, 3, 0, 9, &o, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_loop_torontonian_range(O.data(), M, nullptr, modes, 3, 0, 8, &o, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_loop_torontonian(O.data(), M, gm.data(), modes, 3, 1, nullptr, 1, out, nullptr) == SUP_OK);  // default options
  // errors come before any device work
  CHECK(sup_loop_torontonian(O.data(), M, gm.data(), twice, 3, 1, &o, 0, out, nullptr) == SUP_EINVAL);
  CHECK(sup_loop_torontonian(O.data(), M, nullptr, modes, 3, 1, &o, 0, out, nullptr) == SUP_EINVAL);
  uint64_t subsets = 0;
  double ops = 0.0, tops = 0.0;
  CHECK(sup_loop_torontonian_plan(12, &subsets, &ops) == SUP_OK && subsets == 4096 && ops > 0.0);
  CHECK(sup_torontonian_plan(12, nullptr, &tops) == SUP_OK && tops > 0.0);
  CHECK(sup_loop_torontonian_plan(12, nullptr, nullptr) == SUP_OK);
  CHECK(sup_loop_torontonian_plan(0, &subsets, &ops) == SUP_EINVAL && sup_loop_torontonian_plan(33, &subsets, &ops) == SUP_EINVAL);
  sup_stats st;
  int32_t four[4] = {3, 0, 2, 1};
  CHECK(sup_loop_torontonian(O.data(), M, gm.data(), four, 4, 1, &o, 1, out, &st) == SUP_OK);
  double ops4 = 0.0;
  CHECK(sup_loop_torontonian_plan(4, nullptr, &ops4) == SUP_OK && st.est_ops_per_step == ops4);
  static_assert(SUP_LOOP_TORONTONIAN_MAX_DEVICE_N == 32, "the cap is every n the entry takes");
  // an exponent beyond the fp64 range: inf, no error code
  std::vector<double> big((size_t)4 * M, 0.0);
  big[0] = 80.0;
  int32_t first[1] = {0};
  CHECK(sup_loop_torontonian(O.data(), M, big.data(), first, 1, 1, &o, 1, out, nullptr) == SUP_OK && std::isinf(out[0]));
  // not positive definite: NaN, no error code
  O[2 * ((size_t)1 * 2 * M + 1)] = 1.5;
  CHECK(sup_loop_torontonian(O.data(), M, gm.data(), modes, 3, 1, &o, 1, out, nullptr) == SUP_OK && std::isnan(out[0]));
  int32_t clean[2] = {0, 2};
  CHECK(sup_loop_torontonian(O.data(), M, gm.data(), clean, 2, 1, &o, 1, out, nullptr) == SUP_OK && std::isfinite(out[0]));
}

static void test_exp() {
  const double inf = std::numeric_limits<double>::infinity();
  CHECK(same_bits(sup_ltor_exp(0.0), 1.0) && same_bits(sup_ltor_exp(-0.0), 1.0));
  CHECK(std::isnan(sup_ltor_exp(std::numeric_limits<double>::quiet_NaN())));
  CHECK(sup_ltor_exp(710.0) == inf && sup_ltor_exp(711.5) == inf && sup_ltor_exp(inf) == inf && sup_ltor_exp(1e308) == inf);
  CHECK(same_bits(sup_ltor_exp(-746.0), 0.0) && same_bits(sup_ltor_exp(-751.0), 0.0) && same_bits(sup_ltor_exp(-inf), 0.0));
  CHECK(sup_ltor_exp(-745.0) == std::numeric_limits<double>::denorm_min());
  CHECK(std::isfinite(sup_ltor_exp(709.78)) && sup_ltor_exp(709.78) > 1.7e308);
  CHECK(sup_ltor_exp(5e-324) == 1.0 && sup_ltor_exp(-5e-324) == 1.0);
  std::mt19937_64 g(47);
  std::uniform_real_distribution<double> d(-745.0, 709.0);
  for (int i = 0; i < 20000; ++i) {
    const double x = d(g), v = sup_ltor_exp(x), w = std::exp(x);
    CHECK(std::fabs(v - w) <= 2.0 * 2.220446049250313e-16 * w + std::numeric_limits<double>::denorm_min());
  }
  double out[2] = {0.0, 0.0}, x[2] = {0.0, 1.0};
  CHECK(sup_ltor_exp_device(nullptr, 2, out, 0) == SUP_EINVAL && sup_ltor_exp_device(x, 2, nullptr, 0) == SUP_EINVAL);
  CHECK(sup_ltor_exp_device(nullptr, 0, nullptr, 0) == SUP_OK);
}

int main() {
  test_values_and_bits();
  test_ranges();
  test_arguments();
  test_exp();
  std::printf("selftest_loop_torontonian: %s (%d failed checks)\n", failures ? "FAILED" : "ok", failures);
  return failures ? 1 : 0;
}
