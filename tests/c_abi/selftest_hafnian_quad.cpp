// selftest_hafnian_quad.cpp — host-code self test of the double-double hafnian
// entry points for the sanitizer builds (make -C superman_amd/csrc
// sanitize-hafnian-quad: AddressSanitizer + UndefinedBehaviorSanitizer, and
// ThreadSanitizer).  No GPU is needed.  It drives, with on_cpu = 1 on 1 and 8
// host threads,
//   - sup_hafnian_complex_quad and sup_loop_hafnian_complex_quad at n = 1, 2, 7,
//     12 and one repeated list of order 14, with count 0, 1 and 7: every result
//     has the bits of the call on that matrix alone, the thread count and the
//     slab size change no bit, every pair is normalised, and hi + lo agrees
//     with the recursive definition within 1e-12 of the larger modulus;
//   - Gaussian-integer inputs, exactly; odd n without loop: zeros, no walk;
//   - the stats against sup_hafnian_complex_plan;
//   - every error path: null pointers, n, M, indices, symmetry, too many chunks.
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
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

// A symmetric M x M matrix (interleaved) and a vector mu; integers in {-1, 0, 1} when `ints`.
static void make_matrix(int M, unsigned seed, bool ints, std::vector<double>& A, std::vector<double>& mu) {
  std::mt19937_64 g(seed);
  std::normal_distribution<double> d(0.0, 1.0);
  auto draw = [&]() { return ints ? (double)((int)(g() % 3u) - 1) : d(g); };
  A.assign((size_t)2 * M * M, 0.0);
  mu.assign((size_t)2 * M, 0.0);
  for (int i = 0; i < M; ++i) {
    for (int j = 0; j <= i; ++j)
      for (int p = 0; p < 2; ++p) A[2 * ((size_t)i * M + j) + p] = A[2 * ((size_t)j * M + i) + p] = draw();
    mu[2 * i] = draw(), mu[2 * i + 1] = draw();
  }
}

// Lists of order n: matrix k draws from mod[k % 3] values (n = 14: four values at most, a repeated list).
static std::vector<int32_t> make_lists(int n, uint64_t count, int M, unsigned seed) {
  const int mod[3] = {2, n >= 14 ? 3 : M, 4};
  std::mt19937 g(seed);
  std::vector<int32_t> idx((size_t)(count ? count : 1) * n, 0);
  for (uint64_t k = 0; k < count; ++k)
    for (int j = 0; j < n; ++j) idx[k * n + j] = (int32_t)(g() % (unsigned)mod[k % 3]);
  return idx;
}

// The recursive definition on the gather by ix (mu null: the plain hafnian).
static cplx rec(const std::vector<double>& A, int M, const double* mu, std::vector<int32_t> ix) {
  if (ix.empty()) return cplx(1.0, 0.0);
  if (!mu && (ix.size() & 1)) return cplx(0.0, 0.0);
  const int32_t a = ix[0];
  std::vector<int32_t> rest(ix.begin() + 1, ix.end());
  cplx s = mu ? cplx(mu[2 * a], mu[2 * a + 1]) * rec(A, M, mu, rest) : cplx(0.0, 0.0);
  for (size_t j = 0; j < rest.size(); ++j) {
    std::vector<int32_t> r2(rest);
    r2.erase(r2.begin() + (long)j);
    const double* e = &A[2 * ((size_t)a * M + rest[j])];
    s += cplx(e[0], e[1]) * rec(A, M, mu, r2);
  }
  return s;
}

static int call(bool loop, const std::vector<double>& A, int M, const std::vector<double>& mu, const int32_t* idx,
                int n, uint64_t count, const sup_opts* o, double* out, sup_stats* st) {
  return loop ? sup_loop_hafnian_complex_quad(A.data(), M, mu.data(), idx, n, count, o, 1, out, st)
              : sup_hafnian_complex_quad(A.data(), M, idx, n, count, o, 1, out, st);
}

static void test_values_and_bits() {
  const int M = 12;
  std::vector<double> A, mu;
  make_matrix(M, 9, false, A, mu);
  for (int loop = 0; loop < 2; ++loop)
    for (int n : {1, 2, 7, 12, 14})
      for (uint64_t count : {(uint64_t)0, (uint64_t)1, (uint64_t)7}) {
        const std::vector<int32_t> idx = make_lists(n, count, M, 70u + (unsigned)n);
        std::vector<uint64_t> terms(count + 1, 0);
        CHECK(sup_hafnian_complex_plan(idx.data(), n, count, terms.data()) == SUP_OK);
        uint64_t sum_terms = 0;
        for (uint64_t k = 0; k < count; ++k) sum_terms += terms[k];
        const bool zero = !loop && (n & 1);
        const sup_opts o1 = opts(1);
        std::vector<double> alone(4 * (size_t)count, 0.0);
        for (uint64_t k = 0; k < count; ++k)
          CHECK(call(loop, A, M, mu, idx.data() + k * n, n, 1, &o1, &alone[4 * k], nullptr) == SUP_OK);
        for (int threads : {1, 8})
          for (const char* slab : {"", "2"}) {
            setenv("SUP_HAFNIAN_SLAB", slab, 1);
            const sup_opts o = opts(threads);
            std::vector<double> out(4 * (size_t)count + 2, 42.0);  // two guard values behind the results
            sup_stats st;
            CHECK(call(loop, A, M, mu, idx.data(), n, count, &o, out.data(), &st) == SUP_OK);
            CHECK(out[4 * count] == 42.0 && out[4 * count + 1] == 42.0);
            out.resize(4 * (size_t)count);
            CHECK(same_bits(out, alone));
            CHECK(st.devices_used == 0 && st.leaves == (int)count && st.gray_steps == count << (n - 1));
            CHECK(st.visited_steps == (zero ? 0 : sum_terms));
            CHECK(zero || count == 0 || st.est_ops_per_step >= 188.0);
            for (uint64_t k = 0; k < count; ++k) {
              CHECK(out[4 * k] + out[4 * k + 1] == out[4 * k] && out[4 * k + 2] + out[4 * k + 3] == out[4 * k + 2]);
              if (zero) CHECK(out[4 * k] == 0.0 && out[4 * k + 1] == 0.0 && out[4 * k + 2] == 0.0 && out[4 * k + 3] == 0.0);
              if (n <= 7) {
                const cplx t = rec(A, M, loop ? mu.data() : nullptr,
                                   std::vector<int32_t>(idx.begin() + (long)(k * n), idx.begin() + (long)((k + 1) * n)));
                CHECK(std::abs(cplx(out[4 * k], out[4 * k + 2]) - t) <= 1e-12 * std::max(std::abs(t), 1.0));
              }
            }
          }
        unsetenv("SUP_HAFNIAN_SLAB");
      }
}

static void test_gaussian_integers() {
  const int M = 6, n = 8;
  std::vector<double> A, mu;
  make_matrix(M, 5, true, A, mu);
  const uint64_t count = 6;
  const std::vector<int32_t> idx = make_lists(n, count, M, 123);
  std::vector<double> out(4 * count);
  for (int loop = 0; loop < 2; ++loop)
    for (int threads : {1, 8}) {
      const sup_opts o = opts(threads);
      CHECK(call(loop, A, M, mu, idx.data(), n, count, &o, out.data(), nullptr) == SUP_OK);
      for (uint64_t k = 0; k < count; ++k) {
        const cplx t = rec(A, M, loop ? mu.data() : nullptr,
                           std::vector<int32_t>(idx.begin() + (long)(k * n), idx.begin() + (long)((k + 1) * n)));
        CHECK(std::nearbyint(out[4 * k]) == t.real() && std::nearbyint(out[4 * k + 2]) == t.imag());
        if (!loop)  // every operation of the plain form is exact on these inputs
          CHECK(out[4 * k] == t.real() && out[4 * k + 1] == 0.0 && out[4 * k + 2] == t.imag() && out[4 * k + 3] == 0.0);
      }
    }
  // the all-ones matrix, one group of 8: (n - 1)!! = 105
  std::vector<double> ones(2 * 2 * 2, 0.0);
  for (size_t i = 0; i < ones.size(); i += 2) ones[i] = 1.0;
  const int32_t i8[8] = {1, 1, 1, 1, 1, 1, 1, 1};
  double v[4] = {9, 9, 9, 9};
  CHECK(sup_hafnian_complex_quad(ones.data(), 2, i8, 8, 1, nullptr, 1, v, nullptr) == SUP_OK);
  CHECK(v[0] == 105.0 && v[1] == 0.0 && v[2] == 0.0 && v[3] == 0.0);
}

static void test_arguments() {
  std::vector<double> A, mu;
  make_matrix(64, 5, false, A, mu);
  double out[8] = {1, 1, 1, 1, 1, 1, 1, 1};
  auto untouched = [&]() {
    for (double x : out)
      if (x != 1) return false;
    return true;
  };
  int32_t idx[4] = {0, 1, 2, 0};
  CHECK(sup_hafnian_complex_quad(nullptr, 3, idx, 2, 2, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(std::strstr(sup_last_error(), "sup_hafnian_complex_quad: null pointer") != nullptr);
  CHECK(sup_hafnian_complex_quad(A.data(), 64, nullptr, 2, 2, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_hafnian_complex_quad(A.data(), 64, idx, 2, 2, nullptr, 1, nullptr, nullptr) == SUP_EINVAL);
  CHECK(sup_loop_hafnian_complex_quad(A.data(), 64, nullptr, idx, 2, 2, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(std::strstr(sup_last_error(), "sup_loop_hafnian_complex_quad: null pointer") != nullptr);
  CHECK(sup_hafnian_complex_quad(A.data(), 0, idx, 2, 2, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_hafnian_complex_quad(A.data(), 64, idx, 0, 2, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_hafnian_complex_quad(A.data(), 64, idx, 65, 2, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_hafnian_complex_quad(A.data(), 64, idx, 2, 0, nullptr, 1, out, nullptr) == SUP_OK);
  CHECK(untouched());  // nothing written
  idx[3] = 64;  // k = 1, position 1, M = 64
  CHECK(sup_hafnian_complex_quad(A.data(), 64, idx, 2, 2, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(std::strstr(sup_last_error(), "idx[k = 1][position 1] = 64") != nullptr);
  idx[3] = 0, idx[2] = -1;  // k = 1, position 0
  CHECK(sup_loop_hafnian_complex_quad(A.data(), 64, mu.data(), idx, 2, 2, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(std::strstr(sup_last_error(), "idx[k = 1][position 0] = -1") != nullptr);
  idx[2] = 2;
  // 42 distinct indices: 2^25 wave-chunks, refused before any work
  std::vector<int32_t> id(42);
  for (int j = 0; j < 42; ++j) id[j] = j;
  CHECK(sup_hafnian_complex_quad(A.data(), 64, id.data(), 42, 1, nullptr, 1, out, nullptr) == SUP_EUNSUPPORTED);
  CHECK(sup_loop_hafnian_complex_quad(A.data(), 64, mu.data(), id.data(), 42, 1, nullptr, 1, out, nullptr) ==
        SUP_EUNSUPPORTED);
  // one asymmetric pair
  const double kept = A[2 * (5 * 64 + 9) + 1];
  A[2 * (5 * 64 + 9) + 1] += 1.0;
  CHECK(sup_hafnian_complex_quad(A.data(), 64, idx, 2, 2, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(std::strstr(sup_last_error(), "A[5][9] and A[9][5] differ") != nullptr);
  CHECK(untouched());
  A[2 * (5 * 64 + 9) + 1] = kept;
  CHECK(sup_hafnian_complex_quad(A.data(), 64, idx, 2, 2, nullptr, 1, out, nullptr) == SUP_OK);
  CHECK(!untouched());
  static_assert(SUP_HAFNIAN_QUAD_MAX_DEVICE_N >= 1 && SUP_HAFNIAN_QUAD_MAX_DEVICE_N <= 64, "the cap is an order");
}

int main() {
  test_values_and_bits();
  test_gaussian_integers();
  test_arguments();
  std::printf("selftest_hafnian_quad: %s (%d failed checks)\n", failures ? "FAILED" : "ok", failures);
  return failures ? 1 : 0;
}
