// selftest_hafnian_pt.cpp — host-code self test of the power-trace hafnian
// entry points for the sanitizer builds (make -C superman_amd/csrc
// sanitize-hafnian-pt: AddressSanitizer + UndefinedBehaviorSanitizer, and
// ThreadSanitizer).  No GPU is needed.  It drives, with on_cpu = 1 on 1 and 8
// host threads,
//   - sup_hafnian_complex_pt and sup_loop_hafnian_complex_pt at n = 1, 6, 9, 14
//     with count 0, 1 and 9 (matrices shared among the threads) and at n = 20
//     with count 1 (subsets shared among the threads): every result has the
//     bits of the call on that matrix alone on one thread; small orders agree
//     with the recursive definition and every order with sup_hafnian_complex;
//   - sup_hafnian_complex_pt_range: whole, split and empty ranges, and n = 64
//     (2^14 subsets per wave-chunk) at both ends of the subsets;
//   - sup_hafnian_complex_pt_plan and the stats against it;
//   - the argument, symmetry, index and range checks, and the device cap.
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

// A symmetric M x M matrix (interleaved) and a vector mu.
static void make_matrix(int M, unsigned seed, double scale, std::vector<double>& A, std::vector<double>& mu) {
  std::mt19937_64 g(seed);
  std::normal_distribution<double> d(0.0, scale);
  A.assign((size_t)2 * M * M, 0.0);
  mu.assign((size_t)2 * M, 0.0);
  for (int i = 0; i < M; ++i) {
    for (int j = 0; j <= i; ++j)
      for (int p = 0; p < 2; ++p) A[2 * ((size_t)i * M + j) + p] = A[2 * ((size_t)j * M + i) + p] = d(g);
    mu[2 * i] = d(g), mu[2 * i + 1] = d(g);
  }
}

// Lists of order n: matrix k draws from mod[k % 3] values.
static std::vector<int32_t> make_lists(int n, uint64_t count, int M, unsigned seed) {
  const int mod[3] = {2, M, 4};
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
  return loop ? sup_loop_hafnian_complex_pt(A.data(), M, mu.data(), idx, n, count, o, 1, out, st)
              : sup_hafnian_complex_pt(A.data(), M, idx, n, count, o, 1, out, st);
}

static void test_values_and_bits() {
  const int M = 11;
  std::vector<double> A, mu;
  make_matrix(M, 9, 1.0, A, mu);
  for (int loop = 0; loop < 2; ++loop)
    for (int n : {1, 6, 9, 14, 20})
      for (uint64_t count : {(uint64_t)0, (uint64_t)1, (uint64_t)9}) {
        if (n == 20 && count != 1) continue;
        const std::vector<int32_t> idx = make_lists(n, count, M, 70u + (unsigned)n);
        uint64_t subsets = 7;
        double ops = -1.0;
        CHECK(sup_hafnian_complex_pt_plan(n, loop, &subsets, &ops) == SUP_OK);
        const bool zero = !loop && (n & 1);
        CHECK(subsets == (zero ? 0 : (1ull << ((n + 1) / 2)) - 1));
        const sup_opts o1 = opts(1);
        std::vector<double> alone(2 * (size_t)count, 0.0);
        for (uint64_t k = 0; k < count; ++k)
          CHECK(call(loop, A, M, mu, idx.data() + k * n, n, 1, &o1, &alone[2 * k], nullptr) == SUP_OK);
        for (int threads : {1, 8}) {
          const sup_opts o = opts(threads);
          std::vector<double> out(2 * (size_t)count + 2, 42.0);  // two guard values behind the results
          sup_stats st;
          CHECK(call(loop, A, M, mu, idx.data(), n, count, &o, out.data(), &st) == SUP_OK);
          CHECK(out[2 * count] == 42.0 && out[2 * count + 1] == 42.0);
          out.resize(2 * (size_t)count);
          CHECK(same_bits(out, alone));
          CHECK(st.devices_used == 0 && st.leaves == (int)count && st.gray_steps == count << (n - 1));
          CHECK(st.visited_steps == count * subsets);
          if (count && !zero) CHECK(st.est_ops_per_step == ops);
          for (uint64_t k = 0; k < count; ++k) {
            const cplx v(out[2 * k], out[2 * k + 1]);
            if (zero) CHECK(out[2 * k] == 0.0 && out[2 * k + 1] == 0.0);
            if (n <= 9) {
              const cplx t = rec(A, M, loop ? mu.data() : nullptr,
                                 std::vector<int32_t>(idx.begin() + (long)(k * n), idx.begin() + (long)((k + 1) * n)));
              CHECK(std::abs(v - t) <= 1e-12 * std::max(std::abs(t), 1.0));
            }
            double kan[2] = {0, 0};
            CHECK((loop ? sup_loop_hafnian_complex(A.data(), M, mu.data(), idx.data() + k * n, n, 1, &o, 1, kan, nullptr)
                        : sup_hafnian_complex(A.data(), M, idx.data() + k * n, n, 1, &o, 1, kan, nullptr)) == SUP_OK);
            CHECK(std::abs(v - cplx(kan[0], kan[1])) <= 1e-9 * std::max(std::abs(v), 1.0));
          }
        }
      }
}

static void test_ranges() {
  const int M = 12, n = 12;  // m = 6: one subset per wave-chunk
  std::vector<double> A, mu;
  make_matrix(M, 4, 1.0, A, mu);
  std::vector<int32_t> idx(n);
  for (int j = 0; j < n; ++j) idx[j] = j;
  for (int loop = 0; loop < 2; ++loop) {
    const double* m = loop ? mu.data() : nullptr;
    for (int threads : {1, 8}) {
      const sup_opts o = opts(threads);
      double whole[2], full[2], a[2], b[2], none[2] = {7, 7};
      sup_stats st;
      CHECK(call(loop, A, M, mu, idx.data(), n, 1, &o, whole, nullptr) == SUP_OK);
      CHECK(sup_hafnian_complex_pt_range(A.data(), M, m, idx.data(), n, 0, 64, &o, 1, full, &st) == SUP_OK);
      CHECK(std::memcmp(whole, full, sizeof whole) == 0 && st.visited_steps == 63);
      CHECK(sup_hafnian_complex_pt_range(A.data(), M, m, idx.data(), n, 0, 32, &o, 1, a, nullptr) == SUP_OK);
      CHECK(sup_hafnian_complex_pt_range(A.data(), M, m, idx.data(), n, 32, 64, &o, 1, b, &st) == SUP_OK);
      CHECK(a[0] + b[0] == whole[0] && a[1] + b[1] == whole[1] && st.visited_steps == 32);
      CHECK(sup_hafnian_complex_pt_range(A.data(), M, m, idx.data(), n, 9, 9, &o, 1, none, &st) == SUP_OK);
      CHECK(none[0] == 0.0 && none[1] == 0.0 && st.visited_steps == 0);
      CHECK(sup_hafnian_complex_pt_range(A.data(), M, m, idx.data(), n, 0, 1, &o, 1, none, nullptr) == SUP_OK);
      CHECK(none[0] == 0.0 && none[1] == 0.0);
    }
  }
  // n = 64: both ends of the 2^32 subsets, 1 and 8 threads, the same bits
  const int N = 64;
  make_matrix(N, 6, 0.125, A, mu);
  std::vector<int32_t> id(N);
  for (int j = 0; j < N; ++j) id[j] = j;
  for (int loop = 0; loop < 2; ++loop)
    for (uint64_t z0 : {(uint64_t)1, (uint64_t)((1ull << 32) - 12)}) {
      double r1[2], r8[2];
      const sup_opts o1 = opts(1), o8 = opts(8);
      CHECK(sup_hafnian_complex_pt_range(A.data(), N, loop ? mu.data() : nullptr, id.data(), N, z0, z0 + 12, &o1, 1, r1,
                                         nullptr) == SUP_OK);
      CHECK(sup_hafnian_complex_pt_range(A.data(), N, loop ? mu.data() : nullptr, id.data(), N, z0, z0 + 12, &o8, 1, r8,
                                         nullptr) == SUP_OK);
      CHECK(std::memcmp(r1, r8, sizeof r1) == 0 && std::isfinite(r1[0]) && std::isfinite(r1[1]));
    }
}

static void test_arguments() {
  std::vector<double> A, mu;
  make_matrix(64, 5, 1.0, A, mu);
  double out[4] = {1, 1, 1, 1};
  int32_t idx[4] = {0, 1, 2, 0};
  CHECK(sup_hafnian_complex_pt(nullptr, 3, idx, 2, 2, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_hafnian_complex_pt(A.data(), 64, nullptr, 2, 2, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_hafnian_complex_pt(A.data(), 64, idx, 2, 2, nullptr, 1, nullptr, nullptr) == SUP_EINVAL);
  CHECK(sup_loop_hafnian_complex_pt(A.data(), 64, nullptr, idx, 2, 2, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_hafnian_complex_pt(A.data(), 0, idx, 2, 2, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_hafnian_complex_pt(A.data(), 64, idx, 0, 2, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_hafnian_complex_pt(A.data(), 64, idx, 65, 2, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_hafnian_complex_pt(A.data(), 64, idx, 2, 0, nullptr, 1, out, nullptr) == SUP_OK);
  CHECK(out[0] == 1 && out[1] == 1);  // nothing written
  CHECK(sup_hafnian_complex_pt(A.data(), 64, idx, 2, 2, nullptr, 1, out, nullptr) == SUP_OK);
  CHECK(sup_hafnian_complex_pt_range(A.data(), 64, nullptr, idx, 4, 3, 2, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_hafnian_complex_pt_range(A.data(), 64, nullptr, idx, 4, 0, 5, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(std::strstr(sup_last_error(), "subsets [0, 5)") != nullptr);
  CHECK(sup_hafnian_complex_pt_plan(0, 0, nullptr, nullptr) == SUP_EINVAL);
  CHECK(sup_hafnian_complex_pt_plan(65, 1, nullptr, nullptr) == SUP_EINVAL);
  CHECK(sup_hafnian_complex_pt_plan(64, 1, nullptr, nullptr) == SUP_OK);
  idx[3] = 64;  // k = 1, position 1, M = 64
  CHECK(sup_hafnian_complex_pt(A.data(), 64, idx, 2, 2, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(std::strstr(sup_last_error(), "idx[k = 1][position 1] = 64") != nullptr);
  idx[3] = 0, idx[2] = -1;  // k = 1, position 0
  CHECK(sup_loop_hafnian_complex_pt(A.data(), 64, mu.data(), idx, 2, 2, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(std::strstr(sup_last_error(), "idx[k = 1][position 0] = -1") != nullptr);
  idx[2] = 2;
  // above the device cap: refused before the device is looked for
  std::vector<int32_t> id(SUP_HAFNIAN_PT_MAX_DEVICE_N + 1);
  for (size_t j = 0; j < id.size(); ++j) id[j] = (int32_t)j;
  if (SUP_HAFNIAN_PT_MAX_DEVICE_N < 64) {
    CHECK(sup_hafnian_complex_pt_range(A.data(), 64, nullptr, id.data(), (int)id.size(), 1, 2, nullptr, 0, out, nullptr) ==
          SUP_EUNSUPPORTED);
    CHECK(std::strstr(sup_last_error(), "above the device cap") != nullptr);
  }
  // one asymmetric pair
  A[2 * (5 * 64 + 9) + 1] += 1.0;
  CHECK(sup_hafnian_complex_pt(A.data(), 64, idx, 2, 2, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(std::strstr(sup_last_error(), "A[5][9] and A[9][5] differ") != nullptr);
}

int main() {
  test_values_and_bits();
  test_ranges();
  test_arguments();
  std::printf("selftest_hafnian_pt: %s (%d failed checks)\n", failures ? "FAILED" : "ok", failures);
  return failures ? 1 : 0;
}
