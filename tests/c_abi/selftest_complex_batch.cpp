// selftest_complex_batch.cpp — host-code self test of the batched complex
// entry points for the sanitizer builds (make -C superman_amd/csrc
// sanitize-complex-batch: AddressSanitizer + UndefinedBehaviorSanitizer, and
// ThreadSanitizer).  No GPU is needed.  It drives, with on_cpu = 1 on 1 and 8
// host threads,
//   - sup_perman_complex_batch at n = 1, 7, 12 with count 0, 1 and 5: every
//     result has the bits of sup_perman_complex on that matrix alone, and the
//     thread count changes no bit (5 < 8: the threads share a matrix's chunks;
//     5 >= 1: they are spread over the matrices);
//   - sup_perman_complex_submatrices with repeated rows and columns against
//     the batch of the gathered matrices, and the all-ones matrix (n!);
//   - the argument and index checks.
#include <cmath>
#include <cstdio>
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

static std::vector<double> random_doubles(size_t count, unsigned seed) {
  std::mt19937_64 g(seed);
  std::normal_distribution<double> d(0.0, 1.0);
  std::vector<double> a(count);
  for (auto& v : a) v = d(g);
  return a;
}

static bool same_bits(const std::vector<double>& a, const std::vector<double>& b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0);
}

static sup_opts opts(int threads, int walk_log2) {
  sup_opts o;
  sup_opts_init(&o);
  o.threads = threads;
  o.walk_log2 = walk_log2;
  return o;
}

static void test_batch() {
  for (int n : {1, 7, 12})
    for (uint64_t count : {(uint64_t)0, (uint64_t)1, (uint64_t)5})
      for (int wl : {0, 2}) {
        const size_t per = (size_t)2 * n * n;
        const std::vector<double> mats = random_doubles(per * (size_t)(count ? count : 1), 300u + (unsigned)n);
        std::vector<double> alone(2 * (size_t)count, 0.0);
        for (uint64_t k = 0; k < count; ++k) {
          const sup_opts o = opts(1, wl);
          CHECK(sup_perman_complex(mats.data() + k * per, n, &o, 1, &alone[2 * k], &alone[2 * k + 1], nullptr) ==
                SUP_OK);
        }
        for (int threads : {1, 8}) {
          const sup_opts o = opts(threads, wl);
          std::vector<double> out(2 * (size_t)count + 2, 42.0);  // two guard values behind the results
          sup_stats st;
          CHECK(sup_perman_complex_batch(mats.data(), n, count, &o, 1, out.data(), &st) == SUP_OK);
          CHECK(out[2 * count] == 42.0 && out[2 * count + 1] == 42.0);
          out.resize(2 * (size_t)count);
          CHECK(same_bits(out, alone));
          CHECK(st.devices_used == 0 && st.leaves == (int)count && st.gray_steps == count << (n - 1));
          CHECK(st.est_ops_per_step == 6.0 * n);
        }
      }
}

static void test_submatrices() {
  const int R = 5, C = 7;
  const std::vector<double> U = random_doubles((size_t)2 * R * C, 9);
  for (int n : {1, 7, 12}) {
    const uint64_t count = 5;
    std::mt19937 g(77u + (unsigned)n);
    std::vector<int32_t> rows(count * n), cols(count * n);  // n > R: rows must repeat
    for (auto& r : rows) r = (int32_t)(g() % R);
    for (auto& c : cols) c = (int32_t)(g() % C);
    if (n > 1) rows[1] = rows[0], cols[n - 1] = cols[0];
    std::vector<double> gathered(count * 2 * n * n);
    for (uint64_t k = 0; k < count; ++k)
      for (int j = 0; j < n; ++j)
        for (int c = 0; c < n; ++c)
          for (int part = 0; part < 2; ++part)
            gathered[2 * ((k * n + j) * n + c) + part] = U[2 * ((size_t)rows[k * n + j] * C + cols[k * n + c]) + part];
    std::vector<double> want(2 * count);
    const sup_opts o1 = opts(1, 0);
    CHECK(sup_perman_complex_batch(gathered.data(), n, count, &o1, 1, want.data(), nullptr) == SUP_OK);
    for (int threads : {1, 8}) {
      const sup_opts o = opts(threads, 0);
      std::vector<double> out(2 * count);
      CHECK(sup_perman_complex_submatrices(U.data(), R, C, rows.data(), cols.data(), n, count, &o, 1, out.data(),
                                           nullptr) == SUP_OK);
      CHECK(same_bits(out, want));
    }
  }
  // every row the same row of the all-ones matrix: n!
  const std::vector<double> ones = [] {
    std::vector<double> u(2 * 3 * 3, 0.0);
    for (size_t i = 0; i < u.size(); i += 2) u[i] = 1.0;
    return u;
  }();
  const int32_t rows[6] = {2, 2, 2, 2, 2, 2}, cols[6] = {0, 1, 2, 0, 1, 2};
  double out[2] = {0, 0};
  CHECK(sup_perman_complex_submatrices(ones.data(), 3, 3, rows, cols, 6, 1, nullptr, 1, out, nullptr) == SUP_OK);
  CHECK(out[0] == 720.0 && out[1] == 0.0);
}

static void test_arguments() {
  const std::vector<double> a = random_doubles(2 * 7 * 7 * 2, 5);
  double out[4] = {1, 1, 1, 1};
  CHECK(sup_perman_complex_batch(nullptr, 7, 2, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_perman_complex_batch(a.data(), 7, 2, nullptr, 1, nullptr, nullptr) == SUP_EINVAL);
  CHECK(sup_perman_complex_batch(a.data(), 0, 2, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_perman_complex_batch(a.data(), 65, 2, nullptr, 1, out, nullptr) == SUP_EINVAL);
  sup_opts o = opts(1, 32);
  CHECK(sup_perman_complex_batch(a.data(), 7, 2, &o, 1, out, nullptr) == SUP_EINVAL);
  o.walk_log2 = -1;
  CHECK(sup_perman_complex_batch(a.data(), 7, 2, &o, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_perman_complex_batch(a.data(), 7, 0, nullptr, 1, out, nullptr) == SUP_OK);
  CHECK(out[0] == 1 && out[1] == 1);  // nothing written

  int32_t rows[4] = {0, 1, 2, 0}, cols[4] = {0, 0, 1, 2};
  CHECK(sup_perman_complex_submatrices(nullptr, 3, 3, rows, cols, 2, 2, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_perman_complex_submatrices(a.data(), 3, 3, nullptr, cols, 2, 2, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_perman_complex_submatrices(a.data(), 3, 3, rows, nullptr, 2, 2, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_perman_complex_submatrices(a.data(), 3, 3, rows, cols, 2, 2, nullptr, 1, nullptr, nullptr) == SUP_EINVAL);
  CHECK(sup_perman_complex_submatrices(a.data(), 0, 3, rows, cols, 2, 2, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_perman_complex_submatrices(a.data(), 3, 0, rows, cols, 2, 2, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_perman_complex_submatrices(a.data(), 3, 3, rows, cols, 2, 2, nullptr, 1, out, nullptr) == SUP_OK);
  rows[3] = 3;  // k = 1, position 1, R = 3
  CHECK(sup_perman_complex_submatrices(a.data(), 3, 3, rows, cols, 2, 2, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(std::strstr(sup_last_error(), "rows[k = 1][position 1] = 3") != nullptr);
  rows[3] = 0, cols[2] = -1;  // k = 1, position 0
  CHECK(sup_perman_complex_submatrices(a.data(), 3, 3, rows, cols, 2, 2, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(std::strstr(sup_last_error(), "cols[k = 1][position 0] = -1") != nullptr);
}

int main() {
  test_batch();
  test_submatrices();
  test_arguments();
  std::printf("selftest_complex_batch: %s (%d failed checks)\n", failures ? "FAILED" : "ok", failures);
  return failures ? 1 : 0;
}
