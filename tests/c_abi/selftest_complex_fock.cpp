// selftest_complex_fock.cpp — host-code self test of the collision-aware
// complex entry points for the sanitizer builds (make -C superman_amd/csrc
// sanitize-complex-fock: AddressSanitizer + UndefinedBehaviorSanitizer, and
// ThreadSanitizer).  No GPU is needed.  It drives, with on_cpu = 1 on 1 and 8
// host threads,
//   - sup_perman_complex_fock at n = 1, 7, 12 with count 0, 1 and 5, index
//     lists that repeat on the rows, on the columns and on neither (both
//     sides get collapsed): every result agrees with
//     sup_perman_complex_submatrices within 1e-12 of the larger modulus, has
//     the bits of the call on that matrix alone, and the thread count and the
//     slab size change no bit;
//   - Gaussian-integer inputs against the submatrix entry, exactly;
//   - sup_perman_complex_fock_plan: terms, side, null outputs, and the stats
//     of the walk against it;
//   - the argument and index checks.
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

static sup_opts opts(int threads) {
  sup_opts o;
  sup_opts_init(&o);
  o.threads = threads;
  return o;
}

// Lists of order n for `count` matrices: matrix k draws its rows from
// rmod[k % 3] values and its columns from cmod[k % 3].
static void make_lists(int n, uint64_t count, int R, int C, unsigned seed, std::vector<int32_t>& rows,
                       std::vector<int32_t>& cols) {
  const int rmod[3] = {2, R, 3}, cmod[3] = {C, 2, 3};
  std::mt19937 g(seed);
  rows.assign((size_t)(count ? count : 1) * n, 0);
  cols.assign((size_t)(count ? count : 1) * n, 0);
  for (uint64_t k = 0; k < count; ++k)
    for (int j = 0; j < n; ++j) {
      rows[k * n + j] = (int32_t)(g() % (unsigned)rmod[k % 3]);
      cols[k * n + j] = (int32_t)(g() % (unsigned)cmod[k % 3]);
    }
}

static void test_values_and_bits() {
  const int R = 13, C = 14;
  const std::vector<double> U = random_doubles((size_t)2 * R * C, 9);
  bool side_seen[2] = {false, false};
  for (int n : {1, 7, 12})
    for (uint64_t count : {(uint64_t)0, (uint64_t)1, (uint64_t)5}) {
      std::vector<int32_t> rows, cols;
      make_lists(n, count, R, C, 70u + (unsigned)n, rows, cols);
      std::vector<uint64_t> terms(count + 1, 0);
      std::vector<int> side(count + 1, -1);
      CHECK(sup_perman_complex_fock_plan(rows.data(), cols.data(), n, count, terms.data(), side.data()) == SUP_OK);
      uint64_t sum_terms = 0;
      for (uint64_t k = 0; k < count; ++k) {
        CHECK(terms[k] >= 1 && terms[k] <= (1ull << (n - 1)) && (side[k] == 0 || side[k] == 1));
        sum_terms += terms[k];
        side_seen[side[k]] = true;
      }
      const sup_opts o1 = opts(1);
      std::vector<double> sub(2 * (size_t)count + 2, 0.0), alone(2 * (size_t)count, 0.0);  // never a null pointer
      CHECK(sup_perman_complex_submatrices(U.data(), R, C, rows.data(), cols.data(), n, count, &o1, 1, sub.data(),
                                           nullptr) == SUP_OK);
      for (uint64_t k = 0; k < count; ++k)
        CHECK(sup_perman_complex_fock(U.data(), R, C, rows.data() + k * n, cols.data() + k * n, n, 1, &o1, 1,
                                      &alone[2 * k], nullptr) == SUP_OK);
      for (int threads : {1, 8})
        for (const char* slab : {"", "2"}) {
          setenv("SUP_CPLX_FOCK_SLAB", slab, 1);
          const sup_opts o = opts(threads);
          std::vector<double> out(2 * (size_t)count + 2, 42.0);  // two guard values behind the results
          sup_stats st;
          CHECK(sup_perman_complex_fock(U.data(), R, C, rows.data(), cols.data(), n, count, &o, 1, out.data(), &st) ==
                SUP_OK);
          CHECK(out[2 * count] == 42.0 && out[2 * count + 1] == 42.0);
          out.resize(2 * (size_t)count);
          CHECK(same_bits(out, alone));
          for (uint64_t k = 0; k < count; ++k) {
            const double mod = std::hypot(sub[2 * k], sub[2 * k + 1]);
            CHECK(std::hypot(out[2 * k] - sub[2 * k], out[2 * k + 1] - sub[2 * k + 1]) <= 1e-12 * mod);
          }
          CHECK(st.devices_used == 0 && st.leaves == (int)count && st.gray_steps == count << (n - 1));
          CHECK(st.visited_steps == sum_terms && st.est_ops_per_step == 6.0 * n);
        }
      unsetenv("SUP_CPLX_FOCK_SLAB");
    }
  CHECK(side_seen[0] && side_seen[1]);
}

static void test_gaussian_integers() {
  const int R = 6, C = 6, n = 7;
  std::mt19937 g(5);
  std::vector<double> U((size_t)2 * R * C);
  for (auto& v : U) v = (double)((int)(g() % 3u) - 1);
  const uint64_t count = 5;
  std::vector<int32_t> rows, cols;
  make_lists(n, count, R, C, 123, rows, cols);
  std::vector<double> sub(2 * count), out(2 * count);
  // both walks are exact on these inputs (tests/test_complex_fock.py), so they agree to the bit
  CHECK(sup_perman_complex_submatrices(U.data(), R, C, rows.data(), cols.data(), n, count, nullptr, 1, sub.data(),
                                       nullptr) == SUP_OK);
  for (int threads : {1, 8}) {
    const sup_opts o = opts(threads);
    CHECK(sup_perman_complex_fock(U.data(), R, C, rows.data(), cols.data(), n, count, &o, 1, out.data(), nullptr) ==
          SUP_OK);
    for (size_t i = 0; i < out.size(); ++i) CHECK(out[i] == sub[i]);
  }
  // every row the same row of the all-ones matrix: n!, one group on either side
  std::vector<double> ones(2 * 3 * 3, 0.0);
  for (size_t i = 0; i < ones.size(); i += 2) ones[i] = 1.0;
  const int32_t r6[6] = {2, 2, 2, 2, 2, 2}, c6[6] = {0, 1, 2, 0, 1, 2};
  double v[2] = {0, 0};
  CHECK(sup_perman_complex_fock(ones.data(), 3, 3, r6, c6, 6, 1, nullptr, 1, v, nullptr) == SUP_OK);
  CHECK(v[0] == 720.0 && v[1] == 0.0);
}

static void test_plan() {
  const int32_t rows[7] = {0, 1, 2, 3, 4, 5, 6}, cols[7] = {0, 0, 1, 1, 1, 2, 2};
  uint64_t terms = 0;
  int side = -1;
  CHECK(sup_perman_complex_fock_plan(rows, cols, 7, 1, &terms, &side) == SUP_OK);
  CHECK(terms == 24 && side == 0);  // t' = (1, 3, 2)
  CHECK(sup_perman_complex_fock_plan(cols, rows, 7, 1, &terms, &side) == SUP_OK);
  CHECK(terms == 24 && side == 1);
  CHECK(sup_perman_complex_fock_plan(rows, rows, 7, 1, &terms, &side) == SUP_OK);
  CHECK(terms == 64 && side == 0);  // no repeats: 2^(n-1), a tie
  CHECK(sup_perman_complex_fock_plan(rows, cols, 7, 1, nullptr, &side) == SUP_OK);
  CHECK(sup_perman_complex_fock_plan(rows, cols, 7, 1, &terms, nullptr) == SUP_OK);
  CHECK(sup_perman_complex_fock_plan(rows, cols, 7, 0, nullptr, nullptr) == SUP_OK);
  CHECK(sup_perman_complex_fock_plan(nullptr, cols, 7, 1, &terms, &side) == SUP_EINVAL);
  CHECK(sup_perman_complex_fock_plan(rows, nullptr, 7, 1, &terms, &side) == SUP_EINVAL);
  CHECK(sup_perman_complex_fock_plan(rows, cols, 0, 1, &terms, &side) == SUP_EINVAL);
  CHECK(sup_perman_complex_fock_plan(rows, cols, 65, 1, &terms, &side) == SUP_EINVAL);
}

static void test_arguments() {
  const std::vector<double> a = random_doubles(2 * 64 * 64, 5);
  double out[4] = {1, 1, 1, 1};
  int32_t rows[4] = {0, 1, 2, 0}, cols[4] = {0, 0, 1, 2};
  CHECK(sup_perman_complex_fock(nullptr, 3, 3, rows, cols, 2, 2, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_perman_complex_fock(a.data(), 3, 3, nullptr, cols, 2, 2, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_perman_complex_fock(a.data(), 3, 3, rows, nullptr, 2, 2, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_perman_complex_fock(a.data(), 3, 3, rows, cols, 2, 2, nullptr, 1, nullptr, nullptr) == SUP_EINVAL);
  CHECK(sup_perman_complex_fock(a.data(), 0, 3, rows, cols, 2, 2, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_perman_complex_fock(a.data(), 3, 0, rows, cols, 2, 2, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_perman_complex_fock(a.data(), 3, 3, rows, cols, 0, 2, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_perman_complex_fock(a.data(), 3, 3, rows, cols, 65, 2, nullptr, 1, out, nullptr) == SUP_EINVAL);
  sup_opts o = opts(1);
  o.walk_log2 = 32;
  CHECK(sup_perman_complex_fock(a.data(), 3, 3, rows, cols, 2, 2, &o, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_perman_complex_fock(a.data(), 3, 3, rows, cols, 2, 0, nullptr, 1, out, nullptr) == SUP_OK);
  CHECK(out[0] == 1 && out[1] == 1);  // nothing written
  CHECK(sup_perman_complex_fock(a.data(), 3, 3, rows, cols, 2, 2, nullptr, 1, out, nullptr) == SUP_OK);
  rows[3] = 3;  // k = 1, position 1, R = 3
  CHECK(sup_perman_complex_fock(a.data(), 3, 3, rows, cols, 2, 2, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(std::strstr(sup_last_error(), "rows[k = 1][position 1] = 3") != nullptr);
  rows[3] = 0, cols[2] = -1;  // k = 1, position 0
  CHECK(sup_perman_complex_fock(a.data(), 3, 3, rows, cols, 2, 2, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(std::strstr(sup_last_error(), "cols[k = 1][position 0] = -1") != nullptr);
  // n = 64 without repeats: 2^63 terms, refused before any work
  std::vector<int32_t> id(64);
  for (int j = 0; j < 64; ++j) id[j] = j;
  CHECK(sup_perman_complex_fock(a.data(), 64, 64, id.data(), id.data(), 64, 1, nullptr, 1, out, nullptr) ==
        SUP_EUNSUPPORTED);
}

int main() {
  test_values_and_bits();
  test_gaussian_integers();
  test_plan();
  test_arguments();
  std::printf("selftest_complex_fock: %s (%d failed checks)\n", failures ? "FAILED" : "ok", failures);
  return failures ? 1 : 0;
}
