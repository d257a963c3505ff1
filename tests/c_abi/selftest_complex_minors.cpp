// selftest_complex_minors.cpp — host-code self test of the one-walk minors and
// the boson sampler for the sanitizer builds (make -C superman_amd/csrc
// sanitize-complex-minors: AddressSanitizer + UndefinedBehaviorSanitizer, and
// ThreadSanitizer).  No GPU is needed.  It drives, with on_cpu = 1 on 1 and 8
// host threads,
//   - sup_perman_complex_minors at n = 1, 2, 7, 12 with count 0, 1 and 5 and
//     index lists that repeat: every result agrees with
//     sup_perman_complex_submatrices on the materialised minor within 1e-11 of
//     the sum of the moduli, has the bits of the call on that matrix alone, and
//     the thread count and the slab size change no bit;
//   - sup_perman_complex_minors_range: aligned halves fold to the whole;
//   - sup_boson_sample: 50 samples, sorted rows in range, the same on 1 and 8
//     threads and as a prefix of a longer run;
//   - every argument and index check of the three entries.
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

// rows (count x n) and cols (count x (n-1)); every list with room repeats an entry
static void make_lists(int n, uint64_t count, int R, int C, unsigned seed, std::vector<int32_t>& rows,
                       std::vector<int32_t>& cols) {
  std::mt19937 g(seed);
  const int q = n - 1;
  rows.assign((size_t)(count ? count : 1) * n, 0);
  cols.assign((size_t)(count ? count : 1) * (q ? q : 1), 0);
  for (uint64_t k = 0; k < count; ++k) {
    for (int j = 0; j < n; ++j) rows[k * n + j] = (int32_t)(g() % (unsigned)R);
    for (int c = 0; c < q; ++c) cols[k * q + c] = (int32_t)(g() % (unsigned)C);
    if (n > 2) rows[k * n + n - 1] = rows[k * n], cols[k * q + 1] = cols[k * q];
  }
}

static void test_values_and_bits() {
  const int R = 13, C = 14;
  const std::vector<double> U = random_doubles((size_t)2 * R * C, 9);
  for (int n : {1, 2, 7, 12})
    for (uint64_t count : {(uint64_t)0, (uint64_t)1, (uint64_t)5}) {
      const int q = n - 1;
      std::vector<int32_t> rows, cols;
      make_lists(n, count, R, C, 70u + (unsigned)n, rows, cols);
      const sup_opts o1 = opts(1);
      // the materialised minors through the submatrix entry (q >= 1), and each matrix alone
      std::vector<double> ref(2 * (size_t)count * n + 2, 0.0), alone(2 * (size_t)count * n, 0.0);
      for (uint64_t k = 0; k < count; ++k) {
        for (int j = 0; j < n && q >= 1; ++j) {
          std::vector<int32_t> mr;
          for (int i = 0; i < n; ++i)
            if (i != j) mr.push_back(rows[k * n + i]);
          CHECK(sup_perman_complex_submatrices(U.data(), R, C, mr.data(), cols.data() + k * q, q, 1, &o1, 1,
                                               &ref[2 * (k * n + j)], nullptr) == SUP_OK);
        }
        CHECK(sup_perman_complex_minors(U.data(), R, C, rows.data() + k * n, cols.data() + k * q, n, 1, &o1, 1,
                                        &alone[2 * k * n], nullptr) == SUP_OK);
      }
      for (int threads : {1, 8})
        for (const char* slab : {"", "2"}) {
          setenv("SUP_CPLX_MINORS_SLAB", slab, 1);
          const sup_opts o = opts(threads);
          std::vector<double> out(2 * (size_t)count * n + 2, 42.0);  // two guard values behind the results
          sup_stats st;
          CHECK(sup_perman_complex_minors(U.data(), R, C, rows.data(), cols.data(), n, count, &o, 1, out.data(), &st) ==
                SUP_OK);
          CHECK(out[2 * count * n] == 42.0 && out[2 * count * n + 1] == 42.0);
          out.resize(2 * (size_t)count * n);
          CHECK(same_bits(out, alone));
          for (uint64_t i = 0; i < count * n; ++i) {
            if (q == 0) {
              CHECK(out[2 * i] == 1.0 && out[2 * i + 1] == 0.0);
              continue;
            }
            const double mod = std::hypot(ref[2 * i], ref[2 * i + 1]) + std::hypot(out[2 * i], out[2 * i + 1]);
            CHECK(std::hypot(out[2 * i] - ref[2 * i], out[2 * i + 1] - ref[2 * i + 1]) <= 1e-11 * mod);
          }
          CHECK(st.devices_used == 0 && st.leaves == (int)(count * n));
          CHECK(st.gray_steps == (n >= 2 ? count << (n - 2) : 0));
          CHECK(st.est_ops_per_step == (n >= 2 ? 16.0 * n - 24.0 : 0.0));
        }
      unsetenv("SUP_CPLX_MINORS_SLAB");
    }
  // n = 1 takes no column list
  double one[2] = {0, 0};
  const int32_t r0[1] = {3};
  CHECK(sup_perman_complex_minors(U.data(), R, C, r0, nullptr, 1, 1, nullptr, 1, one, nullptr) == SUP_OK);
  CHECK(one[0] == 1.0 && one[1] == 0.0);
}

static void test_range() {
  const int n = 12, q = 11;
  const std::vector<double> B = random_doubles((size_t)2 * n * q, 21);
  std::vector<int32_t> rows(n), cols(q);
  for (int j = 0; j < n; ++j) rows[j] = j;
  for (int c = 0; c < q; ++c) cols[c] = c;
  for (int threads : {1, 8}) {
    sup_opts o = opts(threads);
    o.walk_log2 = 2;  // order 11: L = 6, m = 2, 4 wave-chunks
    std::vector<double> whole(2 * n), lo(2 * n), hi(2 * n), all(2 * n);
    sup_stats st;
    CHECK(sup_perman_complex_minors(B.data(), n, q, rows.data(), cols.data(), n, 1, &o, 1, whole.data(), nullptr) ==
          SUP_OK);
    CHECK(sup_perman_complex_minors_range(B.data(), n, 0, 2, &o, 1, lo.data(), &st) == SUP_OK);
    CHECK(st.gray_steps == 2ull << 8 && st.walk_bits == 2 && st.lane_bits == 6);
    CHECK(sup_perman_complex_minors_range(B.data(), n, 2, 4, &o, 1, hi.data(), nullptr) == SUP_OK);
    CHECK(sup_perman_complex_minors_range(B.data(), n, 0, 4, &o, 1, all.data(), nullptr) == SUP_OK);
    const double f = 4.0 * (q & 1) - 2.0;
    for (int i = 0; i < 2 * n; ++i) {
      CHECK(f * (lo[i] + hi[i]) == whole[i]);
      CHECK(f * all[i] == whole[i]);
    }
    CHECK(sup_perman_complex_minors_range(B.data(), n, 1, 1, &o, 1, all.data(), nullptr) == SUP_OK);  // empty: zeros
    CHECK(all[0] == 0.0 && all[2 * n - 1] == 0.0);
    CHECK(sup_perman_complex_minors_range(B.data(), n, 3, 2, &o, 1, all.data(), nullptr) == SUP_EINVAL);
    CHECK(sup_perman_complex_minors_range(B.data(), n, 0, 5, &o, 1, all.data(), nullptr) == SUP_EINVAL);
  }
  double out[2 * 33];
  CHECK(sup_perman_complex_minors_range(nullptr, n, 0, 1, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_perman_complex_minors_range(B.data(), n, 0, 1, nullptr, 1, nullptr, nullptr) == SUP_EINVAL);
  CHECK(sup_perman_complex_minors_range(B.data(), 1, 0, 1, nullptr, 1, out, nullptr) == SUP_EUNSUPPORTED);
  CHECK(sup_perman_complex_minors_range(B.data(), 33, 0, 1, nullptr, 1, out, nullptr) == SUP_EUNSUPPORTED);
  sup_opts o = opts(1);
  o.walk_log2 = 32;
  CHECK(sup_perman_complex_minors_range(B.data(), n, 0, 1, &o, 1, out, nullptr) == SUP_EINVAL);
}

static void test_arguments() {
  const std::vector<double> a = random_doubles(2 * 8 * 8, 5);
  double out[8] = {1, 1, 1, 1, 1, 1, 1, 1};
  int32_t rows[4] = {0, 1, 2, 0}, cols[2] = {0, 2};
  CHECK(sup_perman_complex_minors(nullptr, 3, 3, rows, cols, 2, 2, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_perman_complex_minors(a.data(), 3, 3, nullptr, cols, 2, 2, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_perman_complex_minors(a.data(), 3, 3, rows, nullptr, 2, 2, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_perman_complex_minors(a.data(), 3, 3, rows, cols, 2, 2, nullptr, 1, nullptr, nullptr) == SUP_EINVAL);
  CHECK(sup_perman_complex_minors(a.data(), 0, 3, rows, cols, 2, 2, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_perman_complex_minors(a.data(), 3, 0, rows, cols, 2, 2, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_perman_complex_minors(a.data(), 3, 3, rows, cols, 0, 2, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_perman_complex_minors(a.data(), 3, 3, rows, cols, 65, 0, nullptr, 1, out, nullptr) == SUP_EINVAL);
  sup_opts o = opts(1);
  o.walk_log2 = 32;
  CHECK(sup_perman_complex_minors(a.data(), 3, 3, rows, cols, 2, 2, &o, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_perman_complex_minors(a.data(), 3, 3, rows, cols, 2, 0, nullptr, 1, out, nullptr) == SUP_OK);
  CHECK(out[0] == 1 && out[1] == 1);  // nothing written
  CHECK(sup_perman_complex_minors(a.data(), 3, 3, rows, cols, 2, 2, nullptr, 1, out, nullptr) == SUP_OK);
  rows[3] = 3;  // k = 1, position 1, R = 3
  CHECK(sup_perman_complex_minors(a.data(), 3, 3, rows, cols, 2, 2, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(std::strstr(sup_last_error(), "rows[k = 1][position 1] = 3") != nullptr);
  rows[3] = 0, cols[1] = -1;  // k = 1, position 0
  CHECK(sup_perman_complex_minors(a.data(), 3, 3, rows, cols, 2, 2, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(std::strstr(sup_last_error(), "cols[k = 1][position 0] = -1") != nullptr);
}

// M x M unitary: Gram-Schmidt on a random complex matrix's columns
static std::vector<double> random_unitary(int M, unsigned seed) {
  std::vector<double> a = random_doubles((size_t)2 * M * M, seed);
  auto re = [&](int i, int j) -> double& { return a[2 * ((size_t)i * M + j)]; };
  auto im = [&](int i, int j) -> double& { return a[2 * ((size_t)i * M + j) + 1]; };
  for (int pass = 0; pass < 2; ++pass)  // twice: orthonormal to rounding
    for (int j = 0; j < M; ++j) {
      for (int b = 0; b < j; ++b) {
        double pr = 0, pi = 0;  // <col b, col j>
        for (int i = 0; i < M; ++i) {
          pr += re(i, b) * re(i, j) + im(i, b) * im(i, j);
          pi += re(i, b) * im(i, j) - im(i, b) * re(i, j);
        }
        for (int i = 0; i < M; ++i) {
          const double xr = re(i, b), xi = im(i, b);
          re(i, j) -= pr * xr - pi * xi;
          im(i, j) -= pr * xi + pi * xr;
        }
      }
      double nn = 0;
      for (int i = 0; i < M; ++i) nn += re(i, j) * re(i, j) + im(i, j) * im(i, j);
      nn = std::sqrt(nn);
      for (int i = 0; i < M; ++i) re(i, j) /= nn, im(i, j) /= nn;
    }
  return a;
}

static void test_sampler() {
  const int M = 7, n = 4;
  const std::vector<double> U = random_unitary(M, 31);
  const int32_t inputs[n] = {5, 0, 2, 6};
  std::vector<int32_t> s1(50 * n + 1, -7), s8(50 * n, -7), longer(120 * n, -7);
  const sup_opts o1 = opts(1), o8 = opts(8);
  sup_stats st;
  CHECK(sup_boson_sample(U.data(), M, inputs, n, 50, 11, &o1, 1, s1.data(), &st) == SUP_OK);
  CHECK(s1[50 * n] == -7);  // guard
  CHECK(st.leaves == 50 && st.devices_used == 0 && st.gray_steps == 50ull * (1 + 2 + 4));
  CHECK(sup_boson_sample(U.data(), M, inputs, n, 50, 11, &o8, 1, s8.data(), nullptr) == SUP_OK);
  CHECK(sup_boson_sample(U.data(), M, inputs, n, 120, 11, &o8, 1, longer.data(), nullptr) == SUP_OK);
  for (int i = 0; i < 50 * n; ++i) CHECK(s1[i] == s8[i] && s1[i] == longer[i]);
  for (int s = 0; s < 50; ++s)
    for (int j = 0; j < n; ++j) {
      CHECK(s1[s * n + j] >= 0 && s1[s * n + j] < M);
      if (j) CHECK(s1[s * n + j - 1] <= s1[s * n + j]);
    }
  int32_t out[8] = {-7, -7, -7, -7, -7, -7, -7, -7};
  CHECK(sup_boson_sample(U.data(), M, inputs, 1, 2, 0, nullptr, 1, out, nullptr) == SUP_OK);  // n = 1
  CHECK(out[0] >= 0 && out[0] < M && out[1] >= 0 && out[1] < M && out[2] == -7);
  CHECK(sup_boson_sample(U.data(), M, inputs, n, 0, 0, nullptr, 1, out, nullptr) == SUP_OK);
  CHECK(out[2] == -7);
  CHECK(sup_boson_sample(nullptr, M, inputs, n, 1, 0, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_boson_sample(U.data(), M, nullptr, n, 1, 0, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_boson_sample(U.data(), M, inputs, n, 1, 0, nullptr, 1, nullptr, nullptr) == SUP_EINVAL);
  CHECK(sup_boson_sample(U.data(), M, inputs, 0, 1, 0, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_boson_sample(U.data(), 0, inputs, n, 1, 0, nullptr, 1, out, nullptr) == SUP_EINVAL);
  const int32_t rep[3] = {1, 4, 1}, oob[2] = {0, 7}, neg[2] = {-1, 3};
  CHECK(sup_boson_sample(U.data(), M, rep, 3, 1, 0, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(std::strstr(sup_last_error(), "inputs[position 2] = 1 repeats position 0") != nullptr);
  CHECK(sup_boson_sample(U.data(), M, oob, 2, 1, 0, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(std::strstr(sup_last_error(), "inputs[position 1] = 7 outside [0, 7)") != nullptr);
  CHECK(sup_boson_sample(U.data(), M, neg, 2, 1, 0, nullptr, 1, out, nullptr) == SUP_EINVAL);
  std::vector<double> bad = U;
  bad[2 * (3 * M + 5)] += 1e-6;  // column 5 is used
  CHECK(sup_boson_sample(bad.data(), M, inputs, n, 1, 0, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(std::strstr(sup_last_error(), "not orthonormal") != nullptr);
  std::vector<int32_t> many(33);
  for (int j = 0; j < 33; ++j) many[j] = j;
  CHECK(sup_boson_sample(U.data(), 40, many.data(), 33, 1, 0, nullptr, 1, out, nullptr) == SUP_EUNSUPPORTED);
  sup_opts o = opts(1);
  o.walk_log2 = -1;
  CHECK(sup_boson_sample(U.data(), M, inputs, n, 1, 0, &o, 1, out, nullptr) == SUP_EINVAL);
}

int main() {
  test_values_and_bits();
  test_range();
  test_arguments();
  test_sampler();
  std::printf("selftest_complex_minors: %s (%d failed checks)\n", failures ? "FAILED" : "ok", failures);
  return failures ? 1 : 0;
}
