// selftest_complex_fock_minors.cpp — host-code self test of the collision-aware
// one-walk minors and the sampler on them for the sanitizer builds (make -C
// superman_amd/csrc sanitize-complex-fock-minors: AddressSanitizer +
// UndefinedBehaviorSanitizer, and ThreadSanitizer).  No GPU is needed.  It
// drives, with on_cpu = 1 on 1 and 8 host threads,
//   - sup_perman_complex_fock_minors at n = 1, 2, 7, 12 with count 0, 1 and 5
//     and column lists that repeat: every result agrees with
//     sup_perman_complex_minors on the same lists within 1e-10 of the sum of
//     the moduli, has the bits of the call on that matrix alone, and the thread
//     count and the slab size change no bit; visited_steps is the plan entry's sum;
//   - a layout with walk digits and more than one wave-chunk (n = 12, all
//     columns distinct: T = 2^10, Tw = 16, H = 64; n = 12, (1 x 9, 2): T = 768);
//   - sup_perman_complex_fock_minors_plan on hand-counted patterns;
//   - sup_boson_sample_fock: 50 samples, sorted rows in range, the same on 1 and
//     8 threads, as a prefix of a longer run, and equal to sup_boson_sample's;
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

// rows (count x n) and cols (count x (n-1)); matrix k draws its columns from
// 1 + k % 4 ... C values, so the collision patterns differ; rows repeat too
static void make_lists(int n, uint64_t count, int R, int C, unsigned seed, std::vector<int32_t>& rows,
                       std::vector<int32_t>& cols) {
  std::mt19937 g(seed);
  const int q = n - 1;
  rows.assign((size_t)(count ? count : 1) * n, 0);
  cols.assign((size_t)(count ? count : 1) * (q ? q : 1), 0);
  for (uint64_t k = 0; k < count; ++k) {
    const unsigned range = k % 4 == 3 ? (unsigned)C : 1u + (unsigned)(k % 4) * 2u;
    for (int j = 0; j < n; ++j) rows[k * n + j] = (int32_t)(g() % (unsigned)R);
    for (int c = 0; c < q; ++c) cols[k * q + c] = (int32_t)(g() % range);
    if (n > 2) rows[k * n + n - 1] = rows[k * n];
  }
}

static void test_values_and_bits() {
  const int R = 13, C = 14;
  const std::vector<double> U = random_doubles((size_t)2 * R * C, 9);
  for (int n : {1, 2, 7, 12})
    for (uint64_t count : {(uint64_t)0, (uint64_t)1, (uint64_t)5}) {
      const int q = n - 1;
      std::vector<int32_t> rows, cols;
      make_lists(n, count, R, C, 170u + (unsigned)n, rows, cols);
      const sup_opts o1 = opts(1);
      std::vector<double> ref(2 * (size_t)count * n + 2, 0.0), alone(2 * (size_t)count * n, 0.0);
      std::vector<uint64_t> terms(count + 1, 0);
      CHECK(sup_perman_complex_fock_minors_plan(cols.data(), n, count, terms.data()) == SUP_OK);
      uint64_t total = 0;
      for (uint64_t k = 0; k < count; ++k) total += n >= 2 ? terms[k] : 0;
      CHECK(sup_perman_complex_minors(U.data(), R, C, rows.data(), cols.data(), n, count, &o1, 1, ref.data(), nullptr) ==
            SUP_OK);
      for (uint64_t k = 0; k < count; ++k)
        CHECK(sup_perman_complex_fock_minors(U.data(), R, C, rows.data() + k * n, cols.data() + k * q, n, 1, &o1, 1,
                                             &alone[2 * k * n], nullptr) == SUP_OK);
      for (int threads : {1, 8})
        for (const char* slab : {"", "2"}) {
          setenv("SUP_CPLX_FOCK_MINORS_SLAB", slab, 1);
          const sup_opts o = opts(threads);
          std::vector<double> out(2 * (size_t)count * n + 2, 42.0);  // two guard values behind the results
          sup_stats st;
          CHECK(sup_perman_complex_fock_minors(U.data(), R, C, rows.data(), cols.data(), n, count, &o, 1, out.data(),
                                               &st) == SUP_OK);
          CHECK(out[2 * count * n] == 42.0 && out[2 * count * n + 1] == 42.0);
          out.resize(2 * (size_t)count * n);
          CHECK(same_bits(out, alone));
          for (uint64_t i = 0; i < count * n; ++i) {
            if (q == 0) {
              CHECK(out[2 * i] == 1.0 && out[2 * i + 1] == 0.0);
              continue;
            }
            const double mod = std::hypot(ref[2 * i], ref[2 * i + 1]) + std::hypot(out[2 * i], out[2 * i + 1]);
            CHECK(std::hypot(out[2 * i] - ref[2 * i], out[2 * i + 1] - ref[2 * i + 1]) <= 1e-10 * mod);
          }
          CHECK(st.devices_used == 0 && st.leaves == (int)(count * n));
          CHECK(st.gray_steps == (n >= 2 ? count << (n - 2) : 0));
          CHECK(st.visited_steps == total);
          CHECK(st.est_ops_per_step == (n >= 2 ? 16.0 * n - 20.0 : 0.0));
        }
      unsetenv("SUP_CPLX_FOCK_MINORS_SLAB");
    }
  // n = 1 takes no column list
  double one[2] = {0, 0};
  const int32_t r0[1] = {3};
  CHECK(sup_perman_complex_fock_minors(U.data(), R, C, r0, nullptr, 1, 1, nullptr, 1, one, nullptr) == SUP_OK);
  CHECK(one[0] == 1.0 && one[1] == 0.0);
}

// walk digits and more than one wave-chunk, the chunk queue shared by 8 threads
static void test_walk_digits_and_chunks() {
  const int R = 12, C = 14, n = 12, q = 11;
  const std::vector<double> U = random_doubles((size_t)2 * R * C, 19);
  std::vector<int32_t> rows(3 * n), cols(3 * q);
  for (int k = 0; k < 3; ++k)
    for (int j = 0; j < n; ++j) rows[k * n + j] = (j + k) % R;
  for (int c = 0; c < q; ++c) cols[c] = c;                       // all distinct: T = 2^10, Tw = 16, H = 64
  for (int c = 0; c < q; ++c) cols[q + c] = c < 9 ? c : 9;       // (1 x 9, 2): the first single held, T = 2^8 x 3 = 768
  for (int c = 0; c < q; ++c) cols[2 * q + c] = c / 4;           // (4, 4, 3): the last held, T = 5 x 5 x 3 = 75
  uint64_t terms[3];
  CHECK(sup_perman_complex_fock_minors_plan(cols.data(), n, 3, terms) == SUP_OK);
  CHECK(terms[0] == 1024 && terms[1] == 768 && terms[2] == 75);
  std::vector<double> ref(2 * 3 * n), a(2 * 3 * n), b(2 * 3 * n);
  const sup_opts o1 = opts(1), o8 = opts(8);
  CHECK(sup_perman_complex_minors(U.data(), R, C, rows.data(), cols.data(), n, 3, &o1, 1, ref.data(), nullptr) == SUP_OK);
  CHECK(sup_perman_complex_fock_minors(U.data(), R, C, rows.data(), cols.data(), n, 3, &o1, 1, a.data(), nullptr) == SUP_OK);
  CHECK(sup_perman_complex_fock_minors(U.data(), R, C, rows.data(), cols.data(), n, 3, &o8, 1, b.data(), nullptr) == SUP_OK);
  CHECK(same_bits(a, b));
  for (int i = 0; i < 3 * n; ++i) {
    const double mod = std::hypot(ref[2 * i], ref[2 * i + 1]) + std::hypot(a[2 * i], a[2 * i + 1]);
    CHECK(std::hypot(a[2 * i] - ref[2 * i], a[2 * i + 1] - ref[2 * i + 1]) <= 1e-10 * mod);
  }
}

static void test_plan() {
  const int32_t c1[1] = {5}, c3[3] = {2, 2, 2}, c6[6] = {7, 7, 7, 3, 3, 9}, c7[7] = {0, 0, 1, 1, 1, 2, 2};
  uint64_t t = 0;
  CHECK(sup_perman_complex_fock_minors_plan(c1, 2, 1, &t) == SUP_OK && t == 1);
  CHECK(sup_perman_complex_fock_minors_plan(c3, 4, 1, &t) == SUP_OK && t == 3);
  CHECK(sup_perman_complex_fock_minors_plan(c6, 7, 1, &t) == SUP_OK && t == 12);  // (3, 2, 1): the single is held
  CHECK(sup_perman_complex_fock_minors_plan(c7, 8, 1, &t) == SUP_OK && t == 24);  // a tie (2, 2): the first is held
  CHECK(sup_perman_complex_fock_minors_plan(nullptr, 1, 1, &t) == SUP_OK && t == 1);
  CHECK(sup_perman_complex_fock_minors_plan(c3, 4, 0, &t) == SUP_OK);
  CHECK(sup_perman_complex_fock_minors_plan(nullptr, 4, 1, &t) == SUP_EINVAL);
  CHECK(sup_perman_complex_fock_minors_plan(c3, 4, 1, nullptr) == SUP_EINVAL);
  CHECK(sup_perman_complex_fock_minors_plan(c3, 0, 1, &t) == SUP_EINVAL);
  CHECK(sup_perman_complex_fock_minors_plan(c3, 33, 1, &t) == SUP_EUNSUPPORTED);
}

static void test_arguments() {
  const std::vector<double> a = random_doubles(2 * 8 * 8, 5);
  double out[8] = {1, 1, 1, 1, 1, 1, 1, 1};
  int32_t rows[4] = {0, 1, 2, 0}, cols[2] = {0, 2};
  CHECK(sup_perman_complex_fock_minors(nullptr, 3, 3, rows, cols, 2, 2, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_perman_complex_fock_minors(a.data(), 3, 3, nullptr, cols, 2, 2, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_perman_complex_fock_minors(a.data(), 3, 3, rows, nullptr, 2, 2, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_perman_complex_fock_minors(a.data(), 3, 3, rows, cols, 2, 2, nullptr, 1, nullptr, nullptr) == SUP_EINVAL);
  CHECK(sup_perman_complex_fock_minors(a.data(), 0, 3, rows, cols, 2, 2, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_perman_complex_fock_minors(a.data(), 3, 0, rows, cols, 2, 2, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_perman_complex_fock_minors(a.data(), 3, 3, rows, cols, 0, 2, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_perman_complex_fock_minors(a.data(), 3, 3, rows, cols, -3, 2, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_perman_complex_fock_minors(a.data(), 3, 3, rows, cols, 33, 0, nullptr, 1, out, nullptr) == SUP_EUNSUPPORTED);
  CHECK(sup_perman_complex_fock_minors(a.data(), 3, 3, rows, cols, 64, 0, nullptr, 1, out, nullptr) == SUP_EUNSUPPORTED);
  sup_opts o = opts(1);
  o.walk_log2 = 32;
  CHECK(sup_perman_complex_fock_minors(a.data(), 3, 3, rows, cols, 2, 2, &o, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_perman_complex_fock_minors(a.data(), 3, 3, rows, cols, 2, 0, nullptr, 1, out, nullptr) == SUP_OK);
  CHECK(out[0] == 1 && out[1] == 1);  // nothing written
  CHECK(sup_perman_complex_fock_minors(a.data(), 3, 3, rows, cols, 2, 2, nullptr, 1, out, nullptr) == SUP_OK);
  rows[3] = 3;  // k = 1, position 1, R = 3
  CHECK(sup_perman_complex_fock_minors(a.data(), 3, 3, rows, cols, 2, 2, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(std::strstr(sup_last_error(), "rows[k = 1][position 1] = 3") != nullptr);
  rows[3] = 0, cols[1] = -1;  // k = 1, position 0
  CHECK(sup_perman_complex_fock_minors(a.data(), 3, 3, rows, cols, 2, 2, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(std::strstr(sup_last_error(), "cols[k = 1][position 0] = -1") != nullptr);
  cols[1] = 3;  // C = 3
  CHECK(sup_perman_complex_fock_minors(a.data(), 3, 3, rows, cols, 2, 2, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(std::strstr(sup_last_error(), "cols[k = 1][position 0] = 3") != nullptr);
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
  std::vector<int32_t> s1(50 * n + 1, -7), s8(50 * n, -7), longer(120 * n, -7), parent(50 * n, -7);
  const sup_opts o1 = opts(1), o8 = opts(8);
  sup_stats st;
  CHECK(sup_boson_sample_fock(U.data(), M, inputs, n, 50, 11, &o1, 1, s1.data(), &st) == SUP_OK);
  CHECK(s1[50 * n] == -7);  // guard
  CHECK(st.leaves == 50 && st.devices_used == 0 && st.gray_steps == 50ull * (1 + 2 + 4));
  CHECK(st.visited_steps >= 50ull * 3 && st.visited_steps <= st.gray_steps && st.est_ops_per_step == 16.0 * n - 20.0);
  CHECK(sup_boson_sample_fock(U.data(), M, inputs, n, 50, 11, &o8, 1, s8.data(), nullptr) == SUP_OK);
  CHECK(sup_boson_sample_fock(U.data(), M, inputs, n, 120, 11, &o8, 1, longer.data(), nullptr) == SUP_OK);
  CHECK(sup_boson_sample(U.data(), M, inputs, n, 50, 11, &o8, 1, parent.data(), nullptr) == SUP_OK);
  for (int i = 0; i < 50 * n; ++i) CHECK(s1[i] == s8[i] && s1[i] == longer[i] && s1[i] == parent[i]);
  for (int s = 0; s < 50; ++s)
    for (int j = 0; j < n; ++j) {
      CHECK(s1[s * n + j] >= 0 && s1[s * n + j] < M);
      if (j) CHECK(s1[s * n + j - 1] <= s1[s * n + j]);
    }
  int32_t out[8] = {-7, -7, -7, -7, -7, -7, -7, -7};
  CHECK(sup_boson_sample_fock(U.data(), M, inputs, 1, 2, 0, nullptr, 1, out, nullptr) == SUP_OK);  // n = 1
  CHECK(out[0] >= 0 && out[0] < M && out[1] >= 0 && out[1] < M && out[2] == -7);
  CHECK(sup_boson_sample_fock(U.data(), M, inputs, n, 0, 0, nullptr, 1, out, nullptr) == SUP_OK);
  CHECK(out[2] == -7);
  CHECK(sup_boson_sample_fock(nullptr, M, inputs, n, 1, 0, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_boson_sample_fock(U.data(), M, nullptr, n, 1, 0, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_boson_sample_fock(U.data(), M, inputs, n, 1, 0, nullptr, 1, nullptr, nullptr) == SUP_EINVAL);
  CHECK(sup_boson_sample_fock(U.data(), M, inputs, 0, 1, 0, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_boson_sample_fock(U.data(), 0, inputs, n, 1, 0, nullptr, 1, out, nullptr) == SUP_EINVAL);
  const int32_t rep[3] = {1, 4, 1}, oob[2] = {0, 7}, neg[2] = {-1, 3};
  CHECK(sup_boson_sample_fock(U.data(), M, rep, 3, 1, 0, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(std::strstr(sup_last_error(), "inputs[position 2] = 1 repeats position 0") != nullptr);
  CHECK(sup_boson_sample_fock(U.data(), M, oob, 2, 1, 0, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(std::strstr(sup_last_error(), "inputs[position 1] = 7 outside [0, 7)") != nullptr);
  CHECK(sup_boson_sample_fock(U.data(), M, neg, 2, 1, 0, nullptr, 1, out, nullptr) == SUP_EINVAL);
  std::vector<double> bad = U;
  bad[2 * (3 * M + 5)] += 1e-6;  // column 5 is used
  CHECK(sup_boson_sample_fock(bad.data(), M, inputs, n, 1, 0, nullptr, 1, out, nullptr) == SUP_EINVAL);
  CHECK(std::strstr(sup_last_error(), "not orthonormal") != nullptr);
  std::vector<int32_t> many(33);
  for (int j = 0; j < 33; ++j) many[j] = j;
  CHECK(sup_boson_sample_fock(U.data(), 40, many.data(), 33, 1, 0, nullptr, 1, out, nullptr) == SUP_EUNSUPPORTED);
  sup_opts o = opts(1);
  o.walk_log2 = -1;
  CHECK(sup_boson_sample_fock(U.data(), M, inputs, n, 1, 0, &o, 1, out, nullptr) == SUP_EINVAL);
}

int main() {
  test_values_and_bits();
  test_walk_digits_and_chunks();
  test_plan();
  test_arguments();
  test_sampler();
  std::printf("selftest_complex_fock_minors: %s (%d failed checks)\n", failures ? "FAILED" : "ok", failures);
  return failures ? 1 : 0;
}
