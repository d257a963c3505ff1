// selftest_torontonian_table.cpp — host-code self test of the torontonian table
// entry points for the sanitizer builds (make -C superman_amd/csrc
// sanitize-torontonian-table: AddressSanitizer + UndefinedBehaviorSanitizer,
// and ThreadSanitizer).  No GPU is needed.  It drives, with on_cpu = 1 on 1 and
// 8 host threads,
//   - sup_torontonian_table and sup_loop_torontonian_table at n = 1, 3, 6, 10,
//     13 (one run of subsets, several runs shared among the threads, stages of
//     the transform split over the threads): raw and transformed tables have
//     the same bits on 1 and 8 threads; raw[z] has the bits of the one-subset
//     range entry up to its sign; the transformed table has the bits of a
//     naive stage loop over raw and agrees with the per-pattern entry to
//     rounding; gamma = 0 gives the torontonian table's bits; 3^popcount with
//     equality;
//   - sup_mobius_subsets on integers at n = 0, 1, 7, 14 against an integer
//     transform, with SUP_MOBIUS_BITS forcing other shapes and refusing bad ones;
//   - the stats, the argument, mode, device-count and cap checks, and NaN on
//     exactly the supersets of a subset that is not positive definite.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
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

static std::vector<double> make_gamma(int M, unsigned seed) {
  std::mt19937_64 g(seed);
  std::uniform_real_distribution<double> d(-0.5, 0.5);
  std::vector<double> v((size_t)4 * M);
  for (double& x : v) x = d(g);
  return v;
}

static std::vector<int32_t> make_list(int n, int M, unsigned seed) {
  std::mt19937 g(seed);
  std::vector<int32_t> base(M);
  for (int i = 0; i < M; ++i) base[i] = i;
  for (int i = M - 1; i > 0; --i) std::swap(base[i], base[g() % (unsigned)(i + 1)]);
  base.resize(n);
  return base;
}

static void naive_mobius(std::vector<double>& t, int n, double sign) {
  for (int b = 0; b < n; ++b)
    for (size_t z = 0; z < t.size(); ++z)
      if ((z >> b) & 1u) t[z] = t[z] + sign * t[z ^ ((size_t)1 << b)];
}

static int table(bool loop, const std::vector<double>& O, int M, const std::vector<double>& gamma, const int32_t* modes,
                 int n, int transform, const sup_opts* o, double* out, sup_stats* st) {
  return loop ? sup_loop_torontonian_table(O.data(), M, gamma.data(), modes, n, transform, o, 1, out, st)
              : sup_torontonian_table(O.data(), M, modes, n, transform, o, 1, out, st);
}

static void test_tables() {
  const int M = 14;
  const std::vector<double> O = make_matrix(M, 51), gamma = make_gamma(M, 52), zero((size_t)4 * M, 0.0);
  sup_opts o1 = opts(1), o8 = opts(8);
  for (int n : {1, 3, 6, 10, 13})
    for (bool loop : {false, true}) {
      const std::vector<int32_t> modes = make_list(n, M, 200 + n);
      const size_t T = (size_t)1 << n;
      std::vector<double> raw1(T), raw8(T), tab1(T), tab8(T);
      sup_stats st;
      CHECK(table(loop, O, M, gamma, modes.data(), n, 0, &o1, raw1.data(), nullptr) == SUP_OK);
      CHECK(table(loop, O, M, gamma, modes.data(), n, 0, &o8, raw8.data(), &st) == SUP_OK);
      CHECK(table(loop, O, M, gamma, modes.data(), n, 1, &o1, tab1.data(), nullptr) == SUP_OK);
      CHECK(table(loop, O, M, gamma, modes.data(), n, 1, &o8, tab8.data(), nullptr) == SUP_OK);
      CHECK(same_bits(raw1, raw8) && same_bits(tab1, tab8) && raw1[0] == 1.0 && tab1[0] == 1.0);
      CHECK(st.leaves == 1 && st.gray_steps == T && st.visited_steps == T && st.kernel_ms == 0.0);
      double ops = 0.0;
      CHECK((loop ? sup_loop_torontonian_plan(n, nullptr, &ops) : sup_torontonian_plan(n, nullptr, &ops)) == SUP_OK);
      CHECK(st.est_ops_per_step == ops + 0.5 * n);
      std::vector<double> want = raw1, zeta = raw1, again = raw1;
      naive_mobius(want, n, -1.0);
      naive_mobius(zeta, n, +1.0);
      CHECK(same_bits(want, tab1));
      CHECK(sup_mobius_subsets(again.data(), n, &o8, 1) == SUP_OK && same_bits(again, tab1));
      if (n <= 10)
        for (size_t z = 0; z < T; ++z) {
          double r = 0.0;
          CHECK((loop ? sup_loop_torontonian_range(O.data(), M, gamma.data(), modes.data(), n, z, z + 1, &o1, 1, &r, nullptr)
                      : sup_torontonian_range(O.data(), M, modes.data(), n, z, z + 1, &o1, 1, &r, nullptr)) == SUP_OK);
          if ((n - __builtin_popcountll(z)) & 1) r = -r;
          CHECK(std::memcmp(&r, &raw1[z], sizeof(double)) == 0);
        }
      for (size_t mask = 1; mask < T; mask += (n <= 6 ? 1 : 37)) {
        std::vector<int32_t> sub;
        for (int b = 0; b < n; ++b)
          if ((mask >> b) & 1u) sub.push_back(modes[b]);
        double v = 0.0;
        CHECK((loop ? sup_loop_torontonian(O.data(), M, gamma.data(), sub.data(), (int)sub.size(), 1, &o8, 1, &v, nullptr)
                    : sup_torontonian(O.data(), M, sub.data(), (int)sub.size(), 1, &o8, 1, &v, nullptr)) == SUP_OK);
        CHECK(std::fabs(v - tab1[mask]) <= 2.0 * (sub.size() + 21.0) * 1.1102230246251565e-16 * zeta[mask]);
      }
      if (loop) {  // gamma = 0: the torontonian table's bits
        std::vector<double> a(T), b(T);
        CHECK(table(true, O, M, zero, modes.data(), n, 1, &o8, a.data(), nullptr) == SUP_OK);
        CHECK(table(false, O, M, zero, modes.data(), n, 1, &o8, b.data(), nullptr) == SUP_OK);
        CHECK(same_bits(a, b));
      }
    }
  const int n = 11;  // O = (3/4) I: every pivot a power of two
  std::vector<double> D((size_t)8 * n * n, 0.0);
  for (int i = 0; i < 2 * n; ++i) D[2 * ((size_t)i * 2 * n + i)] = 0.75;
  std::vector<int32_t> modes(n);
  for (int i = 0; i < n; ++i) modes[i] = i;
  std::vector<double> tab((size_t)1 << n);
  CHECK(sup_torontonian_table(D.data(), n, modes.data(), n, 1, &o8, 1, tab.data(), nullptr) == SUP_OK);
  for (size_t mask = 0; mask < tab.size(); ++mask) CHECK(tab[mask] == std::pow(3.0, __builtin_popcountll(mask)));
}

static void test_mobius() {
  std::mt19937_64 g(61);
  for (int n : {0, 1, 7, 14})
    for (const char* bits : {"", "6,2", "9,5", "12,6"}) {
      const size_t T = (size_t)1 << n;
      std::vector<double> t(T);
      std::vector<long long> want(T);
      for (size_t z = 0; z < T; ++z) want[z] = (long long)(g() % 2097151) - 1048575, t[z] = (double)want[z];
      for (int b = 0; b < n; ++b)
        for (size_t z = 0; z < T; ++z)
          if ((z >> b) & 1u) want[z] -= want[z ^ ((size_t)1 << b)];
      if (*bits) setenv("SUP_MOBIUS_BITS", bits, 1);
      for (int threads : {1, 8}) {
        std::vector<double> v = t;
        sup_opts o = opts(threads);
        CHECK(sup_mobius_subsets(v.data(), n, &o, 1) == SUP_OK);
        for (size_t z = 0; z < T; ++z) CHECK(v[z] == (double)want[z]);
      }
      unsetenv("SUP_MOBIUS_BITS");
    }
  double t[4] = {1.0, 1.0, 1.0, 1.0};
  for (const char* bad : {"5,3", "13,3", "8,0", "8,7", "8", "8,3,1", "x"}) {
    setenv("SUP_MOBIUS_BITS", bad, 1);
    CHECK(sup_mobius_subsets(t, 2, nullptr, 1) == SUP_EINVAL && std::strstr(sup_last_error(), "SUP_MOBIUS_BITS") != nullptr);
    unsetenv("SUP_MOBIUS_BITS");
  }
  CHECK(t[3] == 1.0);  // a refused call writes nothing
  CHECK(sup_mobius_subsets(nullptr, 2, nullptr, 1) == SUP_EINVAL);
  CHECK(sup_mobius_subsets(t, -1, nullptr, 1) == SUP_EINVAL && sup_mobius_subsets(t, 29, nullptr, 1) == SUP_EINVAL);
  CHECK(sup_mobius_subsets(t, 2, nullptr, 1) == SUP_OK && t[0] == 1.0 && t[1] == 0.0 && t[2] == 0.0 && t[3] == 0.0);
}

static void test_arguments() {
  const int M = 4;
  std::vector<double> O = make_matrix(M, 45), gamma = make_gamma(M, 46);
  int32_t modes[3] = {0, 1, 2};
  double out[8] = {0.0};
  sup_opts o = opts(2);
  CHECK(sup_torontonian_table(nullptr, M, modes, 3, 1, &o, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_torontonian_table(O.data(), M, nullptr, 3, 1, &o, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_torontonian_table(O.data(), M, modes, 3, 1, &o, 1, nullptr, nullptr) == SUP_EINVAL);
  CHECK(sup_loop_torontonian_table(O.data(), M, nullptr, modes, 3, 1, &o, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_torontonian_table(O.data(), M, modes, 0, 1, &o, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_torontonian_table(O.data(), M, modes, 33, 1, &o, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_torontonian_table(O.data(), 0, modes, 3, 1, &o, 1, out, nullptr) == SUP_EINVAL);
  int32_t bad[3] = {0, 4, 2}, neg[3] = {0, -1, 2}, twice[3] = {2, 1, 2};
  CHECK(sup_torontonian_table(O.data(), M, bad, 3, 1, &o, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_torontonian_table(O.data(), M, neg, 3, 1, &o, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_loop_torontonian_table(O.data(), M, gamma.data(), twice, 3, 1, &o, 1, out, nullptr) == SUP_EINVAL);
  CHECK(std::strstr(sup_last_error(), "distinct") != nullptr);
  CHECK(sup_torontonian_table(O.data(), M, twice, 3, 1, &o, 0, out, nullptr) == SUP_EINVAL);  // before any device work
  sup_opts two = opts(2);
  two.gpu_num = 2;
  CHECK(sup_torontonian_table(O.data(), M, modes, 3, 1, &two, 1, out, nullptr) == SUP_EINVAL);
  CHECK(std::strstr(sup_last_error(), "gpu_num") != nullptr);
  CHECK(sup_torontonian_table(O.data(), M, modes, 3, 1, nullptr, 1, out, nullptr) == SUP_OK);  // default options
  static_assert(SUP_TORONTONIAN_TABLE_MAX_N == 28, "2 GiB of results");
  {  // above the cap on either path: refused before anything is written
    const int big = 29;
    std::vector<double> Z((size_t)8 * big * big, 0.0);
    std::vector<int32_t> all(big);
    for (int i = 0; i < big; ++i) all[i] = i;
    for (int on_cpu : {0, 1}) {
      CHECK(sup_torontonian_table(Z.data(), big, all.data(), big, 1, &o, on_cpu, out, nullptr) == SUP_EUNSUPPORTED);
      CHECK(sup_loop_torontonian_table(Z.data(), big, Z.data(), all.data(), big, 1, &o, on_cpu, out, nullptr) == SUP_EUNSUPPORTED);
    }
  }
  // not positive definite: NaN on exactly the masks that hold the position
  O[2 * ((size_t)1 * 2 * M + 1)] = 1.5;
  for (int transform : {0, 1}) {
    CHECK(sup_torontonian_table(O.data(), M, modes, 3, transform, &o, 1, out, nullptr) == SUP_OK);
    for (int z = 0; z < 8; ++z) CHECK(std::isnan(out[z]) == (((z >> 1) & 1) != 0));
  }
}

int main() {
  test_tables();
  test_mobius();
  test_arguments();
  std::printf("selftest_torontonian_table: %s (%d failed checks)\n", failures ? "FAILED" : "ok", failures);
  return failures ? 1 : 0;
}
