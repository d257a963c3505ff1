// selftest_lhaf_table.cpp — host-code self test of the loop-hafnian table entry
// points for the sanitizer builds (make -C superman_amd/csrc
// sanitize-lhaf-table: AddressSanitizer + UndefinedBehaviorSanitizer, and
// ThreadSanitizer).  No GPU is needed.  It drives, with on_cpu = 1 on 1 and 8
// host threads,
//   - sup_loop_hafnian_table at dims (1), (3), (1,1,1), (5,1,4), (1,6), (4,4,3),
//     (17,17,17,3) and (8,8,8,8,8,8) (slabs below and above the size at which
//     they are split over the threads), with mu and with mu = NULL: the same
//     bits on 1 and 8 threads and under every SUP_LHAF_TABLE_LOW; entry 0 is
//     1 + 0i; every entry agrees with sup_loop_hafnian_complex_each on the
//     gathered list to rounding; odd photon totals of the hafnian table are 0;
//     an output buffer at an address that is 8 modulo 16;
//   - sup_loop_hafnian_table_plan's counts against a direct count, and the stats;
//   - every argument, symmetry, option, knob, cap and device-count check, and a
//     NaN in mu on exactly the entries whose recurrence reads it.
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

// A complex symmetric M x M matrix (interleaved) and M loop weights, parts in (-scale, scale).
static std::vector<double> make_matrix(int M, double scale, unsigned seed) {
  std::mt19937_64 g(seed);
  std::uniform_real_distribution<double> d(-scale, scale);
  std::vector<double> A((size_t)2 * M * M);
  for (int i = 0; i < M; ++i)
    for (int j = 0; j <= i; ++j) {
      const double re = d(g), im = d(g);
      A[2 * ((size_t)i * M + j)] = A[2 * ((size_t)j * M + i)] = re;
      A[2 * ((size_t)i * M + j) + 1] = A[2 * ((size_t)j * M + i) + 1] = im;
    }
  return A;
}

static std::vector<double> make_mu(int M, double scale, unsigned seed) {
  std::mt19937_64 g(seed);
  std::uniform_real_distribution<double> d(-scale, scale);
  std::vector<double> v((size_t)2 * M);
  for (double& x : v) x = d(g);
  return v;
}

static size_t entries(const std::vector<int32_t>& dims) {
  size_t e = 1;
  for (int32_t d : dims) e *= (size_t)d;
  return e;
}

static void test_tables() {
  const std::vector<std::vector<int32_t>> shapes = {{1}, {3}, {1, 1, 1}, {5, 1, 4}, {1, 6}, {4, 4, 3}, {17, 17, 17, 3},
                                                    {8, 8, 8, 8, 8, 8}};
  sup_opts o1 = opts(1), o8 = opts(8);
  for (const auto& dims : shapes) {
    const int M = (int)dims.size();
    const size_t E = entries(dims);
    const std::vector<double> A = make_matrix(M, 0.4, 70 + M), mu = make_mu(M, 0.4, 80 + M), zero((size_t)2 * M, 0.0);
    for (const double* m : {mu.data(), (const double*)nullptr}) {
      std::vector<double> t1(2 * E), t8(2 * E), tk(2 * E), off(2 * E + 1);
      sup_stats st;
      CHECK(sup_loop_hafnian_table(A.data(), M, m, dims.data(), &o1, 1, t1.data(), nullptr) == SUP_OK);
      CHECK(sup_loop_hafnian_table(A.data(), M, m, dims.data(), &o8, 1, t8.data(), &st) == SUP_OK);
      CHECK(same_bits(t1, t8) && t1[0] == 1.0 && t1[1] == 0.0 && !std::signbit(t1[1]));
      CHECK(st.leaves == 1 && st.gray_steps == E && st.visited_steps == E && st.kernel_ms == 0.0 && st.devices_used == 0);
      uint64_t pe = 0, pl = 0;
      double ops = -1.0;
      CHECK(sup_loop_hafnian_table_plan(dims.data(), M, &pe, &pl, &ops) == SUP_OK && pe == E && pl >= 1);
      CHECK(st.est_ops_per_step == ops);
      for (const char* low : {"1", "2", "7", "300"}) {
        setenv("SUP_LHAF_TABLE_LOW", low, 1);
        CHECK(sup_loop_hafnian_table(A.data(), M, m, dims.data(), &o8, 1, tk.data(), nullptr) == SUP_OK && same_bits(tk, t1));
        unsetenv("SUP_LHAF_TABLE_LOW");
      }
      // a buffer of doubles need not be 16-byte aligned
      double* shifted = ((uintptr_t)off.data() & 15u) ? off.data() : off.data() + 1;
      CHECK(sup_loop_hafnian_table(A.data(), M, m, dims.data(), &o8, 1, shifted, nullptr) == SUP_OK);
      CHECK(std::memcmp(shifted, t1.data(), 2 * E * sizeof(double)) == 0);
      // the definition on the gathered list, and a direct count of the operations
      std::vector<int32_t> n(M, 0), list;
      double count_ops = 0.0;
      for (size_t x = 0; x < E; ++x) {
        int p = -1, total = 0, terms = 0;
        double fact = 1.0;
        for (int i = 0; i < M; ++i) {
          if (n[i]) p = i;
          total += n[i];
          for (int k = 2; k <= n[i]; ++k) fact *= k;
        }
        if (p >= 0) {
          for (int j = 0; j < p; ++j) terms += n[j] > 0;
          terms += n[p] > 1;
          count_ops += 6.0 + 6.0 * terms;
        }
        if (!m && (total & 1)) CHECK(t1[2 * x] == 0.0 && t1[2 * x + 1] == 0.0);
        if (total >= 1 && total <= 12 && (E <= 4096 || x % 97 == 0)) {
          list.clear();
          for (int i = 0; i < M; ++i) list.insert(list.end(), (size_t)n[i], i);
          const int32_t len = total;
          double v[2] = {0.0, 0.0};
          CHECK(sup_loop_hafnian_complex_each(A.data(), M, m ? m : zero.data(), 1, nullptr, list.data(),
                                              total, &len, 1, &o1, 1, v, nullptr) == SUP_OK);
          const double s = std::sqrt(fact), tol = 1e-12 * (std::hypot(v[0], v[1]) + 1.0);
          CHECK(std::fabs(t1[2 * x] * s - v[0]) <= tol && std::fabs(t1[2 * x + 1] * s - v[1]) <= tol);
        }
        for (int i = 0; i < M; ++i) {  // the next n, mode 0 fastest
          if (++n[i] < dims[i]) break;
          n[i] = 0;
        }
      }
      CHECK(std::fabs(ops * (double)E - count_ops) <= 1e-9 * count_ops + 1e-12);
    }
  }
}

static void test_arguments() {
  const int M = 3;
  std::vector<double> A = make_matrix(M, 0.5, 91), mu = make_mu(M, 0.5, 92);
  int32_t dims[3] = {3, 4, 3};
  double out[72];
  for (double& x : out) x = 7.0;
  sup_opts o = opts(2);
  CHECK(sup_loop_hafnian_table(nullptr, M, mu.data(), dims, &o, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_loop_hafnian_table(A.data(), M, mu.data(), nullptr, &o, 1, out, nullptr) == SUP_EINVAL);
  CHECK(sup_loop_hafnian_table(A.data(), M, mu.data(), dims, &o, 1, nullptr, nullptr) == SUP_EINVAL);
  CHECK(std::strstr(sup_last_error(), "null pointer") != nullptr);
  for (int bad : {0, -1, 65}) {
    CHECK(sup_loop_hafnian_table(A.data(), bad, mu.data(), dims, &o, 1, out, nullptr) == SUP_EINVAL);
    CHECK(std::strstr(sup_last_error(), "outside [1, 64]") != nullptr);
  }
  for (int32_t bad : {0, -2, 66}) {
    int32_t d[3] = {3, bad, 3};
    CHECK(sup_loop_hafnian_table(A.data(), M, mu.data(), d, &o, 1, out, nullptr) == SUP_EINVAL);
    CHECK(std::strstr(sup_last_error(), "dims[1]") != nullptr);
    CHECK(sup_loop_hafnian_table_plan(d, M, nullptr, nullptr, nullptr) == SUP_EINVAL);
  }
  {
    std::vector<double> skew = A;
    skew[2 * (2 * M + 0) + 1] = std::nextafter(skew[2 * (2 * M + 0) + 1], 9.0);
    for (int on_cpu : {0, 1}) {  // before any device work
      CHECK(sup_loop_hafnian_table(skew.data(), M, mu.data(), dims, &o, on_cpu, out, nullptr) == SUP_EINVAL);
      CHECK(std::strstr(sup_last_error(), "A[0][2] and A[2][0] differ") != nullptr);
    }
  }
  sup_opts two = opts(2);
  two.gpu_num = 2;
  CHECK(sup_loop_hafnian_table(A.data(), M, mu.data(), dims, &two, 1, out, nullptr) == SUP_EINVAL);
  CHECK(std::strstr(sup_last_error(), "gpu_num = 2") != nullptr);
  for (const char* bad : {"0", "4097", "-3", "12x", "x", " "}) {
    setenv("SUP_LHAF_TABLE_LOW", bad, 1);
    CHECK(sup_loop_hafnian_table(A.data(), M, mu.data(), dims, &o, 1, out, nullptr) == SUP_EINVAL);
    CHECK(std::strstr(sup_last_error(), "SUP_LHAF_TABLE_LOW") != nullptr);
    CHECK(sup_loop_hafnian_table_plan(dims, M, nullptr, nullptr, nullptr) == SUP_EINVAL);
    unsetenv("SUP_LHAF_TABLE_LOW");
  }
  static_assert(SUP_LHAF_TABLE_MAX_ENTRIES == (1ull << 27), "2 GiB of results");
  {  // above the cap on either path: refused before anything is written
    const int big = 5;
    const std::vector<double> Z((size_t)2 * big * big, 0.0);
    const int32_t over[5] = {65, 65, 65, 65, 8};
    for (int on_cpu : {0, 1}) {
      CHECK(sup_loop_hafnian_table(Z.data(), big, nullptr, over, &o, on_cpu, out, nullptr) == SUP_EUNSUPPORTED);
      CHECK(std::strstr(sup_last_error(), "142805000 above SUP_LHAF_TABLE_MAX_ENTRIES") != nullptr);
    }
    const std::vector<double> Z64((size_t)2 * 64 * 64, 0.0);
    std::vector<int32_t> all(64, 65);
    CHECK(sup_loop_hafnian_table(Z64.data(), 64, nullptr, all.data(), &o, 1, out, nullptr) == SUP_EUNSUPPORTED);
    uint64_t e = 0, l = 0;
    double ops = 1.0;
    CHECK(sup_loop_hafnian_table_plan(all.data(), 64, &e, &l, &ops) == SUP_OK && e == ~0ull && ops == 0.0);
    CHECK(l == 1 + 63 * 64);  // the low kernel takes mode 0 alone: 65^2 = 4225 > 4096
  }
  for (double x : out) CHECK(x == 7.0);  // a refused call writes nothing
  int ndev = -1;
  if (sup_device_count(&ndev) != SUP_OK || ndev == 0)
    CHECK(sup_loop_hafnian_table(A.data(), M, mu.data(), dims, &o, 0, out, nullptr) == SUP_ENODEV);
  CHECK(sup_loop_hafnian_table(A.data(), M, mu.data(), dims, nullptr, 1, out, nullptr) == SUP_OK);  // default options
  CHECK(out[0] == 1.0 && out[1] == 0.0);
  // a NaN in mu_1: exactly the entries with n_1 > 0
  mu[2] = std::nan("");
  CHECK(sup_loop_hafnian_table(A.data(), M, mu.data(), dims, &o, 1, out, nullptr) == SUP_OK);
  for (int x = 0; x < 36; ++x) {
    const bool hit = ((x / 3) % 4) != 0;
    CHECK(std::isnan(out[2 * x]) == hit && std::isnan(out[2 * x + 1]) == hit);
  }
}

int main() {
  test_tables();
  test_arguments();
  std::printf("selftest_lhaf_table: %s (%d failed checks)\n", failures ? "FAILED" : "ok", failures);
  return failures ? 1 : 0;
}
