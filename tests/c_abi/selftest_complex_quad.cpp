// selftest_complex_quad.cpp — host-code self test of the complex
// double-double entry points for the sanitizer builds (make -C
// superman_amd/csrc sanitize-complex-quad: AddressSanitizer +
// UndefinedBehaviorSanitizer, and ThreadSanitizer).  No GPU is needed.  It
// drives
//   - sup_perman_complex_quad and sup_perman_complex_quad_range with
//     on_cpu = 1 at n = 1, 2, 7, 12 on 1 and 8 host threads: the thread count
//     changes no bit, every part is a normalised pair, and aligned ranges
//     folded pairwise in double-double reproduce the whole sum;
//   - every argument check, the empty range, and on_cpu = 0: n above
//     SUP_CPLX_QUAD_MAX_DEVICE_N is SUP_EUNSUPPORTED before any device is
//     looked for, and below it a machine without a device answers SUP_ENODEV.
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

static std::vector<double> random_complex(int n, unsigned seed) {
  std::mt19937_64 g(seed);
  std::normal_distribution<double> d(0.0, 1.0);
  std::vector<double> a((size_t)2 * n * n);
  for (auto& v : a) v = d(g);
  return a;
}

// (hi, lo) + (hi, lo) as the entries' chunk tree adds them (dd.hpp dd_add; IEEE adds only)
static void two_sum(double a, double b, double* s, double* e) {
  *s = a + b;
  const double bb = *s - a;
  *e = (a - (*s - bb)) + (b - bb);
}
static void dd_add(const double* a, const double* b, double* out) {
  double s, se, t, te;
  two_sum(a[0], b[0], &s, &se);
  two_sum(a[1], b[1], &t, &te);
  se += t;
  double h = s + se;
  se = se - (h - s);
  s = h;
  se += te;
  h = s + se;
  out[1] = se - (h - s);
  out[0] = h;
}

static void test_perman() {
  for (int n : {1, 2, 7, 12}) {
    const std::vector<double> a = random_complex(n, 200u + (unsigned)n);
    for (int wl : {0, 2}) {
      double v[2][4];
      sup_stats st;
      int k = 0;
      for (int threads : {1, 8}) {
        sup_opts o;
        sup_opts_init(&o);
        o.threads = threads;
        o.walk_log2 = wl;
        CHECK(sup_perman_complex_quad(a.data(), n, &o, 1, v[k], &st) == SUP_OK);
        CHECK(st.devices_used == 0 && st.gray_steps == (1ull << (n - 1)) && st.est_ops_per_step == 86.0 * n - 28.0);
        ++k;
      }
      CHECK(std::memcmp(v[0], v[1], sizeof(v[0])) == 0);
      CHECK(std::isfinite(v[0][0]) && std::isfinite(v[0][2]));
      CHECK(v[0][0] + v[0][1] == v[0][0] && v[0][2] + v[0][3] == v[0][2]);  // normalised pairs
      // aligned halves (quarters where there are four chunks), folded pairwise, then scaled
      const uint64_t C = 1ull << (n - 1 - st.lane_bits - st.walk_bits);
      for (uint64_t pieces : {(uint64_t)1, (uint64_t)2, (uint64_t)4}) {
        if (pieces > C) continue;
        std::vector<double> p(4 * pieces);
        for (uint64_t i = 0; i < pieces; ++i) {
          sup_opts o;
          sup_opts_init(&o);
          o.threads = i & 1 ? 8 : 1;
          o.walk_log2 = wl;
          sup_stats rs;
          CHECK(sup_perman_complex_quad_range(a.data(), n, i * (C / pieces), (i + 1) * (C / pieces), &o, 1, &p[4 * i],
                                              &rs) == SUP_OK);
          CHECK(rs.gray_steps == (C / pieces) << (rs.lane_bits + rs.walk_bits) && rs.devices_used == 0);
        }
        for (uint64_t w = pieces; w > 1; w /= 2)
          for (uint64_t i = 0; i < w / 2; ++i) {
            double t[4];
            dd_add(&p[8 * i], &p[8 * i + 4], t);
            dd_add(&p[8 * i + 2], &p[8 * i + 6], t + 2);
            std::memcpy(&p[4 * i], t, sizeof(t));
          }
        const double f = 4.0 * (n & 1) - 2.0;
        for (int q = 0; q < 4; ++q) CHECK(f * p[q] == v[0][q]);
      }
    }
  }
  // n = 1: the entry itself; n = 2 with small dyadic entries: exact
  const double one[2] = {3.0, -2.0};
  double v[4] = {9, 9, 9, 9};
  CHECK(sup_perman_complex_quad(one, 1, nullptr, 1, v, nullptr) == SUP_OK);
  CHECK(v[0] == 3.0 && v[1] == 0.0 && v[2] == -2.0 && v[3] == 0.0);
  const double two[8] = {1.0, 2.0, 3.0, -1.0, -2.0, 0.5, 0.25, 4.0};
  CHECK(sup_perman_complex_quad(two, 2, nullptr, 1, v, nullptr) == SUP_OK);
  CHECK(v[0] == -13.25 && v[1] == 0.0 && v[2] == 8.0 && v[3] == 0.0);
  // NaN propagates
  std::vector<double> bad = random_complex(7, 6);
  bad[5] = std::nan("");
  CHECK(sup_perman_complex_quad(bad.data(), 7, nullptr, 1, v, nullptr) == SUP_OK && std::isnan(v[0]) && std::isnan(v[2]));
}

static void test_arguments() {
  const std::vector<double> a = random_complex(7, 5);
  double v[4] = {0, 0, 0, 0};
  for (int on_cpu : {0, 1}) {  // the argument checks come before the cap and the device
    CHECK(sup_perman_complex_quad(nullptr, 7, nullptr, on_cpu, v, nullptr) == SUP_EINVAL);
    CHECK(sup_perman_complex_quad(a.data(), 7, nullptr, on_cpu, nullptr, nullptr) == SUP_EINVAL);
    CHECK(sup_perman_complex_quad(a.data(), 0, nullptr, on_cpu, v, nullptr) == SUP_EINVAL);
    CHECK(sup_perman_complex_quad(a.data(), -3, nullptr, on_cpu, v, nullptr) == SUP_EINVAL);
    CHECK(sup_perman_complex_quad(a.data(), 65, nullptr, on_cpu, v, nullptr) == SUP_EINVAL);
    CHECK(sup_perman_complex_quad_range(nullptr, 7, 0, 1, nullptr, on_cpu, v, nullptr) == SUP_EINVAL);
    CHECK(sup_perman_complex_quad_range(a.data(), 7, 0, 1, nullptr, on_cpu, nullptr, nullptr) == SUP_EINVAL);
    CHECK(sup_perman_complex_quad_range(a.data(), 65, 0, 1, nullptr, on_cpu, v, nullptr) == SUP_EINVAL);
    CHECK(sup_perman_complex_quad_range(a.data(), 0, 0, 1, nullptr, on_cpu, v, nullptr) == SUP_EINVAL);
    for (int wl : {32, -1}) {
      sup_opts o;
      sup_opts_init(&o);
      o.walk_log2 = wl;
      CHECK(sup_perman_complex_quad(a.data(), 7, &o, on_cpu, v, nullptr) == SUP_EINVAL);
      CHECK(sup_perman_complex_quad_range(a.data(), 7, 0, 1, &o, on_cpu, v, nullptr) == SUP_EINVAL);
    }
  }
  CHECK(sup_perman_complex_quad_range(a.data(), 7, 0, 2, nullptr, 1, v, nullptr) == SUP_EINVAL);  // one chunk
  CHECK(sup_perman_complex_quad_range(a.data(), 7, 1, 0, nullptr, 1, v, nullptr) == SUP_EINVAL);
  v[0] = v[1] = v[2] = v[3] = 9.0;
  CHECK(sup_perman_complex_quad_range(a.data(), 7, 1, 1, nullptr, 1, v, nullptr) == SUP_OK);
  CHECK(v[0] == 0.0 && v[1] == 0.0 && v[2] == 0.0 && v[3] == 0.0);
  // on_cpu = 0: above the cap SUP_EUNSUPPORTED with the cap in the message, on any machine
  const int big = SUP_CPLX_QUAD_MAX_DEVICE_N + 1;
  const std::vector<double> b = random_complex(big, 7);
  CHECK(sup_perman_complex_quad(b.data(), big, nullptr, 0, v, nullptr) == SUP_EUNSUPPORTED);
  CHECK(std::strstr(sup_last_error(), std::to_string(SUP_CPLX_QUAD_MAX_DEVICE_N).c_str()) != nullptr);
  CHECK(sup_perman_complex_quad_range(b.data(), big, 0, 1, nullptr, 0, v, nullptr) == SUP_EUNSUPPORTED);
  CHECK(sup_perman_complex_quad(b.data(), 64, nullptr, 0, v, nullptr) == SUP_EUNSUPPORTED);
  // the host twin serves it (two chunks of 2^7 subsets)
  sup_opts o;
  sup_opts_init(&o);
  o.walk_log2 = 1;
  o.threads = 8;
  CHECK(sup_perman_complex_quad_range(b.data(), big, 5, 7, &o, 1, v, nullptr) == SUP_OK && std::isfinite(v[0]));
  // at or below the cap a machine without a device answers SUP_ENODEV (no CPU fallback)
  int ndev = 0;
  if (sup_device_count(&ndev) != SUP_OK || ndev == 0) {
    CHECK(sup_perman_complex_quad(a.data(), 7, nullptr, 0, v, nullptr) == SUP_ENODEV);
    CHECK(sup_perman_complex_quad_range(a.data(), 7, 0, 1, nullptr, 0, v, nullptr) == SUP_ENODEV);
  }
}

int main() {
  test_perman();
  test_arguments();
  std::printf("selftest_complex_quad: %s (%d failed checks)\n", failures ? "FAILED" : "ok", failures);
  return failures ? 1 : 0;
}
