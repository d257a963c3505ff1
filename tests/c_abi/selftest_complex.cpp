// selftest_complex.cpp — host-code self test of the complex-permanent entry
// points for the sanitizer builds (make -C superman_amd/csrc sanitize-complex:
// AddressSanitizer + UndefinedBehaviorSanitizer, and ThreadSanitizer).  No GPU
// is needed.  It drives
//   - sup_read_mtx_complex on good files (general, symmetric, hermitian,
//     comments, duplicates) and on malformed ones (every refusal frees what it
//     allocated);
//   - sup_perman_complex and sup_perman_complex_range with on_cpu = 1 at
//     n = 1, 7, 12 on 1 and 8 host threads: the thread count changes no bit,
//     and aligned ranges folded pairwise reproduce the whole sum;
//   - the argument checks.
// Usage: selftest_complex [scratch directory, default /tmp]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include <unistd.h>

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

static std::string write_file(const std::string& dir, const char* name, const std::string& text) {
  const std::string path = dir + "/sup_selftest_complex_" + std::to_string((long)getpid()) + "_" + name;
  if (FILE* f = std::fopen(path.c_str(), "w")) {
    std::fputs(text.c_str(), f);
    std::fclose(f);
  } else {
    std::fprintf(stderr, "cannot write %s\n", path.c_str());
    ++failures;
  }
  return path;
}

static void test_reader(const std::string& dir) {
  const std::string head = "%%MatrixMarket matrix coordinate complex ";
  const std::string body = "% a comment\n3 3 4\n1 1 2.0 0.0\n2 1 1.5 -0.5\n3 1 0.0 2.0\n2 1 1.0 0.25\n";
  struct Good {
    const char* sym;
    double re12, im12;  // entry (1, 2), 1-based: the mirror of the last (2, 1)
  } good[] = {{"general", 0.0, 0.0}, {"symmetric", 1.0, 0.25}, {"hermitian", 1.0, -0.25}};
  for (const Good& g : good) {
    const std::string p = write_file(dir, g.sym, head + g.sym + "\n" + body);
    double* m = nullptr;
    int n = 0, nz = 0;
    CHECK(sup_read_mtx_complex(p.c_str(), &m, &n, &nz) == SUP_OK);
    CHECK(n == 3 && nz == 4);
    if (m) {
      CHECK(m[0] == 2.0 && m[1] == 0.0);
      CHECK(m[2 * 3] == 1.0 && m[2 * 3 + 1] == 0.25);  // (2, 1): the later duplicate won
      CHECK(m[2 * 1] == g.re12 && m[2 * 1 + 1] == g.im12);
      sup_free(m);
    }
    unlink(p.c_str());
  }
  const std::pair<const char*, std::string> bad[] = {
      {"skew", head + "skew-symmetric\n2 2 1\n2 1 1.0 1.0\n"},
      {"real", "%%MatrixMarket matrix coordinate real general\n2 2 1\n1 1 1.0\n"},
      {"array", "%%MatrixMarket matrix array complex general\n2 2\n1.0 0.0\n"},
      {"nonsquare", head + "general\n2 3 1\n1 1 1.0 0.0\n"},
      {"truncated", head + "general\n2 2 3\n1 1 1.0 0.0\n2 2 1.0\n"},
      {"range", head + "general\n2 2 2\n1 1 1.0 0.0\n3 1 1.0 0.0\n"},
      {"hermdiag", head + "hermitian\n2 2 2\n2 1 1.0 1.0\n1 1 1.0 0.5\n"},
      {"large", head + "general\n65 65 1\n1 1 1.0 0.0\n"},
      {"nosize", head + "general\n"},
      {"banner", "%MatrixMarket matrix coordinate complex general\n1 1 1\n1 1 1.0 0.0\n"},
      {"empty", ""},
  };
  for (const auto& b : bad) {
    const std::string p = write_file(dir, b.first, b.second);
    double* m = nullptr;
    int n = 0;
    CHECK(sup_read_mtx_complex(p.c_str(), &m, &n, nullptr) == SUP_EIO);
    CHECK(m == nullptr);
    unlink(p.c_str());
  }
  double* m = nullptr;
  int n = 0;
  CHECK(sup_read_mtx_complex((dir + "/sup_selftest_complex_no_such_file").c_str(), &m, &n, nullptr) == SUP_EIO);
  CHECK(sup_read_mtx_complex(nullptr, &m, &n, nullptr) == SUP_EINVAL);
  CHECK(sup_read_mtx_complex("x", nullptr, &n, nullptr) == SUP_EINVAL);
}

static std::vector<double> random_complex(int n, unsigned seed) {
  std::mt19937_64 g(seed);
  std::normal_distribution<double> d(0.0, 1.0);
  std::vector<double> a((size_t)2 * n * n);
  for (auto& v : a) v = d(g);
  return a;
}

static void test_perman() {
  for (int n : {1, 7, 12}) {
    const std::vector<double> a = random_complex(n, 100u + (unsigned)n);
    for (int wl : {0, 2}) {
      double re[2] = {0, 0}, im[2] = {0, 0};
      sup_stats st;
      int k = 0;
      for (int threads : {1, 8}) {
        sup_opts o;
        sup_opts_init(&o);
        o.threads = threads;
        o.walk_log2 = wl;
        CHECK(sup_perman_complex(a.data(), n, &o, 1, &re[k], &im[k], &st) == SUP_OK);
        CHECK(st.devices_used == 0 && st.gray_steps == (1ull << (n - 1)) && st.est_ops_per_step == 6.0 * n);
        ++k;
      }
      CHECK(re[0] == re[1] && im[0] == im[1]);
      CHECK(std::isfinite(re[0]) && std::isfinite(im[0]));
      // aligned halves (quarters where there are four chunks), folded pairwise, then scaled
      const uint64_t C = 1ull << (n - 1 - st.lane_bits - st.walk_bits);
      for (uint64_t pieces : {(uint64_t)1, (uint64_t)2, (uint64_t)4}) {
        if (pieces > C) continue;
        std::vector<double> pr(pieces), pi(pieces);
        for (uint64_t i = 0; i < pieces; ++i) {
          sup_opts o;
          sup_opts_init(&o);
          o.threads = i & 1 ? 8 : 1;
          o.walk_log2 = wl;
          CHECK(sup_perman_complex_range(a.data(), n, i * (C / pieces), (i + 1) * (C / pieces), &o, 1, &pr[i], &pi[i],
                                         nullptr) == SUP_OK);
        }
        for (uint64_t w = pieces; w > 1; w /= 2)
          for (uint64_t i = 0; i < w / 2; ++i) pr[i] = pr[2 * i] + pr[2 * i + 1], pi[i] = pi[2 * i] + pi[2 * i + 1];
        const double f = 4.0 * (n & 1) - 2.0;
        CHECK(f * pr[0] == re[0] && f * pi[0] == im[0]);
      }
    }
  }
  // n = 1: the entry itself
  const double one[2] = {3.0, -2.0};
  double re = 0, im = 0;
  CHECK(sup_perman_complex(one, 1, nullptr, 1, &re, &im, nullptr) == SUP_OK && re == 3.0 && im == -2.0);
}

static void test_arguments() {
  const std::vector<double> a = random_complex(7, 5);
  double re = 0, im = 0;
  CHECK(sup_perman_complex(nullptr, 7, nullptr, 1, &re, &im, nullptr) == SUP_EINVAL);
  CHECK(sup_perman_complex(a.data(), 7, nullptr, 1, nullptr, &im, nullptr) == SUP_EINVAL);
  CHECK(sup_perman_complex(a.data(), 7, nullptr, 1, &re, nullptr, nullptr) == SUP_EINVAL);
  CHECK(sup_perman_complex(a.data(), 0, nullptr, 1, &re, &im, nullptr) == SUP_EINVAL);
  CHECK(sup_perman_complex(a.data(), 65, nullptr, 1, &re, &im, nullptr) == SUP_EINVAL);
  CHECK(sup_perman_complex_range(a.data(), 65, 0, 1, nullptr, 1, &re, &im, nullptr) == SUP_EINVAL);
  CHECK(sup_perman_complex_range(a.data(), 7, 0, 2, nullptr, 1, &re, &im, nullptr) == SUP_EINVAL);  // one chunk
  CHECK(sup_perman_complex_range(a.data(), 7, 1, 0, nullptr, 1, &re, &im, nullptr) == SUP_EINVAL);
  CHECK(sup_perman_complex_range(a.data(), 7, 1, 1, nullptr, 1, &re, &im, nullptr) == SUP_OK && re == 0.0 && im == 0.0);
  sup_opts o;
  sup_opts_init(&o);
  o.walk_log2 = 32;
  CHECK(sup_perman_complex(a.data(), 7, &o, 1, &re, &im, nullptr) == SUP_EINVAL);
}

int main(int argc, char** argv) {
  const std::string dir = argc > 1 ? argv[1] : "/tmp";
  test_reader(dir);
  test_perman();
  test_arguments();
  std::printf("selftest_complex: %s (%d failed checks)\n", failures ? "FAILED" : "ok", failures);
  return failures ? 1 : 0;
}
