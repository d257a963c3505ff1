// selftest_threshold_chain.cpp — host-code self test of the ragged loop
// torontonian batch and the threshold-detector sampler for the sanitizer builds
// (make -C superman_amd/csrc sanitize-threshold-chain: AddressSanitizer +
// UndefinedBehaviorSanitizer, and ThreadSanitizer).  No GPU is needed.  It
// drives, with on_cpu = 1 on 1 and 8 host threads,
//   - sup_loop_torontonian_each on 60 items of orders 0, 1, 3, 4, 5, 6, 7, 9,
//     10, 12 with shared and own gamma rows: every item has the bits of
//     sup_loop_torontonian on that item alone, order 0 is exactly 1, and the
//     thread count and the slab size change no bit;
//   - sup_threshold_sample: the vacuum gives zeros, pieces drawn with sample0
//     are the whole run, the thread count changes no sample or weight, and a
//     NaN in zeta marks the sample with -1;
//   - the argument, order, stride, row, mode and knob checks of both.
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

// A Hermitian 2M x 2M matrix (interleaved) with entries of size s (diagonally
// dominant below 1 for small s: I - O_z stays positive definite), and rows x 2M
// complex numbers of size g.
static void make_inputs(int M, int rows, double s, double g, unsigned seed, std::vector<double>& O, std::vector<double>& gam) {
  std::mt19937_64 gen(seed);
  std::uniform_real_distribution<double> d(-1.0, 1.0);
  const int N = 2 * M;
  O.assign((size_t)2 * N * N, 0.0);
  gam.assign((size_t)2 * N * rows, 0.0);
  for (int i = 0; i < N; ++i)
    for (int j = 0; j <= i; ++j) {
      const double re = s * d(gen), im = i == j ? 0.0 : s * d(gen);
      O[2 * ((size_t)i * N + j)] = re, O[2 * ((size_t)i * N + j) + 1] = im;
      O[2 * ((size_t)j * N + i)] = re, O[2 * ((size_t)j * N + i) + 1] = -im;
    }
  for (double& v : gam) v = g * d(gen);
}

static void test_each_bits() {
  const int M = 13, rows = 5, stride = 12;
  const int orders[10] = {0, 1, 3, 4, 5, 6, 7, 9, 10, 12};
  std::vector<double> O, gam;
  make_inputs(M, rows, 0.02, 0.3, 11, O, gam);
  const uint64_t count = 60;
  std::vector<int32_t> modes(count * stride, -7), n(count), of(count);  // entries past n[k] are never read
  std::mt19937 g(5);
  for (uint64_t k = 0; k < count; ++k) {
    n[k] = orders[k % 10];
    of[k] = k < 40 ? 2 : (int32_t)(k % rows);
    int32_t perm[M];
    for (int j = 0; j < M; ++j) perm[j] = j;
    for (int j = M - 1; j > 0; --j) std::swap(perm[j], perm[g() % (unsigned)(j + 1)]);
    for (int j = 0; j < n[k]; ++j) modes[k * stride + j] = perm[j];
  }
  sup_opts o1 = opts(1), o8 = opts(8);
  std::vector<double> v1(count, 9.0), v8(count, 9.0), vs(count, 9.0);
  sup_stats st;
  CHECK(sup_loop_torontonian_each(O.data(), M, gam.data(), rows, of.data(), modes.data(), stride, n.data(), count, &o1, 1,
                                  v1.data(), &st) == SUP_OK);
  CHECK(st.leaves == (int)count && st.visited_steps > 0 && st.est_ops_per_step > 0 && st.devices_used == 0);
  CHECK(sup_loop_torontonian_each(O.data(), M, gam.data(), rows, of.data(), modes.data(), stride, n.data(), count, &o8, 1,
                                  v8.data(), nullptr) == SUP_OK);
  CHECK(same_bits(v1, v8));
  for (const char* slab : {"1", "3"}) {
    setenv("SUP_LTOR_EACH_SLAB", slab, 1);
    CHECK(sup_loop_torontonian_each(O.data(), M, gam.data(), rows, of.data(), modes.data(), stride, n.data(), count, &o8,
                                    1, vs.data(), nullptr) == SUP_OK);
    CHECK(same_bits(v1, vs));
  }
  unsetenv("SUP_LTOR_EACH_SLAB");
  uint64_t subsets = 0;
  for (uint64_t k = 0; k < count; ++k) {
    if (n[k] == 0) {
      CHECK(v1[k] == 1.0);
      continue;
    }
    double one = 0.0;
    CHECK(sup_loop_torontonian(O.data(), M, gam.data() + 4 * M * of[k], modes.data() + k * stride, n[k], 1, &o1, 1, &one,
                               nullptr) == SUP_OK);
    CHECK(std::memcmp(&one, &v1[k], sizeof(one)) == 0 && std::isfinite(one));
    subsets += 1ull << n[k];
  }
  CHECK(st.visited_steps == subsets && st.gray_steps == subsets);
  // gamma_of = NULL: item k reads row k
  std::vector<double> w(rows, 0.0);
  CHECK(sup_loop_torontonian_each(O.data(), M, gam.data(), rows, nullptr, modes.data() + 3 * stride, stride, n.data() + 3,
                                  rows, &o8, 1, w.data(), nullptr) == SUP_OK);
  for (int k = 0; k < rows; ++k) {
    double one = 0.0;
    CHECK(sup_loop_torontonian(O.data(), M, gam.data() + 4 * M * k, modes.data() + (3 + k) * stride, n[3 + k], 1, &o1, 1,
                               &one, nullptr) == SUP_OK);
    CHECK(std::memcmp(&one, &w[k], sizeof(one)) == 0);
  }
}

static void test_each_arguments() {
  const int M = 40;
  std::vector<double> O, gam;
  make_inputs(M, 2, 0.005, 0.2, 3, O, gam);
  double out[2] = {5, 5};
  int32_t modes[8] = {0, 1, 2, 3, 4, 5, 6, 7}, n[2] = {4, 3}, of[2] = {0, 1};
  auto call = [&](const double* o, int m, const double* g, uint64_t ng, const int32_t* f, const int32_t* md, int stride,
                  const int32_t* nn, uint64_t count, double* res) {
    return sup_loop_torontonian_each(o, m, g, ng, f, md, stride, nn, count, nullptr, 1, res, nullptr);
  };
  CHECK(call(O.data(), M, gam.data(), 2, of, modes, 4, n, 2, out) == SUP_OK);
  CHECK(call(nullptr, M, gam.data(), 2, of, modes, 4, n, 2, out) == SUP_EINVAL);
  CHECK(call(O.data(), M, nullptr, 2, of, modes, 4, n, 2, out) == SUP_EINVAL);
  CHECK(call(O.data(), M, gam.data(), 2, of, nullptr, 4, n, 2, out) == SUP_EINVAL);
  CHECK(call(O.data(), M, gam.data(), 2, of, modes, 4, nullptr, 2, out) == SUP_EINVAL);
  CHECK(call(O.data(), M, gam.data(), 2, of, modes, 4, n, 2, nullptr) == SUP_EINVAL);
  CHECK(call(O.data(), 0, gam.data(), 2, of, modes, 4, n, 2, out) == SUP_EINVAL);
  out[0] = out[1] = 5.0;
  CHECK(call(O.data(), M, gam.data(), 2, of, modes, 4, n, 0, out) == SUP_OK);
  CHECK(out[0] == 5.0 && out[1] == 5.0);  // nothing written
  CHECK(call(O.data(), M, gam.data(), 2, of, modes, 3, n, 2, out) == SUP_EINVAL);
  CHECK(std::strstr(sup_last_error(), "stride = 3 < n[k = 0] = 4") != nullptr);
  std::vector<int32_t> wide(2 * 33);
  for (int j = 0; j < 66; ++j) wide[j] = j % 33;
  n[1] = 33;
  CHECK(call(O.data(), M, gam.data(), 2, of, wide.data(), 33, n, 2, out) == SUP_EINVAL);
  CHECK(std::strstr(sup_last_error(), "n[k = 1] = 33 outside [0, 32]") != nullptr);
  n[1] = -1;
  CHECK(call(O.data(), M, gam.data(), 2, of, modes, 4, n, 2, out) == SUP_EINVAL);
  n[1] = 3, of[1] = 2;
  CHECK(call(O.data(), M, gam.data(), 2, of, modes, 4, n, 2, out) == SUP_EINVAL);
  CHECK(std::strstr(sup_last_error(), "gamma_of[k = 1] = 2 outside [0, 2)") != nullptr);
  of[1] = -1;
  CHECK(call(O.data(), M, gam.data(), 2, of, modes, 4, n, 2, out) == SUP_EINVAL);
  of[1] = 1;
  CHECK(call(O.data(), M, gam.data(), 1, nullptr, modes, 4, n, 2, out) == SUP_EINVAL);  // row 1 of one row
  modes[6] = 40;  // k = 1, position 2
  CHECK(call(O.data(), M, gam.data(), 2, of, modes, 4, n, 2, out) == SUP_EINVAL);
  CHECK(std::strstr(sup_last_error(), "modes[k = 1][position 2] = 40") != nullptr);
  modes[6] = 4;  // mode 4 at positions 0 and 2 of list 1
  CHECK(call(O.data(), M, gam.data(), 2, of, modes, 4, n, 2, out) == SUP_EINVAL);
  CHECK(std::strstr(sup_last_error(), "positions 0 and 2") != nullptr);
  modes[6] = 6, modes[7] = 99;  // position 3 >= n[1]: not read
  CHECK(call(O.data(), M, gam.data(), 2, of, modes, 4, n, 2, out) == SUP_OK);
  // every error comes before any work: the order-0 item ahead of a bad one is not written
  int32_t n0[2] = {0, 5};
  out[0] = out[1] = 5.0;
  CHECK(call(O.data(), M, gam.data(), 2, of, modes, 4, n0, 2, out) == SUP_EINVAL);
  CHECK(out[0] == 5.0 && out[1] == 5.0);
  for (const char* knob : {"0", "-1", "x", "3 "}) {
    setenv("SUP_LTOR_EACH_SLAB", knob, 1);
    CHECK(call(O.data(), M, gam.data(), 2, of, modes, 4, n, 2, out) == SUP_EINVAL);
    CHECK(std::strstr(sup_last_error(), "SUP_LTOR_EACH_SLAB") != nullptr);
  }
  unsetenv("SUP_LTOR_EACH_SLAB");
  // 32 modes: the largest order the entry takes is checked and planned (not walked here)
  CHECK(call(O.data(), M, gam.data(), 2, of, modes, 4, n, 2, out) == SUP_OK);
}

static void test_sampler() {
  const int M = 4;
  const uint64_t ns = 97, a = 33, seed = 2028;
  std::mt19937_64 gen(21);
  std::normal_distribution<double> d(0.0, 1.0);
  std::vector<double> B((size_t)2 * M * M), zh((size_t)2 * M * 2 * ns);
  for (int i = 0; i < M; ++i)
    for (int j = 0; j <= i; ++j)
      for (int p = 0; p < 2; ++p) B[2 * ((size_t)i * M + j) + p] = B[2 * ((size_t)j * M + i) + p] = 0.12 * d(gen);
  for (double& v : zh) v = 0.5 * d(gen);  // rows [0, ns): zeta, rows [ns, 2 ns): het
  const double* zeta = zh.data();
  const double* het = zh.data() + 2 * M * ns;
  sup_opts o1 = opts(1), o8 = opts(8);
  std::vector<int32_t> whole(ns * M, 99), again(ns * M, 99), parts(ns * M, 99);
  std::vector<double> w8(ns * M * 2, 9.0), w1(ns * M * 2, 9.0);
  sup_stats st;
  CHECK(sup_threshold_sample(B.data(), M, zeta, het, ns, 0, seed, &o8, 1, whole.data(), w8.data(), &st) == SUP_OK);
  CHECK(st.leaves == (int)ns && st.visited_steps > 0 && st.partials[2] == 0.0 && st.devices_used == 0);
  int clicks = 0;
  for (int32_t v : whole) {
    CHECK(v == 0 || v == 1);
    clicks += v;
  }
  CHECK(clicks > 20 && clicks < (int)(ns * M) - 20);
  for (double v : w8) CHECK(v >= 0.0 && !std::signbit(v));
  CHECK(sup_threshold_sample(B.data(), M, zeta, het, ns, 0, seed, &o1, 1, again.data(), w1.data(), nullptr) == SUP_OK);
  CHECK(whole == again && same_bits(w1, w8));
  CHECK(sup_threshold_sample(B.data(), M, zeta, het, a, 0, seed, &o8, 1, parts.data(), nullptr, nullptr) == SUP_OK);
  CHECK(sup_threshold_sample(B.data(), M, zeta + 2 * M * a, het + 2 * M * a, ns - a, a, seed, &o8, 1, parts.data() + a * M,
                             nullptr, nullptr) == SUP_OK);
  CHECK(whole == parts);
  CHECK(sup_threshold_sample(B.data(), M, zeta, het, ns, 0, seed + 1, &o8, 1, again.data(), nullptr, nullptr) == SUP_OK);
  CHECK(whole != again);
  // the vacuum: zeros
  std::vector<double> zero((size_t)2 * M * ns, 0.0), B0((size_t)2 * M * M, 0.0);
  CHECK(sup_threshold_sample(B0.data(), M, zero.data(), zero.data(), ns, 0, seed, &o8, 1, again.data(), nullptr, nullptr) ==
        SUP_OK);
  for (int32_t v : again) CHECK(v == 0);
  // a NaN in zeta_1 of sample 1: -1 from mode 1 on, counted; its neighbours are the whole run's
  std::vector<double> bad(zh.begin(), zh.begin() + 2 * M * 3);
  bad[2 * (M + 1)] = std::nan("");
  int32_t three[3 * M];
  double w3[3 * M * 2];
  CHECK(sup_threshold_sample(B.data(), M, bad.data(), het, 3, 0, seed, &o8, 1, three, w3, &st) == SUP_OK);
  CHECK(st.partials[2] == 1.0 && three[M] == whole[M] && three[M + 1] == -1 && three[M + 2] == -1 && three[M + 3] == -1);
  CHECK(w3[2 * (M + 2)] == 0.0 && w3[2 * (M + 3) + 1] == 0.0);
  for (int j = 0; j < M; ++j) CHECK(three[j] == whole[j] && three[2 * M + j] == whole[2 * M + j]);
  // arguments
  CHECK(sup_threshold_sample(nullptr, M, zeta, het, ns, 0, seed, nullptr, 1, whole.data(), nullptr, nullptr) == SUP_EINVAL);
  CHECK(sup_threshold_sample(B.data(), 0, zeta, het, ns, 0, seed, nullptr, 1, whole.data(), nullptr, nullptr) == SUP_EINVAL);
  CHECK(sup_threshold_sample(B.data(), 65, zeta, het, ns, 0, seed, nullptr, 1, whole.data(), nullptr, nullptr) == SUP_EINVAL);
  CHECK(sup_threshold_sample(B.data(), M, nullptr, nullptr, 0, 0, seed, nullptr, 1, nullptr, nullptr, nullptr) == SUP_OK);
  CHECK(sup_threshold_sample(B.data(), M, nullptr, het, ns, 0, seed, nullptr, 1, whole.data(), nullptr, nullptr) == SUP_EINVAL);
  CHECK(sup_threshold_sample(B.data(), M, zeta, nullptr, ns, 0, seed, nullptr, 1, whole.data(), nullptr, nullptr) == SUP_EINVAL);
  CHECK(sup_threshold_sample(B.data(), M, zeta, het, ns, 0, seed, nullptr, 1, nullptr, nullptr, nullptr) == SUP_EINVAL);
  B[2 * (1 * M + 2)] += 1.0;
  CHECK(sup_threshold_sample(B.data(), M, zeta, het, ns, 0, seed, nullptr, 1, whole.data(), nullptr, nullptr) == SUP_EINVAL);
  CHECK(std::strstr(sup_last_error(), "B[1][2] and B[2][1] differ") != nullptr);
}

int main() {
  test_each_bits();
  test_each_arguments();
  test_sampler();
  std::printf("selftest_threshold_chain: %s (%d failed checks)\n", failures ? "FAILED" : "ok", failures);
  return failures ? 1 : 0;
}
