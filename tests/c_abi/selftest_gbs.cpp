// selftest_gbs.cpp — host-code self test of the ragged loop-hafnian batch and
// the PNR sampler for the sanitizer builds (make -C superman_amd/csrc
// sanitize-gbs: AddressSanitizer + UndefinedBehaviorSanitizer, and
// ThreadSanitizer).  No GPU is needed.  It drives, with on_cpu = 1 on 1 and 8
// host threads,
//   - sup_loop_hafnian_complex_each on 65 items of orders 0, 1, 2, 3, 7, 8, 16,
//     17 with repeats, shared and own mu rows: every item has the bits of
//     sup_loop_hafnian_complex on that item alone, order 0 is exactly 1, and
//     the thread count and the slab size change no bit;
//   - sup_gbs_sample: the vacuum and cutoff 0 give zeros, pieces drawn with
//     sample0 are the whole run, the thread count changes no sample, and
//     weights that overflow mark the sample with -1;
//   - the argument, symmetry, order, stride, row and index checks of both.
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

// A symmetric M x M matrix (interleaved) scaled by s, and rows x M complex numbers.
static void make_inputs(int M, int rows, double s, unsigned seed, std::vector<double>& A, std::vector<double>& mu) {
  std::mt19937_64 g(seed);
  std::normal_distribution<double> d(0.0, 1.0);
  A.assign((size_t)2 * M * M, 0.0);
  mu.assign((size_t)2 * M * rows, 0.0);
  for (int i = 0; i < M; ++i)
    for (int j = 0; j <= i; ++j)
      for (int p = 0; p < 2; ++p) A[2 * ((size_t)i * M + j) + p] = A[2 * ((size_t)j * M + i) + p] = s * d(g);
  for (double& v : mu) v = d(g);
}

static void test_each_bits() {
  const int M = 9, rows = 5, stride = 17;
  const int orders[8] = {0, 1, 2, 3, 7, 8, 16, 17};
  const int mod[4] = {2, M, 3, 1};
  std::vector<double> A, mu;
  make_inputs(M, rows, 1.0, 11, A, mu);
  const uint64_t count = 65;
  std::vector<int32_t> idx(count * stride, -7), n(count), mu_of(count);  // entries past n[k] are never read
  std::mt19937 g(5);
  for (uint64_t k = 0; k < count; ++k) {
    n[k] = orders[k % 8];
    mu_of[k] = k < 40 ? 2 : (int32_t)(k % rows);
    for (int j = 0; j < n[k]; ++j) idx[k * stride + j] = (int32_t)(g() % (unsigned)mod[k % 4]);
  }
  sup_opts o1 = opts(1), o8 = opts(8);
  std::vector<double> v1(2 * count, 9.0), v8(2 * count, 9.0), vs(2 * count, 9.0);
  sup_stats st;
  CHECK(sup_loop_hafnian_complex_each(A.data(), M, mu.data(), rows, mu_of.data(), idx.data(), stride, n.data(), count,
                                      &o1, 1, v1.data(), &st) == SUP_OK);
  CHECK(st.leaves == (int)count && st.visited_steps > 0 && st.est_ops_per_step > 0 && st.devices_used == 0);
  CHECK(sup_loop_hafnian_complex_each(A.data(), M, mu.data(), rows, mu_of.data(), idx.data(), stride, n.data(), count,
                                      &o8, 1, v8.data(), nullptr) == SUP_OK);
  CHECK(same_bits(v1, v8));
  setenv("SUP_HAFNIAN_SLAB", "3", 1);
  CHECK(sup_loop_hafnian_complex_each(A.data(), M, mu.data(), rows, mu_of.data(), idx.data(), stride, n.data(), count,
                                      &o8, 1, vs.data(), nullptr) == SUP_OK);
  unsetenv("SUP_HAFNIAN_SLAB");
  CHECK(same_bits(v1, vs));
  uint64_t terms = 0;
  for (uint64_t k = 0; k < count; ++k) {
    if (n[k] == 0) {
      CHECK(v1[2 * k] == 1.0 && v1[2 * k + 1] == 0.0 && !std::signbit(v1[2 * k + 1]));
      continue;
    }
    double one[2] = {0, 0};
    uint64_t t = 0;
    CHECK(sup_loop_hafnian_complex(A.data(), M, mu.data() + 2 * M * mu_of[k], idx.data() + k * stride, n[k], 1, &o1, 1,
                                   one, nullptr) == SUP_OK);
    CHECK(std::memcmp(one, &v1[2 * k], sizeof(one)) == 0);
    CHECK(sup_hafnian_complex_plan(idx.data() + k * stride, n[k], 1, &t) == SUP_OK);
    terms += t;
  }
  CHECK(st.visited_steps == terms);
  // mu_of = NULL: item k reads row k
  std::vector<double> w(2 * rows, 0.0);
  CHECK(sup_loop_hafnian_complex_each(A.data(), M, mu.data(), rows, nullptr, idx.data() + 3 * stride, stride,
                                      n.data() + 3, rows, &o8, 1, w.data(), nullptr) == SUP_OK);
  for (int k = 0; k < rows; ++k) {
    double one[2] = {0, 0};
    CHECK(sup_loop_hafnian_complex(A.data(), M, mu.data() + 2 * M * k, idx.data() + (3 + k) * stride, n[3 + k], 1, &o1,
                                   1, one, nullptr) == SUP_OK);
    CHECK(std::memcmp(one, &w[2 * k], sizeof(one)) == 0);
  }
}

static void test_each_arguments() {
  const int M = 64;
  std::vector<double> A, mu;
  make_inputs(M, 2, 1.0, 3, A, mu);
  double out[4] = {1, 1, 1, 1};
  int32_t idx[8] = {0, 1, 2, 3, 4, 5, 6, 7}, n[2] = {4, 3}, of[2] = {0, 1};
  auto call = [&](const double* a, int m, const double* u, uint64_t nmu, const int32_t* f, const int32_t* ix, int stride,
                  const int32_t* nn, uint64_t count, double* o) {
    return sup_loop_hafnian_complex_each(a, m, u, nmu, f, ix, stride, nn, count, nullptr, 1, o, nullptr);
  };
  CHECK(call(A.data(), M, mu.data(), 2, of, idx, 4, n, 2, out) == SUP_OK);
  CHECK(call(nullptr, M, mu.data(), 2, of, idx, 4, n, 2, out) == SUP_EINVAL);
  CHECK(call(A.data(), M, nullptr, 2, of, idx, 4, n, 2, out) == SUP_EINVAL);
  CHECK(call(A.data(), M, mu.data(), 2, of, nullptr, 4, n, 2, out) == SUP_EINVAL);
  CHECK(call(A.data(), M, mu.data(), 2, of, idx, 4, nullptr, 2, out) == SUP_EINVAL);
  CHECK(call(A.data(), M, mu.data(), 2, of, idx, 4, n, 2, nullptr) == SUP_EINVAL);
  CHECK(call(A.data(), 0, mu.data(), 2, of, idx, 4, n, 2, out) == SUP_EINVAL);
  out[0] = out[1] = 5.0;
  CHECK(call(A.data(), M, mu.data(), 2, of, idx, 4, n, 0, out) == SUP_OK);
  CHECK(out[0] == 5.0 && out[1] == 5.0);  // nothing written
  CHECK(call(A.data(), M, mu.data(), 2, of, idx, 3, n, 2, out) == SUP_EINVAL);
  CHECK(std::strstr(sup_last_error(), "stride = 3 < n[k = 0] = 4") != nullptr);
  n[1] = 65;
  CHECK(call(A.data(), M, mu.data(), 2, of, idx, 4, n, 2, out) == SUP_EINVAL);
  CHECK(std::strstr(sup_last_error(), "n[k = 1] = 65 outside [0, 64]") != nullptr);
  n[1] = -1;
  CHECK(call(A.data(), M, mu.data(), 2, of, idx, 4, n, 2, out) == SUP_EINVAL);
  n[1] = 3, of[1] = 2;
  CHECK(call(A.data(), M, mu.data(), 2, of, idx, 4, n, 2, out) == SUP_EINVAL);
  CHECK(std::strstr(sup_last_error(), "mu_of[k = 1] = 2 outside [0, 2)") != nullptr);
  of[1] = -1;
  CHECK(call(A.data(), M, mu.data(), 2, of, idx, 4, n, 2, out) == SUP_EINVAL);
  of[1] = 1;
  CHECK(call(A.data(), M, mu.data(), 1, nullptr, idx, 4, n, 2, out) == SUP_EINVAL);  // row 1 of one row
  idx[6] = 64;  // k = 1, position 2
  CHECK(call(A.data(), M, mu.data(), 2, of, idx, 4, n, 2, out) == SUP_EINVAL);
  CHECK(std::strstr(sup_last_error(), "idx[k = 1][position 2] = 64") != nullptr);
  idx[6] = 6, idx[7] = 64;  // position 3 >= n[1]: not read
  CHECK(call(A.data(), M, mu.data(), 2, of, idx, 4, n, 2, out) == SUP_OK);
  // 42 distinct indices: 2^25 wave-chunks, refused before any work
  std::vector<int32_t> id(2 * 42, 0);
  for (int j = 0; j < 42; ++j) id[42 + j] = j;
  int32_t n42[2] = {2, 42};
  CHECK(call(A.data(), M, mu.data(), 2, of, id.data(), 42, n42, 2, out) == SUP_EUNSUPPORTED);
  CHECK(std::strstr(sup_last_error(), "item k = 1") != nullptr);
  A[2 * (5 * 64 + 9) + 1] += 1.0;  // one asymmetric pair
  CHECK(call(A.data(), M, mu.data(), 2, of, idx, 4, n, 2, out) == SUP_EINVAL);
  CHECK(std::strstr(sup_last_error(), "A[5][9] and A[9][5] differ") != nullptr);
}

static void test_sampler() {
  const int M = 4, cutoff = 5;
  const uint64_t ns = 97, a = 33, seed = 2026;
  std::vector<double> B, zh;
  make_inputs(M, 2 * (int)ns, 0.25, 21, B, zh);  // rows [0, ns): zeta, rows [ns, 2 ns): het
  for (double& v : zh) v *= 0.4;
  const double* zeta = zh.data();
  const double* het = zh.data() + 2 * M * ns;
  sup_opts o1 = opts(1), o8 = opts(8);
  std::vector<int32_t> whole(ns * M, 99), again(ns * M, 99), parts(ns * M, 99);
  sup_stats st;
  CHECK(sup_gbs_sample(B.data(), M, zeta, het, cutoff, ns, 0, seed, &o8, 1, whole.data(), &st) == SUP_OK);
  CHECK(st.leaves == (int)ns && st.visited_steps > 0 && st.partials[2] == 0.0 && st.devices_used == 0);
  int top = 0;
  for (int32_t v : whole) {
    CHECK(v >= 0 && v <= cutoff);
    top = v > top ? v : top;
  }
  CHECK(top >= 2);
  CHECK(sup_gbs_sample(B.data(), M, zeta, het, cutoff, ns, 0, seed, &o1, 1, again.data(), nullptr) == SUP_OK);
  CHECK(whole == again);
  CHECK(sup_gbs_sample(B.data(), M, zeta, het, cutoff, a, 0, seed, &o8, 1, parts.data(), nullptr) == SUP_OK);
  CHECK(sup_gbs_sample(B.data(), M, zeta + 2 * M * a, het + 2 * M * a, cutoff, ns - a, a, seed, &o8, 1,
                       parts.data() + a * M, nullptr) == SUP_OK);
  CHECK(whole == parts);
  CHECK(sup_gbs_sample(B.data(), M, zeta, het, cutoff, ns, 0, seed + 1, &o8, 1, again.data(), nullptr) == SUP_OK);
  CHECK(whole != again);
  // cutoff 0 and the vacuum: zeros
  CHECK(sup_gbs_sample(B.data(), M, zeta, het, 0, ns, 0, seed, &o8, 1, again.data(), nullptr) == SUP_OK);
  for (int32_t v : again) CHECK(v == 0);
  std::vector<double> zero((size_t)2 * M * ns, 0.0), B0((size_t)2 * M * M, 0.0);
  CHECK(sup_gbs_sample(B0.data(), M, zero.data(), zero.data(), cutoff, ns, 0, seed, &o8, 1, again.data(), nullptr) == SUP_OK);
  for (int32_t v : again) CHECK(v == 0);
  // weights that overflow: -1 from that mode on, counted
  std::vector<double> big(zh.begin(), zh.begin() + 2 * M * 3);
  big[2 * (M + 1)] = 1e200;  // sample 1, mode 1
  int32_t three[3 * M];
  CHECK(sup_gbs_sample(B.data(), M, big.data(), het, cutoff, 3, 0, seed, &o8, 1, three, &st) == SUP_OK);
  CHECK(st.partials[2] == 1.0 && three[M] >= 0 && three[M + 1] == -1 && three[M + 2] == -1 && three[M + 3] == -1);
  for (int j = 0; j < M; ++j) CHECK(three[j] == whole[j] && three[2 * M + j] == whole[2 * M + j]);
  // a prefix of 60 photons: the candidates above order 64 have weight 0 and are never drawn
  std::vector<double> z64(2 * 2, 0.0), h64(2 * 2, 0.0), Bd(2 * 2 * 2, 0.0);
  z64[0] = 7.5, z64[2] = 7.5;  // coherent amplitudes: about 56 photons a mode
  int32_t two[2];
  CHECK(sup_gbs_sample(Bd.data(), 2, z64.data(), h64.data(), 64, 1, 0, 1, &o8, 1, two, nullptr) == SUP_OK);
  CHECK(two[0] >= 30 && two[0] <= 64 && two[1] >= 0 && two[0] + two[1] <= 64);
  // arguments
  CHECK(sup_gbs_sample(nullptr, M, zeta, het, cutoff, ns, 0, seed, nullptr, 1, whole.data(), nullptr) == SUP_EINVAL);
  CHECK(sup_gbs_sample(B.data(), 0, zeta, het, cutoff, ns, 0, seed, nullptr, 1, whole.data(), nullptr) == SUP_EINVAL);
  CHECK(sup_gbs_sample(B.data(), 65, zeta, het, cutoff, ns, 0, seed, nullptr, 1, whole.data(), nullptr) == SUP_EINVAL);
  CHECK(sup_gbs_sample(B.data(), M, zeta, het, -1, ns, 0, seed, nullptr, 1, whole.data(), nullptr) == SUP_EINVAL);
  CHECK(sup_gbs_sample(B.data(), M, zeta, het, 65, ns, 0, seed, nullptr, 1, whole.data(), nullptr) == SUP_EINVAL);
  CHECK(sup_gbs_sample(B.data(), M, nullptr, nullptr, cutoff, 0, 0, seed, nullptr, 1, nullptr, nullptr) == SUP_OK);
  CHECK(sup_gbs_sample(B.data(), M, nullptr, het, cutoff, ns, 0, seed, nullptr, 1, whole.data(), nullptr) == SUP_EINVAL);
  CHECK(sup_gbs_sample(B.data(), M, zeta, nullptr, cutoff, ns, 0, seed, nullptr, 1, whole.data(), nullptr) == SUP_EINVAL);
  CHECK(sup_gbs_sample(B.data(), M, zeta, het, cutoff, ns, 0, seed, nullptr, 1, nullptr, nullptr) == SUP_EINVAL);
  B[2 * (1 * M + 2)] += 1.0;
  CHECK(sup_gbs_sample(B.data(), M, zeta, het, cutoff, ns, 0, seed, nullptr, 1, whole.data(), nullptr) == SUP_EINVAL);
  CHECK(std::strstr(sup_last_error(), "B[1][2] and B[2][1] differ") != nullptr);
}

int main() {
  test_each_bits();
  test_each_arguments();
  test_sampler();
  std::printf("selftest_gbs: %s (%d failed checks)\n", failures ? "FAILED" : "ok", failures);
  return failures ? 1 : 0;
}
