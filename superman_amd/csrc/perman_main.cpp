// perman_main.cpp — the `perman` command line, a drop-in for the reference's
// v1 CLI (main.cu:325-600): same short/long options, same algorithm ids, same
// "Result: <name> <perm> in <sec>" line (cout default precision), plus a
// full-precision "Permanent: %.17e" line (the legacy line has ~6 digits).
//
// Extensions (v2 semantics, revised_perman/main.cpp:1298-1476): -l <dev>
// first device, -k <reps> repetitions, -o compression (d1/d2 singletons, then
// the d1/d2/d34 expansion while n > 30), -u <t> scaling; MatrixMarket input
// (detected by its banner, read as main.cpp:1515-1615).  Own additions: -R
// insist on the RCCL combine of multi-GPU partials (by default it runs
// whenever the -d devices are distinct GPUs, else the host pairwise tree); -v per-kernel / per-chunk timing;
// --seed (-S) the estimators' Philox seed (-a / -i; the reference seeds with
// time(0), so its estimates are not reproducible); --jit (-J) <-1|0|1> the
// pattern-specialised segmented walk (sup_opts.jit: never / auto / whenever
// its cost model wins); --exact (-E) the exact integer permanent of an int /
// -b (binary) matrix (sup_perman_exact: residue walk + CRT; the reference's
// int path is fp64): on -g with -p5/-p6 it uses -d devices, with -c alone
// the -t host threads.  -q (v2's quad calculation, main.cpp:141-142): the
// dense walk in double-double (sup_perman_quad), -d devices with -p5/-p6,
// -t host threads with -c; with -o / -u every leaf and the combine in
// double-double (sup_perman_reduced_quad); prints hi and the hi + lo pair.
// --complex (no short letter): the permanent of a MatrixMarket `complex`
// file (sup_read_mtx_complex + sup_perman_complex): the dense walk over
// complex fp64 values on -d devices from -l with -g, on -t host threads with
// -c; prints "Permanent: <re> <im>".  It does not combine with -s, -o, -u,
// -E, -q, -a, -b, -i or -r.
// --complex-quad (no short letter): the same file through
// sup_perman_complex_quad, the complex walk in double-double (on the device up
// to n = SUP_CPLX_QUAD_MAX_DEVICE_N, on -t host threads with -c up to 64);
// prints "Permanent (double-double): <re_hi> <re_lo> <im_hi> <im_lo>".  Refused
// with the options --complex is refused with; --complex beside it changes
// nothing.
// --complex-exact (no short letter): the same file, whose parts must be
// integers, through sup_perman_complex_exact (residue walk over (Z/p)[i] and
// CRT; on the device up to n = SUP_CPLX_EXACT_MAX_DEVICE_N, on -t host threads
// with -c up to 64); prints "Permanent (exact): <re> <im>", two decimal
// integers.  Refused with the options --complex is refused with and with
// --complex-quad; --complex beside it changes nothing.
// --hafnian [--loop] [--rpt 2,0,1,...] (no short letters): the hafnian (--loop:
// the loop hafnian, mu = the diagonal) of the same kind of file, which must be
// symmetric, through sup_hafnian_complex / sup_loop_hafnian_complex; --rpt
// takes mode k rpt[k] times (default: every mode once).  -g the device walk,
// -c the host threads; prints "Hafnian: <re> <im>".  Refused with the options
// --complex is refused with and with the --complex flags.
// --hafnian --powertrace: the same value through sup_hafnian_complex_pt /
// sup_loop_hafnian_complex_pt (2^(n/2) subsets instead of 2^(n-1) states; on
// the device up to n = SUP_HAFNIAN_PT_MAX_DEVICE_N, with -c up to 64).
// --hafnian --exact [--loop] [--rpt ...]: the exact value of a file whose parts
// are integers, through sup_hafnian_complex_exact (residue walk and CRT, -g or
// -c, n <= 64); prints "Hafnian (exact): <re> <im>", two decimal integers.
// Refused with --powertrace.
// --hafnian --quad [--loop] [--rpt ...]: the same value in complex double-double
// through sup_hafnian_complex_quad / sup_loop_hafnian_complex_quad (-g or -c);
// prints "Hafnian (double-double): <re_hi> <re_lo> <im_hi> <im_lo>".  Only the
// long spelling selects it (-q beside --hafnian stays refused); refused with
// --powertrace and with --exact.
// --torontonian [--modes 0,3,5]: sup_torontonian of a 2M x 2M Hermitian
// MatrixMarket `complex` file (thewalrus' ordering) on the listed distinct
// modes (default: all M); prints "Torontonian: <value>".  -g the device
// kernel, -c the host threads.
// --torontonian --loop --gamma g.mtx [--modes ...]: sup_loop_torontonian of the
// same file and the complex 2M x 1 MatrixMarket file g.mtx (coordinate or
// array); prints "Loop torontonian: <value>".  --loop without --gamma, or
// --gamma without --torontonian --loop, is an error.
// --torontonian --table [--raw] [--loop --gamma g.mtx] [--modes ...]: the table
// of every sub-list's (loop) torontonian from one walk (sup_torontonian_table;
// --raw: the untransformed f(z)); prints 2^n lines "mask %.17e".
#include <getopt.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "../../include/superman.h"

namespace {

struct Cli {
  bool generic = true, dense = true, approximation = false, gpu = false, cpu = false, grid_graph = false;
  bool rccl = false, verbose = false, compression = false, exact = false, quad = false;
  bool half_calc = false, half_store = false, complex = false, complex_quad = false, complex_exact = false, preprocessing_given = false, gpu_num_given = false;
  bool hafnian = false, hafnian_quad = false, quad_long = false, loop = false, powertrace = false, torontonian = false, table = false, raw = false;
  int gpu_num = 2, threads = 16, perman_algo = 1, preprocessing = 0, device = 0, reps = 1;
  double scaling = -1.0;
  long number_of_times = 100000;  // main.cu:338-344 defaults
  int scale_intervals = 4, scale_times = 5, gridm = 36, gridn = 36;
  unsigned long long seed = 1;
  int jit = 0;
  std::string filename, checkpoint, rpt;
  std::string modes, gamma;
};

int fail(const char* what) {
  std::fprintf(stderr, "perman: %s: %s\n", what, sup_last_error());
  return 1;
}

void report(const std::string& name, double perm, double sec) {
  std::cout << "Result: " << name << " " << perm << " in " << sec << std::endl;
  std::printf("Permanent: %.17e\n", perm);
  std::fflush(stdout);
}

// main.cu:77-103, 156-183 (GPU) and 193-243 (CPU) approximation dispatch;
// main.cu:250-320 RunPermanForGridGraphs (sparse names, -i -m -n).
int run_approx(const Cli& c) {
  void* mat = nullptr;
  sup_dtype t = SUP_INT32;
  int n = 0, nnz = 0;
  if (c.grid_graph) {
    int* g = nullptr;
    if (sup_grid_graph(c.gridm, c.gridn, &g, &n) != SUP_OK) return fail("grid graph");
    mat = g;
  } else if (sup_read_matrix(c.filename.c_str(), c.generic ? 0 : 1, &mat, &t, &n, &nnz) != SUP_OK) {
    return fail("reading matrix");
  }
  const bool sparse = c.grid_graph || !c.dense;
  const int a = c.perman_algo;
  std::string name;
  int method = 0;
  bool multi = false;
  if (c.gpu) {
    static const char* dn[] = {"", "gpu_perman64_rasmussen", "gpu_perman64_approximation",
                               "gpu_perman64_rasmussen_multigpucpu_chunks",
                               "gpu_perman64_approximation_multigpucpu_chunks"};
    if (a < 1 || a > 4) {
      std::cout << "Unknown Algorithm ID" << std::endl;
      sup_free(mat);
      return 0;
    }
    name = std::string(dn[a]) + (sparse ? "_sparse" : "");
    method = (a == 2 || a == 4) ? 1 : 0;
    multi = a >= 3;
  } else {
    if (a != 1 && a != 2) {
      std::cout << "Unknown Algorithm ID" << std::endl;
      sup_free(mat);
      return 0;
    }
    name = std::string(a == 1 ? "rasmussen" : "approximation_perman64") + (sparse ? "_sparse" : "");
    method = a - 1;
  }
  sup_opts o;
  sup_opts_init(&o);
  o.gpu_num = multi ? c.gpu_num : 1;
  o.device_id = c.device;
  o.threads = c.threads;
  o.cpu_worker = (multi && c.cpu) ? 1 : 0;
  for (int r = 0; r < c.reps; ++r) {
    sup_approx_result res;
    auto t0 = std::chrono::steady_clock::now();
    const int rc = sup_approx(mat, t, n, method, (uint64_t)std::max(1L, c.number_of_times), c.scale_intervals,
                              c.scale_times, c.seed + (unsigned long long)r, &o, c.gpu ? 0 : 1, &res);
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (rc != SUP_OK) {
      sup_free(mat);
      return fail(name.c_str());
    }
    const char* tag = c.grid_graph ? "Try" : "Result";
    std::printf("Result: %s %2lf in %lf\n", name.c_str(), res.mean, sec);
    std::cout << tag << ": " << name << " " << res.mean << " in " << sec << std::endl;
    std::printf("Permanent: %.17e\nStdError: %.6e samples %llu zeros %.4f\n", res.mean, res.std_error,
                (unsigned long long)res.samples, res.zero_fraction);
    std::fflush(stdout);
  }
  sup_free(mat);
  return 0;
}

// --complex: the complex fp64 walk (sup_perman_complex) of a MatrixMarket
// `complex` file; same line shape as -q.  --complex-quad: the same file
// through sup_perman_complex_quad (the walk in double-double).  --complex-exact:
// through sup_perman_complex_exact (Gaussian integers, exact).
int run_complex(const Cli& c) {
  const char* flag = c.complex_exact ? "--complex-exact" : c.complex_quad ? "--complex-quad" : "--complex";
  const struct {
    bool on;
    const char* opt;
  } refused[] = {{!c.dense, "-s"},       {c.compression, "-o"},  {c.scaling > 0.0, "-u"},
                 {c.exact, "-E"},        {c.quad, "-q"},         {c.approximation, "-a"},
                 {!c.generic, "-b"},     {c.grid_graph, "-i"},   {c.preprocessing_given, "-r"},
                 {c.complex_exact && c.complex_quad, "--complex-quad"}};
  for (const auto& r : refused)
    if (r.on) {
      std::fprintf(stderr, "perman: %s does not combine with %s\n", flag, r.opt);
      return 1;
    }
  double* mat = nullptr;
  int n = 0, nnz = 0;
  if (sup_read_mtx_complex(c.filename.c_str(), &mat, &n, &nnz) != SUP_OK) return fail("reading complex matrix");
  sup_opts o;
  sup_opts_init(&o);
  o.gpu_num = (c.gpu && c.gpu_num_given) ? c.gpu_num : 1;  // one device unless -d asks for more
  o.device_id = c.device;
  o.threads = c.threads;
  double re = 0.0, im = 0.0;
  double q[4] = {0.0, 0.0, 0.0, 0.0};  // --complex-quad: re_hi, re_lo, im_hi, im_lo
  char xre[640] = "0", xim[640] = "0";   // --complex-exact: decimal integers
  sup_stats st;
  int rc = SUP_OK;
  const auto t0 = std::chrono::steady_clock::now();
  for (int rep = 0; rep < c.reps && rc == SUP_OK; ++rep)
    rc = c.complex_exact  ? sup_perman_complex_exact(mat, n, &o, c.gpu ? 0 : 1, xre, xim, sizeof(xre), &st)
         : c.complex_quad ? sup_perman_complex_quad(mat, n, &o, c.gpu ? 0 : 1, q, &st)
                          : sup_perman_complex(mat, n, &o, c.gpu ? 0 : 1, &re, &im, &st);
  const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() / (double)c.reps;
  sup_free(mat);
  if (rc != SUP_OK)
    return fail(c.complex_exact  ? "exact complex permanent"
                : c.complex_quad ? "complex double-double permanent"
                                 : "complex permanent");
  if (c.complex_exact) {
    std::cout << "Result: " << (c.gpu ? "gpu_perman64_complex_exact" : "cpu_perman64_complex_exact") << " "
              << std::strtod(xre, nullptr) << " " << std::strtod(xim, nullptr) << " in " << sec << std::endl;
    std::printf("Permanent (exact): %s %s\n", xre, xim);
  } else if (c.complex_quad) {
    std::cout << "Result: " << (c.gpu ? "gpu_perman64_complex_quad" : "cpu_perman64_complex_quad") << " " << q[0]
              << " " << q[2] << " in " << sec << std::endl;
    std::printf("Permanent (double-double): %.17e %.17e %.17e %.17e\n", q[0], q[1], q[2], q[3]);
  } else {
    std::cout << "Result: " << (c.gpu ? "gpu_perman64_complex" : "cpu_perman64_complex") << " " << re << " " << im
              << " in " << sec << std::endl;
    std::printf("Permanent: %.17e %.17e\n", re, im);
  }
  if (c.verbose)
    std::printf("Stats: devices %d kernel_ms %.3f wall_ms %.3f lanes %d walk %d grid %d\n", st.devices_used,
                st.kernel_ms, st.wall_ms, st.lane_bits, st.walk_bits, st.grid);
  return 0;
}

// --hafnian: sup_hafnian_complex / sup_loop_hafnian_complex of a symmetric
// MatrixMarket `complex` file; the line shape follows --complex.
int run_hafnian_cli(const Cli& c) {
  const struct {
    bool on;
    const char* opt;
  } refused[] = {{!c.dense, "-s"},       {c.compression, "-o"},    {c.scaling > 0.0, "-u"},
                 {c.quad, "-q"},         {c.approximation, "-a"},
                 {!c.generic, "-b"},     {c.grid_graph, "-i"},     {c.preprocessing_given, "-r"},
                 {c.complex, "--complex"}, {c.complex_quad, "--complex-quad"}, {c.complex_exact, "--complex-exact"}};
  for (const auto& r : refused)
    if (r.on) {
      std::fprintf(stderr, "perman: --hafnian does not combine with %s\n", r.opt);
      return 1;
    }
  if (c.exact && c.powertrace) {  // -E / --exact beside --hafnian: the exact Kan walk
    std::fprintf(stderr, "perman: --hafnian --exact does not combine with --powertrace\n");
    return 1;
  }
  if (c.hafnian_quad && c.powertrace) {
    std::fprintf(stderr, "perman: --hafnian --quad does not combine with --powertrace\n");
    return 1;
  }
  if (c.hafnian_quad && c.exact) {
    std::fprintf(stderr, "perman: --hafnian --quad does not combine with --exact\n");
    return 1;
  }
  double* mat = nullptr;
  int M = 0, nnz = 0;
  if (sup_read_mtx_complex(c.filename.c_str(), &mat, &M, &nnz) != SUP_OK) return fail("reading complex matrix");
  std::vector<int32_t> idx;
  if (c.rpt.empty()) {
    for (int k = 0; k < M; ++k) idx.push_back(k);
  } else {
    int k = 0;
    for (const char* p = c.rpt.c_str(); *p; ++k) {
      char* end = nullptr;
      const long r = std::strtol(p, &end, 10);
      if (end == p || r < 0 || (*end && *end != ',') || k >= M || idx.size() + (size_t)r > 64) {
        std::fprintf(stderr, "perman: --rpt takes at most %d non-negative counts with a sum in [1, 64]\n", M);
        sup_free(mat);
        return 1;
      }
      idx.insert(idx.end(), (size_t)r, k);
      p = *end ? end + 1 : end;
    }
  }
  if (idx.empty() || idx.size() > 64) {
    std::fprintf(stderr, "perman: --hafnian needs 1 to 64 indices (got %zu)\n", idx.size());
    sup_free(mat);
    return 1;
  }
  std::vector<double> mu((size_t)2 * M);
  for (int k = 0; k < M; ++k) mu[2 * k] = mat[2 * ((size_t)k * M + k)], mu[2 * k + 1] = mat[2 * ((size_t)k * M + k) + 1];
  sup_opts o;
  sup_opts_init(&o);
  o.gpu_num = 1;
  o.device_id = c.device;
  o.threads = c.threads;
  double out[2] = {0.0, 0.0};
  double q[4] = {0.0, 0.0, 0.0, 0.0};   // --quad: re_hi, re_lo, im_hi, im_lo
  char xre[768] = "0", xim[768] = "0";  // --exact: decimal integers
  sup_stats st;
  int rc = SUP_OK;
  const auto t0 = std::chrono::steady_clock::now();
  for (int rep = 0; rep < c.reps && rc == SUP_OK; ++rep)
    if (c.exact)
      rc = sup_hafnian_complex_exact(mat, M, c.loop ? mu.data() : nullptr, idx.data(), (int)idx.size(), 1, &o,
                                     c.gpu ? 0 : 1, xre, xim, sizeof(xre), &st);
    else if (c.hafnian_quad)
      rc = c.loop ? sup_loop_hafnian_complex_quad(mat, M, mu.data(), idx.data(), (int)idx.size(), 1, &o, c.gpu ? 0 : 1, q, &st)
                  : sup_hafnian_complex_quad(mat, M, idx.data(), (int)idx.size(), 1, &o, c.gpu ? 0 : 1, q, &st);
    else if (c.powertrace)
      rc = c.loop ? sup_loop_hafnian_complex_pt(mat, M, mu.data(), idx.data(), (int)idx.size(), 1, &o, c.gpu ? 0 : 1, out, &st)
                  : sup_hafnian_complex_pt(mat, M, idx.data(), (int)idx.size(), 1, &o, c.gpu ? 0 : 1, out, &st);
    else
      rc = c.loop ? sup_loop_hafnian_complex(mat, M, mu.data(), idx.data(), (int)idx.size(), 1, &o, c.gpu ? 0 : 1, out, &st)
                  : sup_hafnian_complex(mat, M, idx.data(), (int)idx.size(), 1, &o, c.gpu ? 0 : 1, out, &st);
  const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() / (double)c.reps;
  sup_free(mat);
  if (rc != SUP_OK)
    return fail(c.exact          ? (c.loop ? "exact loop hafnian" : "exact hafnian")
                : c.hafnian_quad ? (c.loop ? "double-double loop hafnian" : "double-double hafnian")
                : c.loop         ? "loop hafnian"
                                 : "hafnian");
  if (c.hafnian_quad) out[0] = q[0], out[1] = q[2];
  if (c.exact) out[0] = std::strtod(xre, nullptr), out[1] = std::strtod(xim, nullptr);
  std::cout << "Result: " << (c.gpu ? "gpu_" : "cpu_") << (c.loop ? "loop_hafnian64_complex" : "hafnian64_complex")
            << (c.powertrace ? "_powertrace" : "") << (c.exact ? "_exact" : "") << (c.hafnian_quad ? "_quad" : "") << " "
            << out[0] << " " << out[1] << " in " << sec << std::endl;
  if (c.exact) std::printf("Hafnian (exact): %s %s\n", xre, xim);
  else if (c.hafnian_quad) std::printf("Hafnian (double-double): %.17e %.17e %.17e %.17e\n", q[0], q[1], q[2], q[3]);
  else std::printf("Hafnian: %.17e %.17e\n", out[0], out[1]);
  if (c.verbose)
    std::printf("Stats: devices %d kernel_ms %.3f wall_ms %.3f terms %llu grid %d\n", st.devices_used, st.kernel_ms,
                st.wall_ms, (unsigned long long)st.visited_steps, st.grid);
  if (c.verbose && c.exact) std::printf("Exact: primes %d launches %d\n", (int)st.seg_cached_bits, (int)st.seg_pair_bits);
  return 0;
}

// --gamma: a complex N x 1 MatrixMarket file, coordinate ("i 1 re im" lines; the
// entries not named are zero) or array ("re im" lines), into N interleaved pairs.
bool read_gamma(const std::string& path, int N, std::vector<double>& g) {
  std::ifstream in(path);
  std::string line, tag, object, format, field;
  if (!in || !std::getline(in, line)) {
    std::fprintf(stderr, "perman: cannot read the --gamma file %s\n", path.c_str());
    return false;
  }
  std::istringstream ban(line);
  ban >> tag >> object >> format >> field;
  if (tag != "%%MatrixMarket" || object != "matrix" || (format != "coordinate" && format != "array") || field != "complex") {
    std::fprintf(stderr, "perman: --gamma takes a MatrixMarket 'matrix coordinate complex' or 'matrix array complex' file\n");
    return false;
  }
  while (in.peek() == '%') std::getline(in, line);
  long rows = 0, cols = 0, nz = 0;
  const bool coord = format == "coordinate";
  if (!(in >> rows >> cols) || (coord && !(in >> nz)) || rows != N || cols != 1 || nz < 0) {
    std::fprintf(stderr, "perman: --gamma needs a %d x 1 vector, the order of the matrix\n", N);
    return false;
  }
  g.assign((size_t)2 * N, 0.0);
  for (long e = 0; e < (coord ? nz : (long)N); ++e) {
    long i = e + 1, j = 1;
    double re, im;
    if ((coord && !(in >> i >> j)) || !(in >> re >> im) || i < 1 || i > N || j != 1) {
      std::fprintf(stderr, "perman: the --gamma file's entry %ld cannot be read or lies outside the %d x 1 vector\n", e + 1, N);
      return false;
    }
    g[2 * (size_t)(i - 1)] = re, g[2 * (size_t)(i - 1) + 1] = im;
  }
  return true;
}

// --torontonian --table [--raw]: sup_torontonian_table (--loop:
// sup_loop_torontonian_table) of the list; 2^n lines "mask value".  Frees mat.
int run_torontonian_table_cli(const Cli& c, double* mat, int M, const std::vector<int32_t>& modes,
                              const std::vector<double>& gamma, const sup_opts& o) {
  const int n = (int)modes.size();
  if (n > SUP_TORONTONIAN_TABLE_MAX_N) {
    std::fprintf(stderr, "perman: --table takes at most %d modes (got %d)\n", SUP_TORONTONIAN_TABLE_MAX_N, n);
    sup_free(mat);
    return 1;
  }
  std::vector<double> tab((size_t)1 << n);
  sup_stats st;
  int rc = SUP_OK;
  const auto t0 = std::chrono::steady_clock::now();
  for (int rep = 0; rep < c.reps && rc == SUP_OK; ++rep)
    rc = c.loop ? sup_loop_torontonian_table(mat, M, gamma.data(), modes.data(), n, c.raw ? 0 : 1, &o, c.gpu ? 0 : 1,
                                             tab.data(), &st)
                : sup_torontonian_table(mat, M, modes.data(), n, c.raw ? 0 : 1, &o, c.gpu ? 0 : 1, tab.data(), &st);
  const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() / (double)c.reps;
  sup_free(mat);
  if (rc != SUP_OK) return fail(c.loop ? "loop torontonian table" : "torontonian table");
  std::cout << "Result: " << (c.gpu ? "gpu_" : "cpu_") << (c.loop ? "loop_torontonian_table64 " : "torontonian_table64 ")
            << tab.size() << " entries in " << sec << std::endl;
  for (size_t mask = 0; mask < tab.size(); ++mask) std::printf("%zu %.17e\n", mask, tab[mask]);
  if (c.verbose)
    std::printf("Stats: devices %d kernel_ms %.3f wall_ms %.3f subsets %llu grid %d\n", st.devices_used, st.kernel_ms,
                st.wall_ms, (unsigned long long)st.visited_steps, st.grid);
  return 0;
}

// --torontonian: sup_torontonian of a Hermitian MatrixMarket `complex` file of
// even order (--loop --gamma: sup_loop_torontonian); the line shape follows --hafnian.
int run_torontonian_cli(const Cli& c) {
  const struct {
    bool on;
    const char* opt;
  } refused[] = {{!c.dense, "-s"},       {c.compression, "-o"},    {c.scaling > 0.0, "-u"},
                 {c.exact, "-E"},        {c.quad, "-q"},           {c.approximation, "-a"},
                 {!c.generic, "-b"},     {c.grid_graph, "-i"},     {c.preprocessing_given, "-r"},
                 {c.complex, "--complex"}, {c.complex_quad, "--complex-quad"}, {c.complex_exact, "--complex-exact"},
                 {c.hafnian, "--hafnian"}, {!c.rpt.empty(), "--rpt"}, {c.powertrace, "--powertrace"}};
  for (const auto& r : refused)
    if (r.on) {
      std::fprintf(stderr, "perman: --torontonian does not combine with %s\n", r.opt);
      return 1;
    }
  if (c.loop && c.gamma.empty()) {
    std::fprintf(stderr, "perman: --torontonian --loop needs --gamma <file> (a complex 2M x 1 MatrixMarket file)\n");
    return 1;
  }
  if (!c.loop && !c.gamma.empty()) {
    std::fprintf(stderr, "perman: --gamma goes with --torontonian --loop\n");
    return 1;
  }
  if (c.raw && !c.table) {
    std::fprintf(stderr, "perman: --raw goes with --torontonian --table\n");
    return 1;
  }
  double* mat = nullptr;
  int N = 0, nnz = 0;
  if (sup_read_mtx_complex(c.filename.c_str(), &mat, &N, &nnz) != SUP_OK) return fail("reading complex matrix");
  if (N < 2 || (N & 1)) {
    std::fprintf(stderr, "perman: --torontonian needs a matrix of even order 2M (got %d)\n", N);
    sup_free(mat);
    return 1;
  }
  const int M = N / 2;
  std::vector<int32_t> modes;
  if (c.modes.empty()) {
    for (int k = 0; k < M; ++k) modes.push_back(k);
  } else {
    for (const char* p = c.modes.c_str(); *p;) {
      char* end = nullptr;
      const long r = std::strtol(p, &end, 10);
      if (end == p || r < 0 || r >= M || (*end && *end != ',') || modes.size() >= 32) {
        std::fprintf(stderr, "perman: --modes takes at most 32 comma-separated modes in [0, %d)\n", M);
        sup_free(mat);
        return 1;
      }
      modes.push_back((int32_t)r);
      p = *end ? end + 1 : end;
    }
  }
  if (modes.empty() || modes.size() > 32) {
    std::fprintf(stderr, "perman: --torontonian needs 1 to 32 modes (got %zu)\n", modes.size());
    sup_free(mat);
    return 1;
  }
  std::vector<double> gamma;
  if (c.loop && !read_gamma(c.gamma, N, gamma)) {
    sup_free(mat);
    return 1;
  }
  sup_opts o;
  sup_opts_init(&o);
  o.gpu_num = 1;
  o.device_id = c.device;
  o.threads = c.threads;
  if (c.table) return run_torontonian_table_cli(c, mat, M, modes, gamma, o);
  double out = 0.0;
  sup_stats st;
  int rc = SUP_OK;
  const auto t0 = std::chrono::steady_clock::now();
  for (int rep = 0; rep < c.reps && rc == SUP_OK; ++rep)
    rc = c.loop ? sup_loop_torontonian(mat, M, gamma.data(), modes.data(), (int)modes.size(), 1, &o, c.gpu ? 0 : 1, &out, &st)
                : sup_torontonian(mat, M, modes.data(), (int)modes.size(), 1, &o, c.gpu ? 0 : 1, &out, &st);
  const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() / (double)c.reps;
  sup_free(mat);
  if (rc != SUP_OK) return fail(c.loop ? "loop torontonian" : "torontonian");
  std::cout << "Result: " << (c.gpu ? "gpu_" : "cpu_") << (c.loop ? "loop_torontonian64 " : "torontonian64 ") << out << " in "
            << sec << std::endl;
  std::printf(c.loop ? "Loop torontonian: %.17e\n" : "Torontonian: %.17e\n", out);
  if (c.verbose)
    std::printf("Stats: devices %d kernel_ms %.3f wall_ms %.3f subsets %llu grid %d\n", st.devices_used, st.kernel_ms,
                st.wall_ms, (unsigned long long)st.visited_steps, st.grid);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  Cli c;
  const char* const short_options = "bsr:t:f:gd:cap:x:y:z:im:n:l:k:Rvou:S:J:Eqhwe:";
  const struct option long_options[] = {{"binary", 0, NULL, 'b'},       {"sparse", 0, NULL, 's'},
                                        {"preprocessing", 1, NULL, 'r'}, {"threads", 1, NULL, 't'},
                                        {"file", 1, NULL, 'f'},          {"gpu", 0, NULL, 'g'},
                                        {"device", 1, NULL, 'd'},        {"cpu", 0, NULL, 'c'},
                                        {"approximation", 0, NULL, 'a'}, {"perman", 1, NULL, 'p'},
                                        {"numOfTimes", 1, NULL, 'x'},    {"scaleIntervals", 1, NULL, 'y'},
                                        {"scaleTimes", 1, NULL, 'z'},    {"grid", 0, NULL, 'i'},
                                        {"gridm", 1, NULL, 'm'},         {"gridn", 1, NULL, 'n'},
                                        {"gpu-id", 1, NULL, 'l'},        {"reps", 1, NULL, 'k'},
                                        {"rccl", 0, NULL, 'R'},          {"verbose", 0, NULL, 'v'},
                                        {"compression", 0, NULL, 'o'},   {"scaling", 1, NULL, 'u'},
                                        {"seed", 1, NULL, 'S'},          {"jit", 1, NULL, 'J'},
                                        {"exact", 0, NULL, 'E'},         {"quad", 0, NULL, 1012},
                                        {"halfCalc", 0, NULL, 'h'},      {"halfStore", 0, NULL, 'w'},
                                        {"gridMultip", 1, NULL, 'e'},    {"checkpoint", 1, NULL, 'C'},
                                        {"complex", 0, NULL, 1000},
                                        {"complex-quad", 0, NULL, 1001},
                                        {"complex-exact", 0, NULL, 1002},
                                        {"hafnian", 0, NULL, 1003},
                                        {"loop", 0, NULL, 1004},
                                        {"rpt", 1, NULL, 1005},
                                        {"powertrace", 0, NULL, 1006},
                                        {"torontonian", 0, NULL, 1007},
                                        {"modes", 1, NULL, 1008},
                                        {"gamma", 1, NULL, 1009},
                                        {"table", 0, NULL, 1010},
                                        {"raw", 0, NULL, 1011},
                                        {NULL, 0, NULL, 0}};
  int opt;
  auto need_arg = [&](char o) -> bool {
    if (optarg[0] == '-') {
      std::fprintf(stderr, "Option -%c requires an argument.\n", o);
      return false;
    }
    return true;
  };
  while ((opt = getopt_long(argc, argv, short_options, long_options, NULL)) != -1) {
    switch (opt) {
      case 'b': c.generic = false; break;
      case 's': c.dense = false; break;
      case 'r': if (!need_arg('t')) return 1; c.preprocessing = std::atoi(optarg); c.preprocessing_given = true; break;
      case 't': if (!need_arg('t')) return 1; c.threads = std::atoi(optarg); break;
      case 'f': if (!need_arg('f')) return 1; c.filename = optarg; break;
      case 'a': c.approximation = true; break;
      case 'g': c.gpu = true; break;
      case 'd': if (!need_arg('d')) return 1; c.gpu_num = std::atoi(optarg); c.gpu_num_given = true; break;
      case 'c': c.cpu = true; break;
      case 'p': if (!need_arg('p')) return 1; c.perman_algo = std::atoi(optarg); break;
      case 'x': if (!need_arg('x')) return 1; c.number_of_times = std::atol(optarg); break;
      case 'y': if (!need_arg('y')) return 1; c.scale_intervals = std::atoi(optarg); break;
      case 'z': if (!need_arg('z')) return 1; c.scale_times = std::atoi(optarg); break;
      case 'm': if (!need_arg('m')) return 1; c.gridm = std::atoi(optarg); break;
      case 'n': if (!need_arg('n')) return 1; c.gridn = std::atoi(optarg); break;
      case 'S': if (!need_arg('S')) return 1; c.seed = std::strtoull(optarg, nullptr, 10); break;
      case 'J': c.jit = std::atoi(optarg); break;  // may be negative: no need_arg
      case 'C': if (!need_arg('C')) return 1; c.checkpoint = optarg; break;  // -p6 / -p8: resumable
      case 'i': c.grid_graph = true; break;
      case 'l': if (!need_arg('l')) return 1; c.device = std::atoi(optarg); break;
      case 'k': if (!need_arg('k')) return 1; c.reps = std::max(1, std::atoi(optarg)); break;
      case 'R': c.rccl = true; break;
      case 'E': c.exact = true; break;
      case 'q': c.quad = true; break;
      case 1000: c.complex = true; break;
      case 1001: c.complex_quad = true; break;
      case 1002: c.complex_exact = true; break;
      case 1003: c.hafnian = true; break;
      case 1004: c.loop = true; break;
      case 1005: c.rpt = optarg; break;
      case 1006: c.powertrace = true; break;
      case 1007: c.torontonian = true; break;
      case 1008: c.modes = optarg; break;
      case 1009: c.gamma = optarg; break;
      case 1010: c.table = true; break;
      case 1011: c.raw = true; break;
      case 1012: c.quad_long = true; break;
      case 'v': c.verbose = true; break;
      // v2 flags (revised_perman/main.cpp:1431-1460): -w stores the matrix in
      // single precision (the permanent of the float-rounded entries); -h asks
      // for single-precision calculation, which this engine does not provide
      // (float X loses every digit at n >= 30): computed in fp64,
      // with a note; -e <multiplier> scales the reference's launch grid, which
      // the engine sizes from the occupancy itself: accepted, no effect.  (v2's
      // -v, quad storage, is this CLI's verbose flag: fp64 storage rounds an
      // entry by at most 2^-53 relative, below the walk's own rounding.)
      case 'h': c.half_calc = true; break;
      case 'w': c.half_store = true; break;
      case 'e': if (!need_arg('e')) return 1; break;
      case 'o': c.compression = true; break;  // revised_perman/main.cpp:1462
      case 'u':                                // main.cpp:1465 (atoi)
        if (!need_arg('u')) return 1;
        c.scaling = (double)std::atoi(optarg);
        break;
      case '?': return 1;
      default: std::abort();
    }
  }
  if (!c.grid_graph && c.filename.empty()) {
    std::fprintf(stderr, "Option -f is a required argument.\n");
    return 1;
  }
  for (int i = optind; i < argc; ++i) std::printf("Non-option argument %s\n", argv[i]);
  if (!c.cpu && !c.gpu) c.gpu = true;  // main.cu:482-484
  // --quad is -q, except beside --hafnian, where it asks for the double-double hafnian
  if (c.quad_long) (c.hafnian && !c.torontonian ? c.hafnian_quad : c.quad) = true;
  if (c.torontonian) return run_torontonian_cli(c);
  if (c.table || c.raw) {
    std::fprintf(stderr, "perman: --table and --raw go with --torontonian\n");
    return 1;
  }
  if (!c.modes.empty()) {
    std::fprintf(stderr, "perman: --modes goes with --torontonian\n");
    return 1;
  }
  if (!c.gamma.empty()) {
    std::fprintf(stderr, "perman: --gamma goes with --torontonian --loop\n");
    return 1;
  }
  if (c.hafnian) return run_hafnian_cli(c);
  if (c.powertrace) {
    std::fprintf(stderr, "perman: --powertrace goes with --hafnian\n");
    return 1;
  }
  if (c.loop || !c.rpt.empty()) {
    std::fprintf(stderr, "perman: --loop and --rpt go with --hafnian\n");
    return 1;
  }
  if (c.complex || c.complex_quad || c.complex_exact) return run_complex(c);
  if (c.grid_graph || c.approximation) return run_approx(c);

  void* mat = nullptr;
  sup_dtype t;
  int n = 0, nnz = 0;
  if (sup_read_matrix(c.filename.c_str(), c.generic ? 0 : 1, &mat, &t, &n, &nnz) != SUP_OK)
    return fail("reading matrix");
  if (c.half_store && t == SUP_FLOAT64) {  // v2 -w: single-precision storage
    double* d = (double*)mat;
    float* f = (float*)std::malloc(sizeof(float) * (size_t)n * n);
    if (!f) return fail("allocating the single-precision matrix");
    for (size_t i = 0; i < (size_t)n * n; ++i) f[i] = (float)d[i];
    sup_free(mat);
    mat = f;
    t = SUP_FLOAT32;
  }
  if (c.half_calc)
    std::fprintf(stderr, "perman: -h (single-precision calculation) is computed in fp64 by this engine\n");
  // main.cu:512-518 / 544-550 / 577-583: preprocessing rewrites mat (with
  // -o / -u it is applied to every leaf of the reductions instead).
  const bool reduce = c.compression || c.scaling > 0.0;
  sup_reduce_opts ro;
  sup_reduce_opts_init(&ro);
  ro.compress = c.compression ? 1 : 0;
  ro.scale_threshold = c.scaling > 0.0 ? c.scaling : 0.0;
  ro.preprocessing = c.preprocessing;
  std::vector<int> rp(n), cp(n);
  if (!reduce && c.preprocessing == 1) {
    if (sup_sort_order(mat, t, n, cp.data()) != SUP_OK) return fail("SortOrder");
  } else if (!reduce && c.preprocessing == 2) {
    if (sup_skip_order(mat, t, n, rp.data(), cp.data()) != SUP_OK) return fail("SkipOrder");
  }

  sup_opts o;
  sup_opts_init(&o);
  o.gpu_num = c.gpu_num;
  o.device_id = c.device;
  o.threads = c.threads;
  o.cpu_worker = (c.gpu && c.cpu) ? 1 : 0;
  // multi-device partials: RCCL whenever the devices are distinct GPUs (-1),
  // -R insists on it (an error when SUP_DEVICE_MAP shares a GPU)
  o.use_rccl = c.rccl ? 1 : -1;
  o.verbose = c.verbose ? 1 : 0;
  o.jit = c.jit;
  o.checkpoint = c.checkpoint.empty() ? nullptr : c.checkpoint.c_str();

  if (c.exact) {  // exact integer permanent (any -p: the sum does not depend on the kernel)
    if (c.scaling > 0.0) {
      std::fprintf(stderr, "perman: --exact does not combine with -u (scaling is not exact)\n");
      sup_free(mat);
      return 1;
    }
    if (c.gpu && c.perman_algo != 5 && c.perman_algo != 6 && c.perman_algo != 8) o.gpu_num = 1;
    if (c.perman_algo != 6 && c.perman_algo != 8) o.cpu_worker = 0;  // the hybrid worker joins the queues only
    static char buf[1 << 16];
    sup_stats st;
    int rc = SUP_OK;
    const auto t0 = std::chrono::steady_clock::now();
    for (int rep = 0; rep < c.reps && rc == SUP_OK; ++rep)
      rc = reduce ? sup_perman_reduced_exact(mat, t, n, &o, c.gpu ? 0 : 1, &ro, buf, sizeof buf, &st)
                  : sup_perman_exact(mat, t, n, &o, c.gpu ? 0 : 1, buf, sizeof buf, &st);
    const double sec =
        std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() / (double)c.reps;
    sup_free(mat);
    if (rc != SUP_OK) return fail("exact permanent");
    std::cout << "Result: " << (c.gpu ? "gpu_perman64_exact_residue" : "cpu_perman64_exact_residue") << " " << buf
              << " in " << sec << std::endl;
    std::printf("Permanent: %s\n", buf);
    if (c.verbose)
      std::printf("Stats: devices %d kernel_ms %.3f wall_ms %.3f cpu_items %d\n", st.devices_used, st.kernel_ms,
                  st.wall_ms, st.chunks_done_cpu);
    return 0;
  }

  if (c.quad) {  // double-double dense walk (any -p: the sum does not depend on the kernel)
    if (c.gpu && c.perman_algo != 5 && c.perman_algo != 6 && c.perman_algo != 8) o.gpu_num = 1;
    double hi = 0.0, lo = 0.0;
    sup_stats st;
    int rc = SUP_OK;
    const auto t0 = std::chrono::steady_clock::now();
    for (int rep = 0; rep < c.reps && rc == SUP_OK; ++rep)
      rc = reduce ? sup_perman_reduced_quad(mat, t, n, &o, c.gpu ? 0 : 1, &ro, &hi, &lo, &st)
                  : sup_perman_quad(mat, t, n, &o, c.gpu ? 0 : 1, &hi, &lo, &st);
    const double sec =
        std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() / (double)c.reps;
    sup_free(mat);
    if (rc != SUP_OK) return fail("double-double permanent");
    std::cout << "Result: " << (c.gpu ? "gpu_perman64_quad" : "cpu_perman64_quad") << " " << hi << " in " << sec
              << std::endl;
    std::printf("Permanent: %.17e\n", hi);
    std::printf("Permanent (double-double): %.17e %+.17e\n", hi, lo);
    if (c.verbose)
      std::printf("Stats: devices %d kernel_ms %.3f wall_ms %.3f\n", st.devices_used, st.kernel_ms, st.wall_ms);
    return 0;
  }

  std::string name;
  sup_kernel kern = SUP_KERNEL_DENSE;
  sup_sched sched = SUP_SCHED_SINGLE;
  bool on_gpu = c.gpu;
  const int a = c.perman_algo;
  if (on_gpu) {
    // main.cu:30-143 GPU exact dispatch
    if (c.dense) {
      static const char* names[] = {"gpu_perman64_xglobal", "gpu_perman64_xlocal", "gpu_perman64_xshared",
                                    "gpu_perman64_xshared_coalescing",
                                    "gpu_perman64_xshared_coalescing_mshared"};
      if (a >= 0 && a <= 4) {
        name = names[a];
      } else if (a == 5) {
        name = "gpu_perman64_xshared_coalescing_mshared_multigpu";
        sched = SUP_SCHED_STATIC;
      } else if (a == 6) {
        name = "gpu_perman64_xshared_coalescing_mshared_multigpucpu_chunks";
        sched = SUP_SCHED_CHUNKS;
      } else if (a == 66) {
        name = "gpu_perman64_xshared_coalescing_mshared_multigpu_manual_distribution";
        sched = SUP_SCHED_MANUAL;
        o.gpu_num = 4;  // main.cu:75 hard-codes 4 devices
      } else {
        std::cout << "Unknown Algorithm ID" << std::endl;
        sup_free(mat);
        return 0;
      }
    } else {
      static const char* names[] = {"", "gpu_perman64_xlocal_sparse", "gpu_perman64_xshared_sparse",
                                    "gpu_perman64_xshared_coalescing_sparse",
                                    "gpu_perman64_xshared_coalescing_mshared_sparse"};
      kern = SUP_KERNEL_SPARYSER;
      if (a >= 1 && a <= 4) {
        name = names[a];
      } else if (a == 5) {
        name = "gpu_perman64_xshared_coalescing_mshared_multigpu_sparse";
        sched = SUP_SCHED_STATIC;
      } else if (a == 6) {
        name = "gpu_perman64_xshared_coalescing_mshared_multigpucpu_chunks_sparse";
        sched = SUP_SCHED_CHUNKS;
      } else if (a == 7) {
        name = "gpu_perman64_xshared_coalescing_mshared_skipper";
        kern = SUP_KERNEL_SKIPPER;
      } else if (a == 8) {
        name = "gpu_perman64_xshared_coalescing_mshared_multigpucpu_chunks_skipper";
        kern = SUP_KERNEL_SKIPPER;
        sched = SUP_SCHED_CHUNKS;
      } else if (a == 66) {
        name = "gpu_perman64_xshared_coalescing_mshared_multigpu_sparse_manual_distribution";
        sched = SUP_SCHED_MANUAL;
        o.gpu_num = 4;
      } else {
        std::cout << "Unknown Algorithm ID" << std::endl;
        sup_free(mat);
        return 0;
      }
    }
    if (sched == SUP_SCHED_SINGLE) o.gpu_num = 1;
  } else {
    // main.cu:186-238 CPU exact dispatch (dense ignores -p, main.cu:188)
    if (c.dense) {
      name = "parallel_perman64";
    } else if (a == 1) {
      name = "parallel_perman64_sparse";
      kern = SUP_KERNEL_SPARYSER;
    } else if (a == 2 || a == 3) {
      name = a == 2 ? "parallel_skip_perman64_w" : "parallel_skip_perman64_w_balanced";
      kern = SUP_KERNEL_SKIPPER;
    } else {
      sup_free(mat);
      return 0;  // the reference prints nothing for other sparse CPU ids
    }
  }

  // HIP initialisation, the device contexts and the walk code objects on a
  // thread beside the planning sup_perman does first on the host (a cold
  // segmented plan is ~1 s of search and compiles): the walk then starts on a
  // warm runtime.  Its errors surface again in the call itself.
  std::thread warm;
  if (on_gpu) warm = std::thread([&o, n] { (void)sup_device_warmup(o.device_id, o.gpu_num, n); });
  struct Join {
    std::thread& t;
    ~Join() {
      if (t.joinable()) t.join();
    }
  } join_warm{warm};
  for (int r = 0; r < c.reps; ++r) {
    double perm = 0.0;
    sup_stats st;
    auto t0 = std::chrono::steady_clock::now();
    int rc = reduce   ? sup_perman_reduced(mat, t, n, kern, sched, &o, on_gpu ? 0 : 1, &ro, &perm, &st)
             : on_gpu ? sup_perman(mat, t, n, kern, sched, &o, &perm, &st)
                      : sup_perman_cpu(mat, t, n, kern, c.threads, &perm, &st);
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (rc != SUP_OK) {
      sup_free(mat);
      return fail(name.c_str());
    }
    report(name, perm, sec);
    if (c.verbose)
      std::printf("Stats: kernel_ms %.3f gray_steps %llu visited %llu devices %d lanes %d walk %d grid %d leaves %d "
                  "walk_kind %d ops_per_step %.1f jit_ms %.1f cpu_items %d device_checks %llu\n",
                  st.kernel_ms, (unsigned long long)st.gray_steps, (unsigned long long)st.visited_steps,
                  st.devices_used, st.lane_bits, st.walk_bits, st.grid, st.leaves, st.walk_kind, st.est_ops_per_step,
                  st.jit_ms, st.chunks_done_cpu, (unsigned long long)sup_device_checks());
  }
  sup_free(mat);
  return 0;
}
