// walk_tor.hip — the torontonian kernel for gfx950 (sup_torontonian and the
// range entry; torontonian.cpp).  tor.hpp states the sum and the
// order of every operation; torontonian.cpp's host twin runs the same chains.
//
// One wave (a block of 64 threads) takes a wave-chunk of consecutive z, 64 at
// a time.  A lane is a subset: lane l of a group has z = 64 g + l.  The low W =
// kTorW bits of z are the lane's tail; the 64 >> W settings h = z >> W of the
// bits above them that a group holds are taken one after the other, each by
// the whole wave:
//   advance(h)  the compact prefix factor of the positions h selects lives in
//               LDS (packed strictly lower rows, rho, the running product).
//               Only the rows at and below the highest position that changed
//               since the previous h are recomputed: one row at a time, a lane
//               per column, right-looking (lane c holds the chain of entry
//               (i, c); at step l lane l closes its entry, the others take its
//               term), which runs every chain in tor.hpp's order.
//   tail rows   T[t][c], the 2W tail rows against the new prefix columns, the
//               same way with a lane per (row, column); the chains' terms over
//               the kept columns need no exchange and come first.
//   S           the W (2W + 1) chains of the tail block, a lane each, paused
//               after the prefix columns and stored per setting.
// Then every lane reads its setting's S and running product and factors its
// own masked 2W x 2W tail in statically indexed registers: no cross-lane
// traffic until the butterfly of the signed f(z).
// G, the list's gathered matrix, stays in global memory (64 KiB at n = 32,
// each entry read once per recomputed row).
// Resource report: profiles/torontonian/walk_tor_resources.log.
#include "cx.hpp"
#include "tor.hpp"
#include "torontonian.hpp"
#include "tortab.hpp"
#include "walk_common.hpp"

namespace sup {

constexpr int kTorBlock = 64;
constexpr int kTorR = 2 * kTorW;              // tail rows
constexpr int kTorE = kTorW * (kTorR + 1);    // entries of the tail block, e = t (t + 1) / 2 + u
constexpr int kTorSub = 64 >> kTorW;          // settings of the high bits per group

__device__ __forceinline__ cx tor_ld(const double* p, uint32_t pair) { return cx{p[2 * pair], p[2 * pair + 1]}; }
__device__ __forceinline__ void tor_st(double* p, uint32_t pair, cx v) {
  p[2 * pair] = v.re;
  p[2 * pair + 1] = v.im;
}

// 64-lane pairwise sum (ascending xor offsets).
__device__ __forceinline__ double tor_wave_sum(double v) {
#pragma unroll
  for (int off = 1; off <= 32; off <<= 1) v = v + __shfl_xor(v, off, 64);
  return v;
}

// The block's LDS (torontonian.hpp tor_lds_bytes).
struct TorLds {
  double* Lp;    // prefix row i at pair i (i - 1) / 2
  double* T;     // tail row t at pair t PM
  double* S;     // setting q at pair q kTorE
  double* rho;   // PM
  double* prod;  // PM + 1, prod[0] = 1
  double* ps;    // kTorSub: the running product of setting q
  int* prow;     // full index of prefix row i
};

// Rows [r0, r0 + nr) x columns [c0, c1), nr (c1 - c0) <= 64, a lane per entry.
// TAIL: the rows are tail rows (full index PM + t, stored in T, no diagonal);
// otherwise nr = 1 and the row is prefix row r0 with its diagonal at c1 - 1.
// The columns below c0 of these rows are known.
template <bool TAIL>
__device__ __forceinline__ void tor_solve(const TorLds& m, const double* G, uint32_t N, uint32_t PM, uint32_t r0,
                                          uint32_t nr, uint32_t c0, uint32_t c1) {
  const uint32_t lane = threadIdx.x, ncol = c1 - c0;
  const uint32_t ri = lane / ncol, c = c0 + (lane - ri * ncol);
  const bool active = ri < nr;
  const uint32_t row = r0 + (active ? ri : 0u);
  const uint32_t Rr = TAIL ? PM + row : (uint32_t)m.prow[row];
  const uint32_t Rc = (uint32_t)m.prow[c];
  double* xrow = TAIL ? m.T + 2 * (size_t)row * PM : m.Lp + (size_t)row * (row - 1u);
  const double* lc = m.Lp + (size_t)c * (c - 1u);  // row c of the prefix factor
  cx acc = tor_ld(G, Rr * N + Rc);
#pragma unroll 4  // the loads do not wait for the chain
  for (uint32_t l = 0; l < c0; ++l) acc = tor_chain(acc, tor_ld(xrow, l), tor_ld(lc, l));
  for (uint32_t l = c0; l < c1; ++l) {
    if (active && c == l) {
      if (!TAIL && c == row) {
        const double r = tor_rho(acc.re);
        m.rho[l] = r;
        m.prod[l + 1] = m.prod[l] * r;
      } else {
        tor_st(xrow, l, tor_scale(acc, m.rho[l]));
      }
    }
    __syncthreads();
    if (active && c > l) acc = tor_chain(acc, tor_ld(xrow, l), tor_ld(lc, l));
  }
}

// The prefix of setting h after that of hp (have: there is one), then the tail
// block of h into slot q.
__device__ __forceinline__ void tor_advance(const TorLds& m, const double* G, uint32_t N, uint32_t PM, uint32_t H,
                                            uint32_t h, uint32_t hp, bool have, uint32_t q) {
  const uint32_t lane = threadIdx.x;
  uint32_t keep = 0;
  if (have) keep = h == hp ? 2u * (uint32_t)__builtin_popcount(h) : 2u * (uint32_t)__builtin_popcount((h >> (31 - __builtin_clz(h ^ hp))) >> 1);
  const uint32_t P = 2u * (uint32_t)__builtin_popcount(h);
  if (lane >= keep && lane < P) {  // the (lane / 2)-th highest set bit of h
    uint32_t hh = h;
    for (uint32_t j = 0; j < (lane >> 1); ++j) hh &= ~(1u << (31 - __builtin_clz(hh)));
    const uint32_t bit = 31u - (uint32_t)__builtin_clz(hh);
    m.prow[lane] = (int)(2u * (H - 1u - bit) + (lane & 1u));
  }
  __syncthreads();
  for (uint32_t i = keep; i < P; ++i) tor_solve<false>(m, G, N, PM, i, 1u, 0u, i + 1u);
  if (P > keep) {
    const uint32_t ncol = P - keep, per = 64u / ncol;
    for (uint32_t t0 = 0; t0 < (uint32_t)kTorR; t0 += per)
      tor_solve<true>(m, G, N, PM, t0, min(per, (uint32_t)kTorR - t0), keep, P);
  }
  if (lane < (uint32_t)kTorE) {
    uint32_t t = 0;
    while ((t + 1u) * (t + 2u) / 2u <= lane) ++t;
    const uint32_t u = lane - t * (t + 1u) / 2u;
    cx acc = tor_ld(G, (PM + t) * N + PM + u);
    const double* tt = m.T + 2 * (size_t)t * PM;
    const double* tu = m.T + 2 * (size_t)u * PM;
#pragma unroll 4
    for (uint32_t l = 0; l < P; ++l) acc = tor_chain(acc, tor_ld(tt, l), tor_ld(tu, l));
    tor_st(m.S, q * (uint32_t)kTorE + lane, acc);
  }
  if (lane == 0) m.ps[q] = m.prod[P];
  __syncthreads();
}

// A lane's masked tail: f(z) from its setting's paused chains and product.
__device__ __forceinline__ double tor_tail(const double* S, double f, uint32_t bits) {
  cx L[kTorR][kTorR];
  double rho[kTorR];
#pragma unroll
  for (int r = 0; r < kTorR; ++r) {
    const bool sr = (bits >> (kTorW - 1 - (r >> 1))) & 1u;
#pragma unroll
    for (int c = 0; c < r; ++c) {
      const bool sc = (bits >> (kTorW - 1 - (c >> 1))) & 1u;
      cx acc = tor_ld(S, (uint32_t)(r * (r + 1) / 2 + c));
#pragma unroll
      for (int l = 0; l < c; ++l) acc = tor_chain(acc, L[r][l], L[c][l]);
      const cx v = tor_scale(acc, rho[c]);
      L[r][c] = (sr && sc) ? v : cx{0.0, 0.0};
    }
    double d = S[2 * (r * (r + 1) / 2 + r)];
#pragma unroll
    for (int l = 0; l < r; ++l) d = tor_chain_diag(d, L[r][l]);
    rho[r] = sr ? tor_rho(d) : 1.0;
    f = f * rho[r];
  }
  return f;
}

// TABLE (tortab.hpp): the lane that holds z stores its unsigned f(z) to
// chunk_out[z], the 2^n table of the one list, and the sign, the butterfly, the
// chunk partial and the fold are left out.
template <bool TABLE>
__device__ __forceinline__ void walk_tor_body(const TorParams& p) {
  extern __shared__ double tor_lds[];
  const uint32_t lane = threadIdx.x;
  const uint32_t n = p.n, nn = p.nn, H = nn - (uint32_t)kTorW, PM = 2u * H, N = 2u * nn;
  TorLds m;
  m.Lp = tor_lds;
  m.T = m.Lp + (size_t)PM * (PM > 0u ? PM - 1u : 0u);
  m.S = m.T + 2 * (size_t)kTorR * PM;
  m.rho = m.S + 2 * (size_t)kTorSub * kTorE;
  m.prod = m.rho + PM;
  m.ps = m.prod + PM + 1u;
  m.prow = (int*)(m.ps + kTorSub);
  if (lane == 0) m.prod[0] = 1.0;
  __syncthreads();
  for (uint32_t g = next_chunk(p.counter); (uint64_t)g * p.group < p.chunk_count; g = next_chunk(p.counter)) {
    double keepv = 0.0;  // lane j keeps the partial of chunk g * group + j
    for (uint32_t j = 0; j < p.group; ++j) {
      const uint64_t a = (uint64_t)g * p.group + j;
      if (a >= p.chunk_count) break;
      const uint32_t list = (uint32_t)(a / p.cm), local = (uint32_t)(a - (uint64_t)list * p.cm);
      const double* G = p.G + (uint64_t)list * (2ull * N * N);
      const uint64_t c = p.chunk_first + local;
      uint64_t zlo = c << p.llog, zhi = (c + 1ull) << p.llog;
      if (zlo < p.z_begin) zlo = p.z_begin;
      if (zhi > p.z_end) zhi = p.z_end;
      double acc = 0.0;
      bool have = false;
      uint32_t hp = 0;
      for (uint64_t grp = zlo >> 6; (grp << 6) < zhi; ++grp) {
        for (uint32_t q = 0; q < (uint32_t)kTorSub; ++q) {
          const uint32_t h = (uint32_t)(((grp << 6) >> kTorW) + q);
          if (((uint64_t)h << kTorW) >= zhi) break;  // z < 2^n below: h stays below 2^H
          tor_advance(m, G, N, PM, H, h, hp, have, q);
          hp = h, have = true;
        }
        const uint64_t z = (grp << 6) + lane;
        double f = 0.0;
        if (z >= zlo && z < zhi) {
          const uint32_t q = lane >> kTorW;
          f = tor_tail(m.S + 2 * (size_t)q * kTorE, m.ps[q], lane & ((1u << kTorW) - 1u));
          if (TABLE) p.chunk_out[z] = f;
          else if ((n - (uint32_t)__builtin_popcountll(z)) & 1u) f = -f;
        }
        if (!TABLE) acc = acc + tor_wave_sum(f);
        __syncthreads();  // the next group's advance overwrites S
      }
      if (lane == j) keepv = acc;
    }
    const uint64_t a = (uint64_t)g * p.group + lane;
    if (!TABLE && lane < p.group && a < p.chunk_count) {
      p.chunk_out[2 * a] = keepv;
      p.chunk_out[2 * a + 1] = 0.0;
    }
  }
}

__global__ __launch_bounds__(kTorBlock) void walk_tor(TorParams p) { walk_tor_body<false>(p); }
__global__ __launch_bounds__(kTorBlock) void walk_tor_table(TorParams p) { walk_tor_body<true>(p); }

// tor_prepare: one block per list writes its gathered matrix (tor.hpp
// tor_entry, the host twin's own function) from O and the list.
__global__ __launch_bounds__(256) void tor_prepare(const double* __restrict__ O, int Mo, const int32_t* __restrict__ modes,
                                                   int n, double* __restrict__ G) {
  const uint32_t N = 2u * (uint32_t)tor_nn(n);
  double* g = G + (uint64_t)blockIdx.x * (2ull * N * N);
  const int32_t* s = modes + (uint64_t)blockIdx.x * (uint64_t)n;
  for (uint32_t e = threadIdx.x; e < N * N; e += 256u) {
    const cx v = tor_entry(O, Mo, s, n, (int)(e / N), (int)(e % N));
    g[2 * (uint64_t)e] = v.re;
    g[2 * (uint64_t)e + 1] = v.im;
  }
}

// tor_fold: one thread per list runs fock_fold over its cm chunk partials.
__global__ __launch_bounds__(256) void tor_fold(const double* __restrict__ parts, uint32_t cm, uint64_t K,
                                                double* __restrict__ out) {
  const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (k >= K) return;
  out[k] = fock_fold(parts + 2 * k * (uint64_t)cm, cm).re;
}

static bool tor_params_ok(const TorParams& p) {
  return p.n >= 1 && p.n <= (unsigned)SUP_TORONTONIAN_MAX_DEVICE_N && p.nn == (unsigned)tor_nn((int)p.n) &&
         tor_lds_bytes((int)p.n) <= 65536 && p.llog == (unsigned)tor_chunk_log((int)p.n) && p.llog >= 6 && p.cm >= 1 &&
         p.z_begin < p.z_end && p.z_end <= (1ull << p.n) && p.group >= 1 && p.group <= 64 && p.chunk_count >= 1 &&
         p.chunk_count <= 0x7fffffffull && p.chunk_count % p.cm == 0 && p.chunk_first == (p.z_begin >> p.llog) &&
         p.chunk_first + p.cm == ((p.z_end + (1ull << p.llog) - 1) >> p.llog) && p.G && p.chunk_out && p.counter;
}

hipError_t launch_tor(const TorParams& p, int grid, hipStream_t s) {
  if (!tor_params_ok(p) || grid < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(walk_tor, dim3(grid), dim3(kTorBlock), tor_lds_bytes((int)p.n), s, p);
  return hipGetLastError();
}

// p.chunk_out: the 2^n doubles of the one list's table.
hipError_t launch_tor_table(const TorParams& p, int grid, hipStream_t s) {
  if (!tor_params_ok(p) || grid < 1 || p.n > (unsigned)kTorTabMaxN || p.chunk_count != p.cm || p.z_begin != 0 ||
      p.z_end != (1ull << p.n))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(walk_tor_table, dim3(grid), dim3(kTorBlock), tor_lds_bytes((int)p.n), s, p);
  return hipGetLastError();
}

hipError_t tor_table_occupancy(int n, int* blocks_per_cu) {
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, walk_tor_table, kTorBlock, tor_lds_bytes(n));
}

hipError_t tor_occupancy(int n, int* blocks_per_cu) {
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, walk_tor, kTorBlock, tor_lds_bytes(n));
}

hipError_t launch_tor_prepare(const double* O, int M, const int32_t* modes, int n, uint64_t K, double* G, hipStream_t s) {
  if (M < 1 || n < 1 || n > kTorMaxN || K == 0 || K > 0x7fffffffull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(tor_prepare, dim3((unsigned)K), dim3(256), 0, s, O, M, modes, n, G);
  return hipGetLastError();
}

hipError_t launch_tor_fold(const double* parts, uint32_t cm, uint64_t K, double* out, hipStream_t s) {
  if (K == 0 || cm == 0) return hipErrorInvalidValue;
  const uint64_t blocks = (K + 255) / 256;
  if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(tor_fold, dim3((unsigned)blocks), dim3(256), 0, s, parts, cm, K, out);
  return hipGetLastError();
}

}  // namespace sup
