// walk_ltor.hip — the loop torontonian kernel for gfx950 (sup_loop_torontonian
// and the range entry; loop_torontonian.cpp).  tor.hpp and
// ltor.hpp state the sum and the order of every operation;
// loop_torontonian.cpp's host twin runs the same chains.
//
// The structure is walk_tor.hip's: one wave takes a wave-chunk of consecutive
// z, 64 at a time, a lane is a subset, the low W = kLtorW bits of z are the
// lane's tail, and the 64 >> W settings h of the bits above them are taken one
// after the other by the whole wave (advance: the compact prefix factor in
// LDS, only the rows below the highest changed position recomputed; the tail
// rows' prefix columns T; the paused chains S of the tail block).  The border
// (ltor.hpp) rides along as one more row:
//   T           has 2W + 1 rows: row 2W is the border's prefix columns w_l,
//               solved with the tail rows (a lane per (row, new column)) and
//               kept between settings like them;
//   S           has (2W + 1)(2W + 2) / 2 chains per setting: the tail block's
//               W (2W + 1), the border's 2W off-diagonal chains and its
//               diagonal chain d, paused after the prefix columns.  That is 66
//               at W = 5, two more than the wave has lanes: the pausing step
//               walks the entries in strides of 64;
//   tail        every lane continues the border over its own masked tail
//               columns in statically indexed registers next to its 2W x 2W
//               factor, closes d, and multiplies ltor_exp(-0.5 d) in last.
// G, the list's gathered matrix with the border as its last row, stays in
// global memory.  Resource report: profiles/loop_torontonian/walk_ltor_resources.log.
// walk_ltore (sup_loop_torontonian_each) walks the same chunks
// for lists of different orders in one queue, with ltore_prepare and
// ltore_fold beside it: profiles/threshold_chain/walk_ltore_resources.log.
#include "cx.hpp"
#include "loop_torontonian.hpp"
#include "ltor.hpp"
#include "tortab.hpp"
#include "walk_common.hpp"

namespace sup {

constexpr int kLtorBlock = 64;
constexpr int kLtorR = 2 * kLtorW;                          // tail rows; row kLtorR of T and S is the border
constexpr int kLtorE = (kLtorR + 1) * (kLtorR + 2) / 2;     // paused chains, e = t (t + 1) / 2 + u, u <= t <= kLtorR
constexpr int kLtorSub = 64 >> kLtorW;                      // settings of the high bits per group

__device__ __forceinline__ cx ltor_ld(const double* p, uint32_t pair) { return cx{p[2 * pair], p[2 * pair + 1]}; }
__device__ __forceinline__ void ltor_st(double* p, uint32_t pair, cx v) {
  p[2 * pair] = v.re;
  p[2 * pair + 1] = v.im;
}

// 64-lane pairwise sum (ascending xor offsets).
__device__ __forceinline__ double ltor_wave_sum(double v) {
#pragma unroll
  for (int off = 1; off <= 32; off <<= 1) v = v + __shfl_xor(v, off, 64);
  return v;
}

// The block's LDS (loop_torontonian.hpp ltor_lds_bytes).
struct LtorLds {
  double* Lp;    // prefix row i at pair i (i - 1) / 2
  double* T;     // tail row t (t = kLtorR: the border) at pair t PM
  double* S;     // setting q at pair q kLtorE
  double* rho;   // PM
  double* prod;  // PM + 1, prod[0] = 1
  double* ps;    // kLtorSub: the running product of setting q
  int* prow;     // full index of prefix row i
};

// Rows [r0, r0 + nr) x columns [c0, c1), nr (c1 - c0) <= 64, a lane per entry.
// TAIL: the rows are tail rows or the border (row PM + t of G, stored in T, no
// diagonal); otherwise nr = 1 and the row is prefix row r0 with its diagonal
// at c1 - 1.  The columns below c0 of these rows are known.
template <bool TAIL>
__device__ __forceinline__ void ltor_solve(const LtorLds& m, const double* G, uint32_t N, uint32_t PM, uint32_t r0,
                                           uint32_t nr, uint32_t c0, uint32_t c1) {
  const uint32_t lane = threadIdx.x, ncol = c1 - c0;
  const uint32_t ri = lane / ncol, c = c0 + (lane - ri * ncol);
  const bool active = ri < nr;
  const uint32_t row = r0 + (active ? ri : 0u);
  const uint32_t Rr = TAIL ? PM + row : (uint32_t)m.prow[row];
  const uint32_t Rc = (uint32_t)m.prow[c];
  double* xrow = TAIL ? m.T + 2 * (size_t)row * PM : m.Lp + (size_t)row * (row - 1u);
  const double* lc = m.Lp + (size_t)c * (c - 1u);  // row c of the prefix factor
  cx acc = ltor_ld(G, Rr * N + Rc);
#pragma unroll 4  // the loads do not wait for the chain
  for (uint32_t l = 0; l < c0; ++l) acc = tor_chain(acc, ltor_ld(xrow, l), ltor_ld(lc, l));
  for (uint32_t l = c0; l < c1; ++l) {
    if (active && c == l) {
      if (!TAIL && c == row) {
        const double r = tor_rho(acc.re);
        m.rho[l] = r;
        m.prod[l + 1] = m.prod[l] * r;
      } else {
        ltor_st(xrow, l, tor_scale(acc, m.rho[l]));
      }
    }
    __syncthreads();
    if (active && c > l) acc = tor_chain(acc, ltor_ld(xrow, l), ltor_ld(lc, l));
  }
}

// The prefix of setting h after that of hp (have: there is one), then the
// paused chains of h into slot q.
__device__ __forceinline__ void ltor_advance(const LtorLds& m, const double* G, uint32_t N, uint32_t PM, uint32_t H,
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
  for (uint32_t i = keep; i < P; ++i) ltor_solve<false>(m, G, N, PM, i, 1u, 0u, i + 1u);
  if (P > keep) {
    const uint32_t ncol = P - keep, per = 64u / ncol;
    for (uint32_t t0 = 0; t0 < (uint32_t)kLtorR + 1u; t0 += per)
      ltor_solve<true>(m, G, N, PM, t0, min(per, (uint32_t)kLtorR + 1u - t0), keep, P);
  }
  // kLtorE may pass 64: the entries beyond a wave go in a second round
  for (uint32_t e = lane; e < (uint32_t)kLtorE; e += 64u) {
    uint32_t t = 0;
    while ((t + 1u) * (t + 2u) / 2u <= e) ++t;
    const uint32_t u = e - t * (t + 1u) / 2u;
    // the border's own diagonal entry is +0: its chain is tor_chain_diag's
    cx acc = (t == (uint32_t)kLtorR && u == (uint32_t)kLtorR) ? cx{0.0, 0.0} : ltor_ld(G, (PM + t) * N + PM + u);
    const double* tt = m.T + 2 * (size_t)t * PM;
    const double* tu = m.T + 2 * (size_t)u * PM;
#pragma unroll 4
    for (uint32_t l = 0; l < P; ++l) acc = tor_chain(acc, ltor_ld(tt, l), ltor_ld(tu, l));
    ltor_st(m.S, q * (uint32_t)kLtorE + e, acc);
  }
  if (lane == 0) m.ps[q] = m.prod[P];
  __syncthreads();
}

// A lane's masked tail: f(z) from its setting's paused chains and product.
__device__ __forceinline__ double ltor_tail(const double* S, double f, uint32_t bits) {
  cx L[kLtorR][kLtorR];
  cx w[kLtorR];
  double rho[kLtorR];
  constexpr int kB = kLtorR * (kLtorR + 1) / 2;  // the border's chains
  double d = S[2 * (kB + kLtorR)];
#pragma unroll
  for (int r = 0; r < kLtorR; ++r) {
    const bool sr = (bits >> (kLtorW - 1 - (r >> 1))) & 1u;
#pragma unroll
    for (int c = 0; c < r; ++c) {
      const bool sc = (bits >> (kLtorW - 1 - (c >> 1))) & 1u;
      cx acc = ltor_ld(S, (uint32_t)(r * (r + 1) / 2 + c));
#pragma unroll
      for (int l = 0; l < c; ++l) acc = tor_chain(acc, L[r][l], L[c][l]);
      const cx v = tor_scale(acc, rho[c]);
      L[r][c] = (sr && sc) ? v : cx{0.0, 0.0};
    }
    double dr = S[2 * (r * (r + 1) / 2 + r)];
#pragma unroll
    for (int l = 0; l < r; ++l) dr = tor_chain_diag(dr, L[r][l]);
    rho[r] = sr ? tor_rho(dr) : 1.0;
    f = f * rho[r];
    // column r of the border
    cx acc = ltor_ld(S, (uint32_t)(kB + r));
#pragma unroll
    for (int l = 0; l < r; ++l) acc = tor_chain(acc, w[l], L[r][l]);
    const cx v = tor_scale(acc, rho[r]);
    w[r] = sr ? v : cx{0.0, 0.0};
    d = tor_chain_diag(d, w[r]);
  }
  return f * ltor_exp(-0.5 * d);
}

// The wave's LDS carved for PM prefix rows (loop_torontonian.hpp ltor_lds_bytes).
__device__ __forceinline__ LtorLds ltor_carve(double* lds, uint32_t PM) {
  LtorLds m;
  m.Lp = lds;
  m.T = m.Lp + (size_t)PM * (PM > 0u ? PM - 1u : 0u);
  m.S = m.T + 2 * (size_t)(kLtorR + 1) * PM;
  m.rho = m.S + 2 * (size_t)kLtorSub * kLtorE;
  m.prod = m.rho + PM;
  m.ps = m.prod + PM + 1u;
  m.prow = (int*)(m.ps + kLtorSub);
  return m;
}

// The partial of the z in [zlo, zhi) of one wave-chunk of a list of order n
// (zhi <= 2^n): its 64-aligned groups ascending from +0.
// TABLE (tortab.hpp): the lane that holds z stores its unsigned f(z) to
// table[z], the 2^n table of the one list, and the sign, the butterfly and the
// partial are left out.
template <bool TABLE>
__device__ __forceinline__ double ltor_walk_chunk(const LtorLds& m, const double* G, uint32_t n, uint32_t N, uint32_t PM,
                                                  uint32_t H, uint64_t zlo, uint64_t zhi, double* table) {
  const uint32_t lane = threadIdx.x;
  double acc = 0.0;
  bool have = false;
  uint32_t hp = 0;
  for (uint64_t grp = zlo >> 6; (grp << 6) < zhi; ++grp) {
    for (uint32_t q = 0; q < (uint32_t)kLtorSub; ++q) {
      const uint32_t h = (uint32_t)(((grp << 6) >> kLtorW) + q);
      if (((uint64_t)h << kLtorW) >= zhi) break;  // z < 2^n below: h stays below 2^H
      ltor_advance(m, G, N, PM, H, h, hp, have, q);
      hp = h, have = true;
    }
    const uint64_t z = (grp << 6) + lane;
    double f = 0.0;
    if (z >= zlo && z < zhi) {
      const uint32_t q = lane >> kLtorW;
      f = ltor_tail(m.S + 2 * (size_t)q * kLtorE, m.ps[q], lane & ((1u << kLtorW) - 1u));
      if (TABLE) table[z] = f;
      else if ((n - (uint32_t)__builtin_popcountll(z)) & 1u) f = -f;
    }
    if (!TABLE) acc = acc + ltor_wave_sum(f);
    __syncthreads();  // the next group's advance overwrites S
  }
  return acc;
}

// TABLE: the fold is left out too; p.chunk_out is the table.
template <bool TABLE>
__device__ __forceinline__ void walk_ltor_body(const TorParams& p) {
  extern __shared__ double ltor_lds[];
  const uint32_t lane = threadIdx.x;
  const uint32_t n = p.n, nn = p.nn, H = nn - (uint32_t)kLtorW, PM = 2u * H, N = 2u * nn;
  const LtorLds m = ltor_carve(ltor_lds, PM);
  if (lane == 0) m.prod[0] = 1.0;
  __syncthreads();
  for (uint32_t g = next_chunk(p.counter); (uint64_t)g * p.group < p.chunk_count; g = next_chunk(p.counter)) {
    double keepv = 0.0;  // lane j keeps the partial of chunk g * group + j
    for (uint32_t j = 0; j < p.group; ++j) {
      const uint64_t a = (uint64_t)g * p.group + j;
      if (a >= p.chunk_count) break;
      const uint32_t list = (uint32_t)(a / p.cm), local = (uint32_t)(a - (uint64_t)list * p.cm);
      const double* G = p.G + (uint64_t)list * (2ull * N * (N + 1ull));
      const uint64_t c = p.chunk_first + local;
      uint64_t zlo = c << p.llog, zhi = (c + 1ull) << p.llog;
      if (zlo < p.z_begin) zlo = p.z_begin;
      if (zhi > p.z_end) zhi = p.z_end;
      const double acc = ltor_walk_chunk<TABLE>(m, G, n, N, PM, H, zlo, zhi, p.chunk_out);
      if (lane == j) keepv = acc;
    }
    const uint64_t a = (uint64_t)g * p.group + lane;
    if (!TABLE && lane < p.group && a < p.chunk_count) {
      p.chunk_out[2 * a] = keepv;
      p.chunk_out[2 * a + 1] = 0.0;
    }
  }
}

__global__ __launch_bounds__(kLtorBlock) void walk_ltor(TorParams p) { walk_ltor_body<false>(p); }
__global__ __launch_bounds__(kLtorBlock) void walk_ltor_table(TorParams p) { walk_ltor_body<true>(p); }

// A descriptor field is the same in every lane: say so, and it lives in a scalar register.
__device__ __forceinline__ uint32_t ltor_uniform(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }

// walk_ltore: the ragged batch (sup_loop_torontonian_each).  The
// queue holds the wave-chunks of every item of the slab one after the other
// (item i: slots [chunk0, chunk0 + cm)); a ticket finds the item of its first
// slot by bisection over chunk0 and steps on from there.  The order, the
// padded order, the chunk size and the place of the item's G come from its
// descriptor, all wave-uniform; the LDS is carved again for every chunk from
// the item's own PM, and the chunk is walk_ltor's.
__global__ __launch_bounds__(kLtorBlock) void walk_ltore(LtorEachParams p) {
  extern __shared__ double ltor_lds[];
  const uint32_t lane = threadIdx.x;
  for (uint32_t g = next_chunk(p.counter); (uint64_t)g * p.group < p.chunk_count; g = next_chunk(p.counter)) {
    const uint32_t a0 = g * p.group;  // the queue has fewer than 2^31 slots
    uint32_t it = 0, end = p.item_count;  // the last item with chunk0 <= a0
    while (end - it > 1u) {
      const uint32_t mid = (it + end) >> 1;
      if (p.items[mid].chunk0 <= a0) it = mid;
      else end = mid;
    }
    double keepv = 0.0;  // lane j keeps the partial of slot a0 + j
    for (uint32_t j = 0; j < p.group; ++j) {
      const uint32_t a = a0 + j;
      if (a >= (uint32_t)p.chunk_count) break;
      while (it + 1u < p.item_count && a >= p.items[it + 1u].chunk0) ++it;
      const LtorItem* d = p.items + it;
      const uint32_t n = ltor_uniform(d->n), nn = ltor_uniform(d->nn), llog = ltor_uniform(d->llog);
      const uint32_t c = ltor_uniform(a - d->chunk0);
      const double* G = p.G + (((uint64_t)ltor_uniform((uint32_t)(d->g_off >> 32)) << 32) | ltor_uniform((uint32_t)d->g_off));
      const uint32_t H = nn - (uint32_t)kLtorW, PM = 2u * H, N = 2u * nn;
      const LtorLds m = ltor_carve(ltor_lds, PM);
      if (lane == 0) m.prod[0] = 1.0;
      __syncthreads();
      uint64_t zlo = (uint64_t)c << llog, zhi = ((uint64_t)c + 1ull) << llog;
      if (zhi > (1ull << n)) zhi = 1ull << n;
      const double acc = ltor_walk_chunk<false>(m, G, n, N, PM, H, zlo, zhi, nullptr);
      if (lane == j) keepv = acc;
    }
    const uint32_t a = a0 + lane;
    if (lane < p.group && a < (uint32_t)p.chunk_count) {
      p.chunk_out[2 * (uint64_t)a] = keepv;
      p.chunk_out[2 * (uint64_t)a + 1] = 0.0;
    }
  }
}

// ltor_prepare: one block per list writes its gathered matrix (tor.hpp
// tor_entry) and border row (ltor.hpp ltor_border), the host twin's own
// functions, from O, gamma and the list.
__global__ __launch_bounds__(256) void ltor_prepare(const double* __restrict__ O, int Mo, const double* __restrict__ gamma,
                                                    const int32_t* __restrict__ modes, int n, double* __restrict__ G) {
  const uint32_t N = 2u * (uint32_t)tor_nn(n);
  double* g = G + (uint64_t)blockIdx.x * (2ull * N * (N + 1ull));
  const int32_t* s = modes + (uint64_t)blockIdx.x * (uint64_t)n;
  for (uint32_t e = threadIdx.x; e < N * (N + 1u); e += 256u) {
    const uint32_t R = e / N, C = e % N;
    const cx v = R < N ? tor_entry(O, Mo, s, n, (int)R, (int)C) : ltor_border(gamma, Mo, s, n, (int)C);
    g[2 * (uint64_t)e] = v.re;
    g[2 * (uint64_t)e + 1] = v.im;
  }
}

// ltore_prepare: ltor_prepare with the item's own list (its first n entries),
// order, gamma row and place in G.
__global__ __launch_bounds__(256) void ltore_prepare(const double* __restrict__ O, int Mo, const double* __restrict__ gammas,
                                                     const int32_t* __restrict__ modes, int stride,
                                                     const LtorItem* __restrict__ items, double* __restrict__ G) {
  const LtorItem d = items[blockIdx.x];
  const int n = (int)d.n;
  const uint32_t N = 2u * d.nn;
  double* g = G + d.g_off;
  const int32_t* s = modes + (uint64_t)blockIdx.x * (uint64_t)stride;
  const double* gamma = gammas + 4ull * (uint64_t)Mo * (uint64_t)d.row;
  for (uint32_t e = threadIdx.x; e < N * (N + 1u); e += 256u) {
    const uint32_t R = e / N, C = e % N;
    const cx v = R < N ? tor_entry(O, Mo, s, n, (int)R, (int)C) : ltor_border(gamma, Mo, s, n, (int)C);
    g[2 * (uint64_t)e] = v.re;
    g[2 * (uint64_t)e + 1] = v.im;
  }
}

// ltore_fold: tor_fold over each item's own slots.
__global__ __launch_bounds__(256) void ltore_fold(const double* __restrict__ parts, const LtorItem* __restrict__ items,
                                                  uint64_t K, double* __restrict__ out) {
  const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (k >= K) return;
  out[k] = fock_fold(parts + 2 * (uint64_t)items[k].chunk0, items[k].cm).re;
}

// ltor_exp_each: out[i] = ltor_exp(x[i]) (sup_ltor_exp_device, the tests' helper).
__global__ __launch_bounds__(256) void ltor_exp_each(const double* __restrict__ x, uint64_t count, double* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i < count) out[i] = ltor_exp(x[i]);
}

static bool ltor_params_ok(const TorParams& p) {
  return p.n >= 1 && p.n <= (unsigned)SUP_LOOP_TORONTONIAN_MAX_DEVICE_N && p.nn == (unsigned)tor_nn((int)p.n) &&
         p.nn >= (unsigned)kLtorW && ltor_lds_bytes((int)p.n) <= 65536 && p.llog == (unsigned)tor_chunk_log((int)p.n) &&
         p.llog >= 6 && p.cm >= 1 && p.z_begin < p.z_end && p.z_end <= (1ull << p.n) && p.group >= 1 && p.group <= 64 &&
         p.chunk_count >= 1 && p.chunk_count <= 0x7fffffffull && p.chunk_count % p.cm == 0 &&
         p.chunk_first == (p.z_begin >> p.llog) &&
         p.chunk_first + p.cm == ((p.z_end + (1ull << p.llog) - 1) >> p.llog) && p.G && p.chunk_out && p.counter;
}

hipError_t launch_ltor(const TorParams& p, int grid, hipStream_t s) {
  if (!ltor_params_ok(p) || grid < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(walk_ltor, dim3(grid), dim3(kLtorBlock), ltor_lds_bytes((int)p.n), s, p);
  return hipGetLastError();
}

// p.chunk_out: the 2^n doubles of the one list's table.
hipError_t launch_ltor_table(const TorParams& p, int grid, hipStream_t s) {
  if (!ltor_params_ok(p) || grid < 1 || p.n > (unsigned)kTorTabMaxN || p.chunk_count != p.cm || p.z_begin != 0 ||
      p.z_end != (1ull << p.n))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(walk_ltor_table, dim3(grid), dim3(kLtorBlock), ltor_lds_bytes((int)p.n), s, p);
  return hipGetLastError();
}

hipError_t ltor_table_occupancy(int n, int* blocks_per_cu) {
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, walk_ltor_table, kLtorBlock, ltor_lds_bytes(n));
}

hipError_t ltor_occupancy(int n, int* blocks_per_cu) {
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, walk_ltor, kLtorBlock, ltor_lds_bytes(n));
}

hipError_t launch_ltor_prepare(const double* O, int M, const double* gamma, const int32_t* modes, int n, uint64_t K,
                               double* G, hipStream_t s) {
  if (M < 1 || n < 1 || n > kTorMaxN || K == 0 || K > 0x7fffffffull || !O || !gamma || !modes || !G) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ltor_prepare, dim3((unsigned)K), dim3(256), 0, s, O, M, gamma, modes, n, G);
  return hipGetLastError();
}

// The host has checked every descriptor (loop_torontonian.cpp ltor_each_slab);
// max_n: the slab's largest order, whose LDS the launch asks for.
hipError_t launch_ltore(const LtorEachParams& p, int max_n, int grid, hipStream_t s) {
  if (grid < 1 || max_n < 1 || max_n > SUP_LOOP_TORONTONIAN_MAX_DEVICE_N || ltor_lds_bytes(max_n) > 65536 || !p.G || !p.items ||
      p.item_count < 1 || p.chunk_count < p.item_count || p.chunk_count > 0x7fffffffull || p.group < 1 || p.group > 64 ||
      !p.chunk_out || !p.counter)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(walk_ltore, dim3(grid), dim3(kLtorBlock), ltor_lds_bytes(max_n), s, p);
  return hipGetLastError();
}

hipError_t ltore_occupancy(int max_n, int* blocks_per_cu) {
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, walk_ltore, kLtorBlock, ltor_lds_bytes(max_n));
}

hipError_t launch_ltore_prepare(const double* O, int M, const double* gammas, const int32_t* modes, int stride,
                                const LtorItem* items, uint64_t K, double* G, hipStream_t s) {
  if (M < 1 || stride < 1 || K == 0 || K > 0x7fffffffull || !O || !gammas || !modes || !items || !G) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ltore_prepare, dim3((unsigned)K), dim3(256), 0, s, O, M, gammas, modes, stride, items, G);
  return hipGetLastError();
}

hipError_t launch_ltore_fold(const double* parts, const LtorItem* items, uint64_t K, double* out, hipStream_t s) {
  const uint64_t blocks = (K + 255) / 256;
  if (K == 0 || blocks > 0x7fffffffull || !parts || !items || !out) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ltore_fold, dim3((unsigned)blocks), dim3(256), 0, s, parts, items, K, out);
  return hipGetLastError();
}

hipError_t launch_ltor_exp(const double* x, uint64_t count, double* out, hipStream_t s) {
  if (!x || !out || count == 0) return hipErrorInvalidValue;
  const uint64_t blocks = (count + 255) / 256;
  if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ltor_exp_each, dim3((unsigned)blocks), dim3(256), 0, s, x, count, out);
  return hipGetLastError();
}

}  // namespace sup
