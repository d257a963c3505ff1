// kernels.hpp — host-visible launch entry points of the gfx950 walk kernels.
#pragma once
#include <hip/hip_runtime.h>

#include "cplx_fock.hpp"
#include "haf.hpp"
#include "cxexact.hpp"
#include "walk_batch.hpp"
#include "walk_params.hpp"

namespace sup {

// SkipPer (walk_skip.hip, its host twin engine_cpu.cpp; oracle/oracle.c
// restates it): zero checks and jumps at the starts of aligned segments of
// 2^kSkipSegBits Gray steps.
#ifndef SUP_SKIP_SEG_BITS
#define SUP_SKIP_SEG_BITS 4  // (other values: experiments; oracle/oracle.c must agree)
#endif
constexpr int kSkipSegBits = SUP_SKIP_SEG_BITS;
constexpr uint32_t kSkipSegMask = (1u << kSkipSegBits) - 1u;

// Per-N-range launchers (one translation unit per range, see Makefile).
#define SUP_DECL_RANGE(KIND, LO)                                                      \
  hipError_t launch_##KIND##_##LO(int n, const WalkParams& p, int grid, hipStream_t s); \
  hipError_t occupancy_##KIND##_##LO(int n, int* blocks_per_cu);
SUP_DECL_RANGE(dense, 1)
SUP_DECL_RANGE(dense, 17)
SUP_DECL_RANGE(dense, 33)
SUP_DECL_RANGE(dense, 49)
SUP_DECL_RANGE(sparse, 1)
SUP_DECL_RANGE(sparse, 17)
SUP_DECL_RANGE(sparse, 33)
SUP_DECL_RANGE(sparse, 49)
SUP_DECL_RANGE(skip, 1)
SUP_DECL_RANGE(skip, 17)
SUP_DECL_RANGE(skip, 33)
SUP_DECL_RANGE(skip, 49)
#undef SUP_DECL_RANGE
#define SUP_DECL_BATCH(KIND, LO)                                                                       \
  hipError_t launch_batch_##KIND##_##LO(int n, const WalkParams& p, const LeafBatch& b, int grid, hipStream_t s); \
  hipError_t occupancy_batch_##KIND##_##LO(int n, int* blocks_per_cu);
SUP_DECL_BATCH(dense, 1)
SUP_DECL_BATCH(dense, 17)
SUP_DECL_BATCH(dense, 33)
SUP_DECL_BATCH(dense, 49)
SUP_DECL_BATCH(sparse, 1)
SUP_DECL_BATCH(sparse, 17)
SUP_DECL_BATCH(sparse, 33)
SUP_DECL_BATCH(sparse, 49)
#undef SUP_DECL_BATCH
#define SUP_DECL_EXACT(LO)                                                                                  \
  hipError_t launch_exact_##LO(int n, int g, const WalkParams& p, const ExactParams& e, int grid,        \
                               hipStream_t s);                                                        \
  hipError_t occupancy_exact_##LO(int n, int g, int* blocks_per_cu);
SUP_DECL_EXACT(1)
SUP_DECL_EXACT(17)
SUP_DECL_EXACT(33)
SUP_DECL_EXACT(49)
#undef SUP_DECL_EXACT
#define SUP_DECL_DD(LO)                                                               \
  hipError_t launch_dd_##LO(int n, const WalkParams& p, int grid, hipStream_t s);    \
  hipError_t occupancy_dd_##LO(int n, int* blocks_per_cu);
SUP_DECL_DD(1)
SUP_DECL_DD(17)
SUP_DECL_DD(33)
SUP_DECL_DD(49)
#undef SUP_DECL_DD
#define SUP_DECL_DDB(LO)                                                                  \
  hipError_t launch_ddblocked_##LO(int n, const WalkParams& p, int grid, hipStream_t s);  \
  hipError_t occupancy_ddblocked_##LO(int n, int* blocks_per_cu);
SUP_DECL_DDB(1)
SUP_DECL_DDB(17)
SUP_DECL_DDB(33)
SUP_DECL_DDB(49)
#undef SUP_DECL_DDB
#define SUP_DECL_CPLX(LO)                                                              \
  hipError_t launch_cplx_##LO(int n, const WalkParams& p, int grid, hipStream_t s);   \
  hipError_t occupancy_cplx_##LO(int n, int* blocks_per_cu);
SUP_DECL_CPLX(1)
SUP_DECL_CPLX(17)
SUP_DECL_CPLX(33)
SUP_DECL_CPLX(49)
#undef SUP_DECL_CPLX
// walk_cplxdd.hip is instantiated up to SUP_CPLX_QUAD_MAX_DEVICE_N = 40 only: its third range is 33..40
#define SUP_DECL_CPLXDD(LO)                                                              \
  hipError_t launch_cplxdd_##LO(int n, const WalkParams& p, int grid, hipStream_t s);   \
  hipError_t occupancy_cplxdd_##LO(int n, int* blocks_per_cu);
SUP_DECL_CPLXDD(1)
SUP_DECL_CPLXDD(17)
SUP_DECL_CPLXDD(33)
#undef SUP_DECL_CPLXDD
// walk_cplxexact.hip: N = 1..SUP_CPLX_EXACT_MAX_DEVICE_N, g = 1 or 2
#define SUP_DECL_CPLXEXACT(LO)                                                                                \
  hipError_t launch_cplxexact_##LO(int n, int g, const WalkParams& p, const CxExactParams& e, int grid,   \
                                   hipStream_t s);                                                        \
  hipError_t occupancy_cplxexact_##LO(int n, int g, int* blocks_per_cu);
SUP_DECL_CPLXEXACT(1)
SUP_DECL_CPLXEXACT(17)
SUP_DECL_CPLXEXACT(33)
SUP_DECL_CPLXEXACT(49)
#undef SUP_DECL_CPLXEXACT
#define SUP_DECL_CPLXB(LO)                                                                       \
  hipError_t launch_cplxb_##LO(int n, const WalkParams& p, int hbits, int grid, hipStream_t s); \
  hipError_t occupancy_cplxb_##LO(int n, int* blocks_per_cu);
SUP_DECL_CPLXB(1)
SUP_DECL_CPLXB(17)
#undef SUP_DECL_CPLXB
#define SUP_DECL_CPLXM(LO)                                                                                       \
  hipError_t launch_cplxm_##LO(int n, const WalkParams& p, int hbits, unsigned long long ostride, int grid, \
                               hipStream_t s);                                                               \
  hipError_t occupancy_cplxm_##LO(int n, int* blocks_per_cu);
SUP_DECL_CPLXM(1)
SUP_DECL_CPLXM(17)
#undef SUP_DECL_CPLXM
#define SUP_DECL_CPLXF(LO)                                                             \
  hipError_t launch_cplxf_##LO(int n, const FockParams& p, int grid, hipStream_t s);   \
  hipError_t occupancy_cplxf_##LO(int n, int* blocks_per_cu);
SUP_DECL_CPLXF(1)
SUP_DECL_CPLXF(17)
SUP_DECL_CPLXF(33)
SUP_DECL_CPLXF(49)
#undef SUP_DECL_CPLXF
#define SUP_DECL_CPLXFM(LO)                                                             \
  hipError_t launch_cplxfm_##LO(int n, const FockParams& p, int grid, hipStream_t s);   \
  hipError_t occupancy_cplxfm_##LO(int n, int* blocks_per_cu);
SUP_DECL_CPLXFM(1)
SUP_DECL_CPLXFM(17)
#undef SUP_DECL_CPLXFM
#define SUP_DECL_LDS(LO)                                                                  \
  hipError_t launch_lds_##LO(int n, const WalkParams& p, int grid, hipStream_t s);        \
  hipError_t occupancy_lds_##LO(int n, int m, int* blocks_per_cu);
SUP_DECL_LDS(1)
SUP_DECL_LDS(17)
SUP_DECL_LDS(33)
SUP_DECL_LDS(49)
#undef SUP_DECL_LDS

// kWalkSeg: the pattern-specialised segmented walk (jit.cpp), compiled at run
// time with hiprtc for one matrix pattern; launched through hipModule APIs.
enum WalkKind { kWalkDense = 0, kWalkSparse = 1, kWalkSkip = 2, kWalkSeg = 3 };

// Launch the walk kernel of `kind` for matrix order n (1..64).
hipError_t launch_walk(WalkKind kind, int n, const WalkParams& p, int grid, hipStream_t s);
// Resident 256-thread blocks per CU for that kernel (occupancy API).
hipError_t walk_occupancy(WalkKind kind, int n, int* blocks_per_cu);

// A batch of leaves of one order and layout in one launch (walk_batch.hpp;
// kWalkDense / kWalkSparse), and its occupancy.
hipError_t launch_walk_batch(WalkKind kind, int n, const WalkParams& p, const LeafBatch& b, int grid, hipStream_t s);
hipError_t walk_batch_occupancy(WalkKind kind, int n, int* blocks_per_cu);

// LDS-staged dense walk (walk_lds.hip; 64-thread blocks, X in LDS).
hipError_t launch_lds(int n, const WalkParams& p, int grid, hipStream_t s);
hipError_t lds_occupancy(int n, int m, int* blocks_per_cu);

// Exact residue walk (walk_exact.hip) for matrix order n (1..64), rows
// multiplied in exact groups of g (1, 2 or 4) before the residue chain.
hipError_t launch_exact(int n, int g, const WalkParams& p, const ExactParams& e, int grid, hipStream_t s);
hipError_t exact_occupancy(int n, int g, int* blocks_per_cu);

// Double-double dense walk (walk_dd.hip): p.x0 = 2 NP doubles (hi, lo),
// p.chunk_out = 2 doubles (hi, lo) per wave-chunk.
hipError_t launch_dd(int n, const WalkParams& p, int grid, hipStream_t s);
hipError_t dd_occupancy(int n, int* blocks_per_cu);
// Its prefix-blocked form (walk_dd_blocked, a kWalkSparse plan: p.nb_lo / nb_hi).
hipError_t launch_dd_blocked(int n, const WalkParams& p, int grid, hipStream_t s);
hipError_t dd_blocked_occupancy(int n, int* blocks_per_cu);

// Complex fp64 dense walk (walk_cplx.hip): p.cols = the Re plane, then the Im
// plane of the signed column table; p.x0 = 2 NP doubles (re, im);
// p.chunk_out = 2 doubles (re, im) per wave-chunk.
hipError_t launch_cplx(int n, const WalkParams& p, int grid, hipStream_t s);
hipError_t cplx_occupancy(int n, int* blocks_per_cu);

// Complex double-double dense walk (walk_cplxdd.hip), n <=
// SUP_CPLX_QUAD_MAX_DEVICE_N (larger: hipErrorInvalidValue): p.cols as
// launch_cplx's; p.x0 = 4 NP doubles (re.hi, re.lo, im.hi, im.lo blocks);
// p.chunk_out = 4 doubles (re.hi, re.lo, im.hi, im.lo) per wave-chunk.
hipError_t launch_cplxdd(int n, const WalkParams& p, int grid, hipStream_t s);
hipError_t cplxdd_occupancy(int n, int* blocks_per_cu);

// Exact complex residue walk (walk_cplxexact.hip), n <=
// SUP_CPLX_EXACT_MAX_DEVICE_N (larger: hipErrorInvalidValue): p.cols / p.x0 as
// launch_cplx's, of the doubled matrix; rows multiplied in exact groups of g
// (1 or 2); e.wave_out = 2 kMaxCxPrimes doubles per wave of the grid.
hipError_t launch_cplxexact(int n, int g, const WalkParams& p, const CxExactParams& e, int grid, hipStream_t s);
hipError_t cplxexact_occupancy(int n, int g, int* blocks_per_cu);

// Batched complex walk (walk_cplxb.hip, n <= 32): the wave-chunks of
// p.chunk_count >> hbits matrices in one queue; global chunk a is chunk
// a & (2^hbits - 1) of matrix a >> hbits.  p.cols / p.x0 = the matrices'
// tables / start vectors one after another (walk_cplx's layout each),
// p.chunk_out = 2 doubles per global chunk.
hipError_t launch_cplx_batch(int n, const WalkParams& p, int hbits, int grid, hipStream_t s);
hipError_t cplx_batch_occupancy(int n, int* blocks_per_cu);
// Where a slab's matrices come from (device pointers): `mats`, K matrices of
// 2 n^2 doubles, or — U non-null — the R x C matrix U (row-major interleaved,
// C its row length) and the slab's index lists (K x n each).
struct CplxBatchSrc {
  const double* mats;
  const double* U;
  const int32_t* rows;
  const int32_t* cols;
  int C;
  int pad_;
};
// The tables and start vectors of K matrices of order n (cplx_batch.hip).
hipError_t launch_cplx_batch_prepare(const CplxBatchSrc& src, int n, uint64_t K, double* tabs, double* x0s,
                                     hipStream_t s);
// out[2k], out[2k + 1] = (4(n&1) - 2) x the pairwise tree over matrix k's
// 2^hbits (re, im) partials at parts + 2 (k << hbits).
hipError_t launch_cplx_batch_fold(const double* parts, int n, int hbits, uint64_t K, double* out, hipStream_t s);

// One-walk permanent minors (walk_cplxm.hip, 2 <= n <= 32 rows, q = n - 1
// columns): queue entry a walks global chunk p.chunk_begin + a, chunk
// & (2^hbits - 1) of matrix >> hbits in the layout of order q.  p.cols / p.x0
// = the matrices' tables (Re, then Im plane, each 2 max(q-1, 1) x NP) / start
// vectors one after another; the partial of output j goes to
// p.chunk_out[2 ((matrix n + j) ostride + a - (matrix << hbits))].
hipError_t launch_cplx_minors(int n, const WalkParams& p, int hbits, unsigned long long ostride, int grid,
                              hipStream_t s);
hipError_t cplx_minors_occupancy(int n, int* blocks_per_cu);
// The tables and start vectors of K such matrices from U (src.C its row
// length) and the slab's index lists (rows K x n, cols K x (n - 1));
// cplx_minors.hip.  src.mats is not used.
hipError_t launch_cplx_minors_prepare(const CplxBatchSrc& src, int n, uint64_t K, double* tabs, double* x0s,
                                      hipStream_t s);

// Collision-aware complex walk (walk_cplxf.hip, n <= 64): the wave-chunks of a
// slab of matrices in one queue, described by FockParams (cplx_fock.hpp).
hipError_t launch_cplx_fock(int n, const FockParams& p, int grid, hipStream_t s);
hipError_t cplx_fock_occupancy(int n, int* blocks_per_cu);
// The signed column tables and x(0) of the K matrices of a slab, written from
// U (C its row length) and the slab's index lists (K x n each) as
// cplx_fock.cpp's fock_append writes them on the host: mats[k] names matrix
// k's offsets, side and groups (grp: index value, multiplicity pairs).
hipError_t launch_cplx_fock_prepare(const double* U, int C, const int32_t* rows, const int32_t* cols, const int32_t* grp,
                                    const FockMat* mats, int n, uint64_t K, double* tabs, double* x0s, hipStream_t s);
// out[2k], out[2k + 1] = 2 x fock_fold over matrix k's (re, im) partials at
// parts + 2 mats[k].chunk0 (cplx_fock.hip).
hipError_t launch_cplx_fock_fold(const double* parts, const FockMat* mats, uint64_t K, double* out, hipStream_t s);

// Collision-aware one-walk minors (walk_cplxfm.hip, 2 <= n <= 32 rows): the
// slab's tables have n rows; the partial of output j of chunk `local` of
// matrix M goes to p.chunk_out[2 (n M.chunk0 + j M.chunks + local)].  Its
// tables and x(0) are launch_cplx_fock_prepare's with side 0.
hipError_t launch_cplx_fock_minors(int n, const FockParams& p, int grid, hipStream_t s);
hipError_t cplx_fock_minors_occupancy(int n, int* blocks_per_cu);
// out[2 (k n + j)], [.. + 1] = 2 x fock_fold over output j of matrix k's
// partials at parts + 2 (n mats[k].chunk0 + j mats[k].chunks) (cplx_fock.hip).
hipError_t launch_cplx_fock_minors_fold(const double* parts, const FockMat* mats, uint64_t K, int n, double* out,
                                        hipStream_t s);

// Hafnian / loop hafnian walk (walk_haf.hip, n <= 64, one kernel per form): the
// wave-chunks of a slab of matrices in one queue, described by HafParams
// (haf.hpp).
hipError_t launch_haf(bool loop, const HafParams& p, int grid, hipStream_t s);
hipError_t haf_occupancy(bool loop, int* blocks_per_cu);
// The tables of the K matrices of a slab (haf.hpp haf_entry), written from A
// (M x M), mu (M, or null for the plain hafnian) and the groups in grp.
hipError_t launch_haf_prepare(const double* A, int M, const double* mu, const int32_t* grp, const HafMat* mats,
                              uint64_t K, double* tabs, hipStream_t s);
// out[2k], out[2k + 1] = 2 x fock_fold over matrix k's partials, divided by div.
hipError_t launch_haf_fold(const double* parts, const HafMat* mats, uint64_t K, double div, double* out,
                           hipStream_t s);
// The ragged loop-hafnian batch (walk_lhafe.hip): the same queue with an order
// and a coefficient row per matrix (HafMat::ord; p.coef = the pool of rows, p.n
// unused), and a prepare that reads row mu_row[k] of mus (M complex each) for
// matrix k.  The fold is launch_haf_fold with div = 1.
hipError_t launch_lhafe(const HafParams& p, int grid, hipStream_t s);
hipError_t lhafe_occupancy(int* blocks_per_cu);
hipError_t launch_lhafe_prepare(const double* A, int M, const double* mus, const int32_t* mu_row, const int32_t* grp,
                                const HafMat* mats, uint64_t K, double* tabs, hipStream_t s);

// Fixed-order pairwise reduction of `count` doubles into *out (64-way passes,
// zero padded; mirrored by oracle/oracle.c orc_pairwise_reduce).  `scratch`
// must hold ceil(count/64) + ceil(count/4096) + ... doubles.
// reset_counter (optional): zeroed by the first pass, which runs after the
// walk that used it (the next launch's queue then needs no memset).
// flag (optional, count > 1): the last pass stores `seq` there after *out,
// system-scope ordered (mapped host memory: the host waits on it).
hipError_t launch_pairwise_reduce(const double* in, uint64_t count, double* scratch, double* out,
                                  hipStream_t s, unsigned int* reset_counter = nullptr, unsigned int* flag = nullptr,
                                  unsigned seq = 0);
uint64_t pairwise_scratch_size(uint64_t count);
// *out = sum of `count` unsigned values (zeroed first, on stream s).
hipError_t launch_sum_visited(const unsigned* in, uint64_t count, unsigned long long* out, hipStream_t s);
// walk_sparse counts the chunks it ended (walk_sparse.hip count_chunk_end) in
// kChunkEndWords unsigned words, zero before the launch; their sum is the
// count.  The wave holding ticket g adds to word chunk_end_word(g): one word in
// 64 bytes, so the adds of waves with neighbouring tickets meet in no line.
constexpr unsigned kChunkEndSlots = 1024, kChunkEndWords = kChunkEndSlots * 16;
constexpr unsigned chunk_end_word(unsigned g) { return (g & (kChunkEndSlots - 1u)) * 16u; }
// The same tree over each of `nseg` consecutive segments of `count` doubles
// (a leaf batch's chunk partials): out[i] is bit-identical to
// launch_pairwise_reduce over segment i alone.  `scratch` holds nseg times
// pairwise_scratch_size(count).
hipError_t launch_pairwise_reduce_seg(const double* in, uint64_t count, uint64_t nseg, double* scratch, double* out,
                                      hipStream_t s);

}  // namespace sup
