/*
 * superman.h — C ABI of the MI355X-native Ryser / Gray-code permanent engine.
 *
 * This is the drop-in boundary for the reference's GPU exact-permanent path
 * (kamerkaya/SUPerman, v1 top level).  Every entry point below names the
 * reference symbol it replaces (file:line in the reference tree).  The
 * reference's wrappers are C++ templates over the storage type T in
 * {int, float, double}; here T travels as a `sup_dtype` tag next to a
 * `const void*`, so the ABI is plain C (pointers, sizes, an error code).
 *
 * Conventions (reference behaviour kept, reference defects fixed):
 *   - Host arrays are borrowed read-only; the caller owns them
 *     (reference: main.cu:501-528 new[]/delete[] around RunAlgo).
 *   - Device memory is owned by the library (per-device context, created on
 *     first use, reused across calls).
 *   - Every function returns 0 (SUP_OK) or a negative SUP_E* code; the
 *     message is available from sup_last_error() (thread-local).  The
 *     reference reports nothing (no cudaGetLastError anywhere).
 *   - The permanent is written through `out` as a double
 *     (reference returns it by value; interface_connector.c:22 truncated it
 *     to int — not reproduced).
 *   - X is always fp64 (the reference v1 float-X path, algo.h:664 /
 *     gpu_exact_dense.cu:336, is numerically wrong on real matrices and is
 *     not reproduced).
 *   - Device 0 is the default device (the reference hard-codes
 *     cudaSetDevice(1), gpu_exact_dense.cu:664); `sup_opts.device_id`
 *     selects another one (v2 flag -l, revised_perman/main.cpp:1443).
 */
#ifndef SUPERMAN_H
#define SUPERMAN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SUP_ABI_VERSION 29  /* 29: sup_hafnian_complex_quad, sup_loop_hafnian_complex_quad, SUP_HAFNIAN_QUAD_MAX_DEVICE_N; 28: sup_loop_torontonian_each, sup_threshold_sample; 27: sup_loop_hafnian_table, sup_loop_hafnian_table_plan, SUP_LHAF_TABLE_MAX_ENTRIES; 26: sup_loop_hafnian_complex_each, sup_gbs_sample; 25: sup_torontonian_table, sup_loop_torontonian_table, sup_mobius_subsets, SUP_TORONTONIAN_TABLE_MAX_N; 24: sup_loop_torontonian, sup_loop_torontonian_range, sup_loop_torontonian_plan, sup_ltor_exp, sup_ltor_exp_device, SUP_LOOP_TORONTONIAN_MAX_DEVICE_N; 23: sup_hafnian_complex_exact; 22: sup_torontonian, sup_torontonian_range, sup_torontonian_plan, SUP_TORONTONIAN_MAX_DEVICE_N; 21: sup_hafnian_complex_pt, sup_loop_hafnian_complex_pt, sup_hafnian_complex_pt_range, sup_hafnian_complex_pt_plan, SUP_HAFNIAN_PT_MAX_DEVICE_N; 20: sup_hafnian_complex, sup_loop_hafnian_complex, sup_hafnian_complex_plan; 19: sup_perman_complex_exact, sup_perman_complex_exact_range, SUP_CPLX_EXACT_MAX_DEVICE_N; 18: sup_perman_complex_quad, sup_perman_complex_quad_range, SUP_CPLX_QUAD_MAX_DEVICE_N; 17:sup_perman_complex_fock_minors, sup_perman_complex_fock_minors_plan, sup_boson_sample_fock; 16: sup_plan_census; 15: sup_perman_complex_minors, sup_perman_complex_minors_range, sup_boson_sample; 14: sup_perman_complex_fock, sup_perman_complex_fock_plan; 13: sup_perman_exact_range, sup_perman_quad_range, sup_perman_exact / sup_perman_quad report the walk that ran; 12: sup_perman_complex_batch, sup_perman_complex_submatrices; 11: sup_perman_complex, sup_perman_complex_range, sup_read_mtx_complex; 10: sup_opts.timing, sup_kernel_time (round 6); 9: sup_device_warmup, sup_opts.use_rccl = -1 (round 6); 8: sup_device_checks (round 5); 7: sup_rccl_devices, sup_stats.seg_cached_bits / seg_pair_bits */

/* ---- error codes ------------------------------------------------------ */
#define SUP_OK            0
#define SUP_EINVAL      (-1)   /* bad argument (n out of range, null pointer, bad range) */
#define SUP_ENODEV      (-2)   /* no HIP device / device id out of range                 */
#define SUP_EHIP        (-3)   /* a HIP runtime call failed                              */
#define SUP_ERCCL       (-4)   /* an RCCL call failed                                    */
#define SUP_ENOMEM      (-5)   /* host or device allocation failed                       */
#define SUP_EIO         (-6)   /* matrix file could not be read                          */
#define SUP_EUNSUPPORTED (-7)  /* algorithm id / option combination not provided         */

#define SUP_MAX_N 64           /* 64-bit Gray index: reference limit algo.h:752,781      */
#define SUP_MAX_READ_N 4096    /* MatrixMarket input and sup_decompose: larger matrices
                                  are accepted when the -o reductions shrink every leaf
                                  to <= SUP_MAX_N                                       */

/* ---- storage type of the input matrix (reference template parameter T) -- */
typedef enum {
  SUP_INT32 = 0,    /* file header "int"    (main.cu:494) */
  SUP_FLOAT32 = 1,  /* file header "float"  (main.cu:530) */
  SUP_FLOAT64 = 2   /* file header "double" (main.cu:563) */
} sup_dtype;

/* ---- kernel family ------------------------------------------------------ */
typedef enum {
  SUP_KERNEL_DENSE = 0,       /* kernel_xshared_coalescing_mshared          gpu_exact_dense.cu:329-399.
                                 The engine runs the plain dense walk, or the prefix-blocked walk when
                                 its cost model says the matrix's zeros make that cheaper (same sum) */
  SUP_KERNEL_SPARYSER = 1,    /* kernel_xshared_coalescing_mshared_sparse   gpu_exact_sparse.cu:455-552 */
  SUP_KERNEL_SKIPPER = 2,     /* kernel_xshared_coalescing_mshared_skipper  gpu_exact_sparse.cu:555-670 */
  SUP_KERNEL_DENSE_PLAIN = 3, /* always the plain dense walk (2n fp64 ops per Gray step)                */
  SUP_KERNEL_SEGMENTED = 4,   /* always the segmented walk specialised for the matrix pattern (n >= 10;
                                 the GPU entry points compile it with hiprtc, sup_perman_cpu runs the
                                 same operations on host threads)                                       */
  SUP_KERNEL_DENSE_LDS = 5    /* the plain dense walk with X and the walk columns staged in LDS, as the
                                 reference kernel (gpu_exact_dense.cu:329-399); bit-identical to
                                 SUP_KERNEL_DENSE_PLAIN, kept to measure the layout    */
} sup_kernel;

/* ---- multi-device scheduling policy -------------------------------------- */
typedef enum {
  SUP_SCHED_SINGLE = 0,   /* one device           (-p4; gpu_exact_dense.cu:640-699)            */
  SUP_SCHED_STATIC = 1,   /* static split         (-p5; gpu_exact_dense.cu:701-774)            */
  SUP_SCHED_CHUNKS = 2,   /* dynamic chunk queue  (-p6/-p8; gpu_exact_dense.cu:776-904,
                                                   gpu_exact_sparse.cu:1192-1324)            */
  SUP_SCHED_MANUAL = 3    /* manual distribution  (-p66; gpu_exact_dense.cu:913-990,
                             gpu_exact_sparse.cu:1328-1400): 3/8, 3/8, 1/8, 1/8 of the space
                             on devices 0-3 (gpu_num 4, as main.cu:71 passes; with fewer
                             devices the pieces wrap round modulo gpu_num)             */
} sup_sched;

typedef struct {
  int gpu_num;        /* devices to use (-d); default 1                                      */
  int device_id;      /* first device (v2 -l); default 0                                     */
  int threads;        /* host threads for the CPU worker (-t); default 16 (main.cu:333)      */
  int cpu_worker;     /* -c together with -g: a CPU thread also takes chunks                 */
  int grid_dim;       /* 0 = auto (resident-wave sized); reference default 2048              */
  int block_dim;      /* 0 = auto (256); the engine only supports 256                         */
  int walk_log2;      /* 0 = auto (the segmented walk lengthens its wave-chunks where its    */
                      /*  steps are cheap); else each lane walks 2^walk_log2 Gray steps per  */
                      /*  wave-chunk (sup_perman, sup_perman_shard, sup_plan_info)           */
  int chunk_log2;     /* 0 = auto; for SUP_SCHED_CHUNKS: wave-chunks per queue item = 2^x    */
  int use_rccl;       /* 1: multi-device partials combined by one RCCL all-reduce (bit-     */
                      /*    identical to the host combine); 2: also with a single device;   */
                      /*    -1: RCCL when the devices are distinct physical GPUs, else the  */
                      /*    host pairwise tree (the perman CLI's default); 0: host tree     */
  int verbose;        /* print per-device / per-chunk timing lines like the reference        */
  int jit;            /* segmented walk specialised for the matrix pattern (hiprtc, gfx950):  */
                      /*  -1 never; 0 auto: when its cost model wins and the predicted walk  */
                      /*  time saved exceeds what the plan costs (3 s, or twice this host's  */
                      /*  last cold plan; 0.1 s with the matrix's choices on disk; the first */
                      /*  decision for a matrix holds for the process); 1 whenever its cost  */
                      /*  model wins                                                         */
  const char* checkpoint; /* SUP_SCHED_CHUNKS (-p6/-p8) only, NULL = none: file recording every */
                      /*  finished queue item's partial (appended and flushed as items finish;*/
                      /*  header: plan fingerprint, chunk range, item size).  A call given a  */
                      /*  file with a matching header takes the items it lists instead of    */
                      /*  walking them, so an interrupted run resumes; the result is bit-    */
                      /*  identical to an uninterrupted one.  A mismatching header is         */
                      /*  SUP_EINVAL.  (ABI version 6)                                        */
  int timing;         /* sup_perman_shard: 1 (default) sup_stats.kernel_ms of the call (it waits */
                      /*  for the walk's end event); 0: the walk's HIP events are recorded but */
                      /*  read later by sup_kernel_time (kernel_ms 0) — the call returns as   */
                      /*  soon as its result is there (~8 us sooner on a 0.5 ms walk).        */
                      /*  (ABI version 10)                                                    */
} sup_opts;

typedef struct {
  double   kernel_ms;       /* device time of the walk kernels (max over devices, hipEvents)   */
  double   wall_ms;         /* host wall time of the call (upload + launch + reduce)           */
  uint64_t gray_steps;      /* nominal Gray steps = 2^(n-1)                                    */
  uint64_t visited_steps;   /* steps whose product was actually evaluated (sparse/skipper)     */
  int      devices_used;
  int      lane_bits;       /* L: Gray bits spread over the 64 lanes of a wave                  */
  int      walk_bits;       /* m: Gray bits walked by every wave-chunk                          */
  int      grid;            /* blocks per launch (256 threads each) on each device             */
  int      chunks_done_cpu; /* queue items taken by the CPU worker                              */
  double   partials[16];    /* per-device partial sums (before the final combine)              */
  int      walk_kind;       /* walk actually run: 0 dense, 1 prefix-blocked (SpaRyser), 2 SkipPer,
                               3 segmented (pattern-specialised, sup_opts.jit), 4 dense with X
                               in LDS (SUP_KERNEL_DENSE_LDS)                                     */
  int      leaves;          /* permanents computed: 1, or the leaf count of sup_perman_reduced   */
  double   est_ops_per_step;/* cost model: fp64 VALU ops per Gray step and lane                 */
  double   jit_ms;          /* hiprtc compile time spent by this call (0 when cached / unused)   */
  int      items_resumed;   /* queue items taken from sup_opts.checkpoint instead of walked      */
  int16_t  seg_cached_bits; /* segmented walk (walk_kind 3): cached walk bits of the plan run    */
  int16_t  seg_pair_bits;   /* segmented walk: specialised pair bits (0 for other walks);
                               sup_perman_exact, sup_perman_exact_range: G, the rows the residue
                               walk multiplies exactly before each reduction (1, 2 or 4)         */
} sup_stats;

/* Fill `o` with defaults. */
void sup_opts_init(sup_opts* o);

/* Library metadata. */
int         sup_abi_version(void);
const char* sup_last_error(void);     /* thread-local message of the last failing call */
int         sup_device_count(int* count);
/* The physical HIP device of logical devices 0..ndev-1 as the -R RCCL combine
 * uses them (its communicators, slot buffers and streams); SUP_DEVICE_MAP may
 * permute or repeat physical ids, and SUP_ERCCL is returned when two logical
 * devices share one GPU (RCCL needs distinct devices).  No HIP call. */
int         sup_rccl_devices(int ndev, int* phys);
/* Device-placement assertions passed so far in this process.  With
 * SUP_CHECK_DEVICE=1 in the environment, every allocation, module load and
 * launch of a device thread first checks that the thread's HIP device is the
 * physical device behind the logical device whose context it uses, and that
 * this logical device is the one the thread last selected (a mismatch fails
 * the call with SUP_EHIP); 0 when the mode is off.  Tests and diagnostics. */
uint64_t    sup_device_checks(void);
/* Initialise the HIP runtime, the contexts of devices [device_id, device_id +
 * gpu_num) and the ahead-of-time walk code objects of order n (0: none), so a
 * caller can run it on a thread beside its planning (the perman CLI does).
 * Thread-safe; a later call on the same devices returns at once. */
int         sup_device_warmup(int device_id, int gpu_num, int n);
/* The walk-kernel times (HIP events on the walk's stream) of the
 * sup_perman_shard calls made with sup_opts.timing = 0 on the calling thread's
 * context — logical device `device_id` and the thread's context lane — since
 * the last sup_kernel_time there: waits for them, returns their sum
 * (*total_ms) and count (*launches), and starts a new tally.  The tally
 * belongs to the context, not the thread: threads that share a device and
 * lane share it.  Any pointer may be NULL (the tally is still reset). */
int         sup_kernel_time(int device_id, double* total_ms, uint64_t* launches);

/* ------------------------------------------------------------------------ *
 * Generic entry point.  `mat` is n x n row-major of type `t` (already
 * preprocessed by the caller when the reference would have rewritten it:
 * SortOrder / SkipOrder, util.h:553-684).  `kernel` picks the Gray walk,
 * `sched` the device policy.  Result: the permanent, fp64.
 * Replaces RunAlgo<T>'s GPU exact branch (main.cu:30-143).
 * ------------------------------------------------------------------------ */
int sup_perman(const void* mat, sup_dtype t, int n, sup_kernel kernel, sup_sched sched,
               const sup_opts* o, double* out, sup_stats* st);

/* Partial Ryser sum over reference Gray indices [start, end):
 *   sum_{i in [start,end)} (-1)^i * prod_j x_j(gray(i))
 * with x(0) = Nijenhuis-Wilf start vector (gpu_exact_dense.cu:642-652).
 * This is exactly what the reference chunk helpers return
 * (cpu_perman64 gpu_exact_dense.cu:6-69; cpu_perman64_sparse
 * gpu_exact_sparse.cu:6-87; cpu_perman64_skipper :89-191) except that index
 * 0 (the p0 term) is included when start == 0.  start and end must be
 * multiples of 2^(lane_bits + walk_bits) reported by the engine for this n
 * (any power-of-two aligned chunk boundary >= 64 works), or end == 2^(n-1). */
int sup_partial(const void* mat, sup_dtype t, int n, sup_kernel kernel,
                uint64_t start, uint64_t end, const sup_opts* o, double* out, sup_stats* st);

/* Shard `shard` of `nshards` of the engine's own enumeration of the full sum
 * (same plan as sup_perman): the shards' partials add up to
 * perm / (4(n&1)-2).  For one process per GPU (torch.distributed / MPI):
 * each rank computes its shard on `o->device_id`, then one all-reduce. */
int sup_perman_shard(const void* mat, sup_dtype t, int n, sup_kernel kernel, int shard, int nshards,
                     const sup_opts* o, double* out_partial, sup_stats* st);

/* The plan sup_perman would run with options `o` (NULL = defaults; o->jit and
 * o->gpu_num matter): walk kind (0 dense, 1 prefix/SpaRyser, 2 SkipPer,
 * 3 segmented), engine-bit -> column map (n-1 entries), lane and walk bits,
 * and (segmented walk) the walk bits held in every state (*cached_bits, 0-4)
 * and the pair bits with a specialised step (*pair_bits, 3-8; the walk loop is
 * unrolled by 2^pair_bits pair steps); *est_ops_per_step = the walk's cost
 * model (sup_stats.est_ops_per_step); any pointer may be NULL.  For the test
 * harness's bit-exact mirror of the enumeration. */
int sup_plan_info(const void* mat, sup_dtype t, int n, sup_kernel kernel, const sup_opts* o, int* walk_kind,
                  int* colmap, int* lane_bits, int* walk_bits, int* cached_bits, int* pair_bits,
                  double* est_ops_per_step);

/* Op census of the plan sup_plan_info describes (ABI 16): the fp64 VALU
 * operations per Gray step of the segmented walk's generated kernel, by class,
 * counted from the generated statements.  census[0 .. SUP_CENSUS_CLASSES):
 *    0 x^0 column adds of the specialised pair steps
 *    1 derived row-copy adds              2 outer tree node re-forms
 *    3 segment 0 tree node re-forms       4 D fmas
 *    5 accumulates                        6 the two-level lane sum
 *    7 generic shared step: column adds   8 its row-copy adds   9 its re-forms
 *   10 specialised high-bit steps: column adds   11 their row-copy adds
 *   12 their re-forms
 * Classes 0..12 are the walk loop; added in index order they give
 * sup_plan_info's *est_ops_per_step exactly.  Beside them, not in that sum:
 *   13 chunk start and end, amortised over the chunk's 2^walk_bits Gray steps
 * (est_ops_per_step prices the walk loop; the planner prices a chunk start on
 * its own when it chooses the walk length).
 * *hi_bits = the walk bits above the specialised pair bits that have
 * straight-line steps of their own (the kernel's outer loop is unrolled by
 * 2^hi_bits; SUP_JIT_HI forces it).  Other walk kinds: zeros, *hi_bits = 0.
 * Any pointer may be NULL. */
#define SUP_CENSUS_CLASSES 14
int sup_plan_census(const void* mat, sup_dtype t, int n, sup_kernel kernel, const sup_opts* o, int* hi_bits,
                    double* census);

/* 64-bit fingerprint of the plan sup_perman / sup_perman_shard would run
 * with options `o` (walk kind, layout, engine column map, signed column
 * table, start vector, the segmented walk's cached / pair bits, budget and
 * kernel source).  One process per GPU: every rank plans on its own, and the
 * shards add up to the permanent only if all ranks walk the same plan —
 * all-gather the keys before summing (bench.py does, and aborts on a
 * mismatch). */
int sup_plan_key(const void* mat, sup_dtype t, int n, sup_kernel kernel, const sup_opts* o, uint64_t* key);

/* Build the plan sup_perman would run and, if it is the segmented walk,
 * compile its kernel now (hiprtc; no device needed) into the in-memory and
 * disk caches, so a later sup_perman does not pay the compile.  (A SkipPer
 * request on an integer matrix measures SkipPer's visited fraction on a
 * sample of its chunks when a device is visible, here and in sup_plan_info.)  *walk_kind =
 * the plan's walk kind; *compile_ms = hiprtc time spent (0 when cached). */
int sup_prepare(const void* mat, sup_dtype t, int n, sup_kernel kernel, const sup_opts* o, int* walk_kind,
                double* compile_ms);
/* Explicit CPU algorithm for the CLI's `-c` mode (reference RunAlgo cpu
 * branch, main.cu:186-238): the same wave-chunk walk on `threads` host
 * threads, bit-identical to the GPU kernels.  Never used as a fallback by the
 * GPU entry points above, which fail with SUP_ENODEV without a device. */
int sup_perman_cpu(const void* mat, sup_dtype t, int n, sup_kernel kernel, int threads,
                   double* out, sup_stats* st);

/* Exact permanent of an integer matrix (int32, or float/double holding
 * integers; |a| < 2^31, row sums of |a| < 2^31).  The reference computes int
 * and -b (binary) inputs in fp64 (rounded beyond 2^53); here the same Ryser /
 * Gray-code walk runs on 2A in residue arithmetic modulo primes < 2^42 and
 * the residues are joined by CRT (walk_exact.hip, exact.cpp), with a built-in
 * divisibility self-check.  *out receives the signed decimal integer,
 * NUL-terminated (520 bytes always suffice).  o->gpu_num devices from
 * o->device_id take power-of-two items of wave-chunks from a queue
 * (o->chunk_log2 wave-chunks each, 0 = ~16 items per taker; one device alone
 * walks its whole range), and with o->cpu_worker a CPU thread (o->threads
 * host threads) takes items too; on_cpu = 1 runs o->threads host threads
 * instead.  The result never depends on who took which item (residue sums).
 * st (optional): kernel_ms (max over devices), wall_ms, devices_used,
 * gray_steps, chunks_done_cpu, lane_bits, walk_bits, walk_kind (0 the dense
 * residue kernel, 1 the prefix-blocked one: whichever the planner ran) and
 * seg_pair_bits = G, its exact group size. */
int sup_perman_exact(const void* mat, sup_dtype t, int n, const sup_opts* o, int on_cpu, char* out,
                     size_t out_len, sup_stats* st);

/* Wave-chunks [c0, c1) of sup_perman_exact's walk (ABI 13): per prime, the sum
 * of the terms (-1)^|S| prod_j X_j(S) of the doubled matrix 2A over the
 * range's subsets, in [0, p).  The plan is sup_perman_exact's plan of 2A with
 * the default layout, or o->walk_log2 walk bits when non-zero (m =
 * min(walk_log2, n - 1 - lane_bits); walk_log2 outside [0, 31]: SUP_EINVAL);
 * it has 2^(n-1-lane_bits-walk_bits) chunks.  Chunk a covers the subsets S of
 * engine bits whose bits >= lane_bits + walk_bits are gray(a) = a ^ (a >> 1)
 * and whose low bits are arbitrary; engine bit e is matrix column colmap[e]
 * (colmap: optional, n - 1 ints), and X_j(S) = 2 a_j,n-1 - sum_c a_jc +
 * 2 sum_{e in S} a_j,colmap[e].  The whole range, times 4(n&1) - 2, divided by
 * 2^(n-1), is the permanent; residues of disjoint ranges add modulo p.
 * form: 0 the planner's choice as in sup_perman_exact, 1 the dense kernel with
 * the greedy column order, 2 the prefix-blocked kernel with that order (no
 * chunk-end search; SUP_EINVAL when the layout has no walk bits, n <= 7).
 * group: 0 the cost model's choice, or G = 1, 2, 4 rows multiplied exactly
 * before each reduction.  The primes are sup_perman_exact's for that G: the
 * largest below 2^pbits, pbits = min(42, 51 - G xbits), row sums of |a| below
 * 2^xbits, until their product exceeds 8 |T|'s bound; a G whose pbits is
 * below 20 is SUP_EINVAL (the message names xbits).
 * primes, residues: cap entries each, *nprimes of them written; cap below the
 * prime count is SUP_EINVAL before any walk (128 always suffice).  More than
 * 8 primes take several launches.  One device (o->device_id; o->gpu_num is
 * not used), or on_cpu = 1: o->threads host threads, the same residues.
 * c0 > c1, c1 beyond the plan's chunks, a null matrix or output, n outside
 * [1, 64]: SUP_EINVAL; c0 == c1: zeros.
 * st: kernel_ms (summed over the launches), wall_ms, gray_steps = (c1 - c0)
 * 2^(lane_bits + walk_bits), devices_used, lane_bits, walk_bits, walk_kind (0
 * dense, 1 prefix-blocked: the kernel that ran), seg_pair_bits = G, leaves 1,
 * est_ops_per_step (the plan's fp64 cost model). */
int sup_perman_exact_range(const void* mat, sup_dtype t, int n, uint64_t c0, uint64_t c1, const sup_opts* o,
                           int on_cpu, int form, int group, uint64_t* primes, uint64_t* residues, int cap,
                           int* nprimes, int* colmap, sup_stats* st);

/* The permanent in double-double (~106-bit significand): the MI355X form of
 * the reference's quad-precision calculation (v2 `-q`,
 * revised_perman/main.cpp:141-142 -> parallel_perman64<__float128,S>,
 * cpu_algos.hpp:761-873, CPU only).  The dense Ryser / Gray walk of
 * sup_perman (default layout, same wave-chunks) with every value a
 * double-double (walk_dd.hip); perm = *out_hi + *out_lo (out_lo may be NULL).
 * o->gpu_num devices from o->device_id split the wave-chunks statically;
 * on_cpu = 1 runs the same operations on o->threads host threads.  Chunk
 * partials are combined in one fixed pairwise order, so the result is
 * bit-identical for any device or thread count.  ~8x the fp64 walk's work
 * (16n + 13 fp64 ops per Gray step).  st: walk_kind is the kernel the planner
 * ran (0 dense, 1 prefix-blocked), lane_bits, walk_bits, and est_ops_per_step
 * comes from that plan (16n + 13 for the dense walk, scaled by the plan's
 * share of the dense cost model for the prefix-blocked one). */
int sup_perman_quad(const void* mat, sup_dtype t, int n, const sup_opts* o, int on_cpu, double* out_hi,
                    double* out_lo, sup_stats* st);

/* Wave-chunks [c0, c1) of sup_perman_quad's walk (ABI 13): the double-double
 * chunk partials of that range folded by the pairwise tree over c - c0 (an odd
 * last element moves up as it is), NOT scaled by 4(n&1) - 2, as *out_hi +
 * *out_lo (both required).  Plan and start vector are sup_perman_quad's, with
 * o->walk_log2 walk bits when non-zero; chunks, colmap, form and the error
 * cases as sup_perman_exact_range, with x_j(S) = a_j,n-1 - sum_c a_jc / 2 +
 * sum_{e in S} a_j,colmap[e].  Aligned power-of-two ranges folded pairwise in
 * order (double-double adds) reproduce the whole range's bits, and the whole
 * range with form 0 and walk_log2 0, times 4(n&1) - 2, is sup_perman_quad's
 * result bit for bit.  One device (o->device_id; o->gpu_num
 * is not used) or on_cpu = 1: o->threads host threads, bit-identical.
 * st: as sup_perman_exact_range's, est_ops_per_step as sup_perman_quad's. */
int sup_perman_quad_range(const void* mat, sup_dtype t, int n, uint64_t c0, uint64_t c1, const sup_opts* o,
                          int on_cpu, int form, double* out_hi, double* out_lo, int* colmap, sup_stats* st);

/* The permanent of a complex fp64 matrix (ABI 11).  The reference refuses
 * complex input (revised_perman/main.cpp:1557); boson-sampling amplitudes are
 * permanents of dense complex submatrices of unitaries.
 * mat: n x n row-major, interleaved (re, im) doubles: 2 n^2 doubles; n in
 * [1, 64].  The dense Ryser / Gray walk of sup_perman (default layout, or
 * o->walk_log2 walk bits when non-zero; same wave-chunks) with every value a
 * complex fp64 pair (walk_cplx.hip): 6n - 2 fp64 ops per Gray step, ~3x the
 * fp64 walk.  o->gpu_num devices from o->device_id split the wave-chunks
 * statically; on_cpu = 1 runs the same operations in the same order on
 * o->threads host threads.  Chunk partials are combined in one fixed pairwise
 * tree over the chunk index, so the result is a function of (matrix, walk
 * bits) only: bit-identical for any device count, split or thread count.
 * Non-finite input propagates.  No device with on_cpu = 0: SUP_ENODEV (no
 * silent CPU fallback).  st: kernel_ms, wall_ms, gray_steps, devices_used,
 * lane_bits, walk_bits, grid, est_ops_per_step = 6n. */
int sup_perman_complex(const double* mat, int n, const sup_opts* o, int on_cpu,
                       double* out_re, double* out_im, sup_stats* st);
/* The part of the sum from wave-chunks [c0, c1) of the plan (o->walk_log2
 * honoured; the plan has 2^(n-1-lane_bits-walk_bits) chunks), folded by the
 * pairwise tree over c - c0, NOT scaled by 4(n&1)-2.
 * Aligned power-of-two ranges folded pairwise in order reproduce
 * sup_perman_complex's bits.  One device (o->device_id) or host threads.
 * c0 > c1 or c1 beyond the plan's chunks: SUP_EINVAL. */
int sup_perman_complex_range(const double* mat, int n, uint64_t c0, uint64_t c1,
                             const sup_opts* o, int on_cpu,
                             double* out_re, double* out_im, sup_stats* st);

/* The permanent of a complex fp64 matrix in double-double (ABI 18): the
 * higher-precision result the fp64 complex entries are judged against, as
 * sup_perman_quad is for the real ones.  mat as sup_perman_complex's (n x n
 * row-major interleaved fp64, n in [1, 64]); out = 4 doubles, re_hi, re_lo,
 * im_hi, im_lo: Re perm = re_hi + re_lo, Im perm = im_hi + im_lo, each a
 * normalised pair (~100 bits).  sup_perman_complex's plan and wave-chunks
 * (default layout, or o->walk_log2 walk bits) with every value a complex
 * double-double (walk_cplxdd.hip, cxdd.hpp); the start vector's row sums are
 * accumulated in double-double.  The whole sum is scaled by 4(n&1) - 2,
 * exactly.  o->gpu_num devices from o->device_id split the wave-chunks
 * statically; on_cpu = 1 runs the same operations in the same order on
 * o->threads host threads.  Chunk partials are combined in one fixed pairwise
 * tree over the chunk index (double-double adds per part): bit-identical for
 * any device count, split or thread count.
 * The device walk holds 8n registers of state per lane and serves n <=
 * SUP_CPLX_QUAD_MAX_DEVICE_N, the largest order (contiguous from 1) whose
 * kernel compiles without scratch memory; the host twin serves every n <= 64.
 * Checks, in this order: a null pointer, n outside [1, 64] or o->walk_log2
 * outside [0, 31]: SUP_EINVAL; on_cpu = 0 and n above the cap:
 * SUP_EUNSUPPORTED, the message naming the cap (on any machine, with or
 * without a device: no silent CPU fallback); on_cpu = 0 and no device:
 * SUP_ENODEV.  Non-finite input propagates.
 * st: kernel_ms, wall_ms, gray_steps, devices_used, lane_bits, walk_bits,
 * grid, est_ops_per_step = 86n - 28: 18n for the column add, 68(n-1) for the
 * product, 40 for the accumulate, in dd.hpp's nominal op counts, as
 * sup_perman_quad's 16n + 13 (its column add is 10 instructions where dd.hpp
 * says 9: the kernel's loop holds 88n - 28 fp64 instructions per step). */
#define SUP_CPLX_QUAD_MAX_DEVICE_N 40
int sup_perman_complex_quad(const double* mat, int n, const sup_opts* o, int on_cpu,
                            double* out /* 4: re_hi, re_lo, im_hi, im_lo */, sup_stats* st);
/* The part of that sum from wave-chunks [c0, c1) of the plan (o->walk_log2
 * honoured; chunks, subsets and sign convention as sup_perman_quad_range's
 * with the identity column map), folded by the pairwise tree over c - c0 (an
 * odd last element moves up as it is), NOT scaled by 4(n&1) - 2.  Aligned
 * power-of-two ranges folded pairwise in order (double-double adds per part),
 * then scaled, reproduce sup_perman_complex_quad's bits.  One device
 * (o->device_id; o->gpu_num is not used) or host threads.  c0 == c1: zeros.
 * c0 > c1 or c1 beyond the plan's chunks: SUP_EINVAL; the other checks and st
 * as sup_perman_complex_quad's (gray_steps = (c1 - c0) 2^(lane_bits +
 * walk_bits)). */
int sup_perman_complex_quad_range(const double* mat, int n, uint64_t c0, uint64_t c1, const sup_opts* o,
                                  int on_cpu, double* out /* 4 */, sup_stats* st);

/* Exact permanent of a matrix of Gaussian integers (ABI 19): the complex
 * counterpart of sup_perman_exact, the integer truth the floating complex
 * entries are judged against.  mat as sup_perman_complex's (n x n row-major
 * interleaved fp64, n in [1, 64]), every part an integer with |part| < 2^31
 * and every row bound R_j = sum_c (|Re a_jc| + |Im a_jc|) < 2^31.
 * The Ryser / Gray sum runs on 2A: X_j(S) = 2 a_j,n-1 - sum_c a_jc + 2
 * sum_{e in S} a_je is a Gaussian integer with parts <= R_j, exact in two fp64
 * values; T = sum_S (-1)^|S| prod_j X_j(S), |Re T|, |Im T| <= 2^(n-1) prod_j
 * R_j, and perm = (4(n&1) - 2) T / 2^n.  Each product is formed in (Z/p)[i]
 * for primes p < 2^pbits in exact fp64 residue arithmetic (walk_cplxexact.hip,
 * cxexact.hpp): rows multiplied exactly in groups of G = 1 or 2 first, then a
 * residue (u, v), |u|, |v| < 1.5 p, times a group product (c, d) with parts <=
 * Y is (red(uc - vd), red(ud + vc)), exact while 1.5 p Y < 2^52.  G = 1: Y <
 * 2^xbits (R_j < 2^xbits), pbits = min(42, 51 - xbits), at least 20 within the
 * input limits; G = 2: Y <= 2 4^xbits, pbits = min(42, 51 - (2 xbits + 1)),
 * eligible while that is at least 20; a cost model picks the cheaper.  The
 * primes are the largest below 2^pbits, taken until their product exceeds 8
 * times the bound on |T|; the residues of Re T and Im T are joined separately
 * by CRT.  Both parts must be divisible by 2^(n-1): a built-in self-check (a
 * failure is SUP_EHIP with a message, never a wrong number).
 * sup_perman_complex's plan (default layout, identity column map; no
 * chunk-end skipping, column-order search or prefix-blocked form).
 * o->gpu_num devices from o->device_id split the wave-chunks statically, at
 * most 4 primes per launch; on_cpu = 1 runs the same residue operations on
 * o->threads host threads.  Residue sums are exact, so device and host agree
 * residue for residue for any split.  o->cpu_worker is not used.  A zero row
 * gives "0", "0" without a walk.
 * out_re / out_im: signed decimal integers, NUL-terminated; out_len applies to
 * each buffer, 640 bytes always suffice (|perm| <= prod R_j < 2^1984); a
 * shorter buffer that does not fit is SUP_EINVAL with the needed length in the
 * message.
 * The device walk serves n <= SUP_CPLX_EXACT_MAX_DEVICE_N, the largest order
 * (contiguous from 1) whose kernel compiles without scratch memory or spilled
 * registers for both G; the host twin serves every n <= 64.
 * Checks, in this order: a null pointer, n outside [1, 64], o->walk_log2
 * outside [0, 31], a non-integral or non-finite part, a part or row bound out
 * of range: SUP_EINVAL, the message naming the first offending (row, column,
 * part) or row; on_cpu = 0 and n above the cap: SUP_EUNSUPPORTED, the message
 * naming the cap (on any machine: no CPU fallback); on_cpu = 0 and no device:
 * SUP_ENODEV.
 * st: kernel_ms, wall_ms, gray_steps, devices_used, lane_bits, walk_bits,
 * grid, seg_pair_bits = G, leaves 1, est_ops_per_step = 2n + [G = 2] 4
 * floor(n/2) + P (10 ceil(n/G) - 2) fp64 instructions per Gray step and lane
 * in a launch with P primes (P = min(4, primes); the column add, the exact
 * pair products, and per prime 6 for the first reduction, 10 per further group
 * and 2 for the accumulate); the kernel's loop holds that count with P = 4. */
#define SUP_CPLX_EXACT_MAX_DEVICE_N 61
int sup_perman_complex_exact(const double* mat, int n, const sup_opts* o, int on_cpu, char* out_re, char* out_im,
                             size_t out_len, sup_stats* st);
/* Per prime, the residues in [0, p) of Re and Im of the part of T from
 * wave-chunks [c0, c1) of that walk (o->walk_log2 honoured; chunks, subsets
 * and sign convention as sup_perman_complex_quad_range's), NOT scaled:
 * disjoint ranges add modulo p, the whole range is T.  A zero row is walked
 * like any other.  group: 0 the cost model's G, 1 or 2 forces it (SUP_EINVAL
 * for other values, or when its primes would fall below 20 bits).  primes,
 * res_re, res_im: `cap` entries each; more primes than cap: SUP_EINVAL before
 * any walk; *nprimes = the count.  One device (o->device_id; o->gpu_num is
 * not used) or host threads.  c0 == c1: zeros.  c0 > c1 or c1 beyond the
 * plan's chunks: SUP_EINVAL; the other checks and st as
 * sup_perman_complex_exact's (gray_steps = (c1 - c0) 2^(lane_bits +
 * walk_bits)). */
int sup_perman_complex_exact_range(const double* mat, int n, uint64_t c0, uint64_t c1, const sup_opts* o,
                                   int on_cpu, int group, uint64_t* primes, uint64_t* res_re, uint64_t* res_im,
                                   int cap, int* nprimes, sup_stats* st);

/* Many complex permanents in one call (ABI 12): boson-sampling simulators
 * evaluate 10^4..10^7 permanents of n x n submatrices (n ~ 8..28) of one
 * unitary per run, and one matrix of order n < 26 leaves most of an MI355X
 * idle (one wave at n <= 13, 128 waves at n = 20).
 * count permanents of n x n complex matrices: mats = count * 2 n^2 doubles
 * (matrix k at mats + k*2*n*n, row-major interleaved re, im); out = 2*count
 * doubles (re, im per matrix).
 * Result k is bit-identical to sup_perman_complex of matrix k alone with the
 * same o->walk_log2 — on the GPU, on any device count, on host threads and for
 * any slab size: every matrix keeps its layout, chunk enumeration, operation
 * order and the pairwise tree over its own chunk partials.
 * n <= 32 on the device: slabs of matrices, each slab three launches (tables
 * and start vectors written on the device, the batched walk walk_cplxb.hip
 * over the wave-chunks of all its matrices in one queue, the per-matrix fold)
 * and one download.  A slab holds as many matrices as keep its tables and
 * partials under 256 MiB; the environment variable
 * SUP_CPLX_BATCH_SLAB=<matrices> overrides that (tests).  n in 33..64: the
 * matrices one after another through sup_perman_complex's walk.
 * o->gpu_num devices from o->device_id take contiguous ranges of matrices
 * (fewer matrices than devices: fewer devices); on_cpu = 1 runs the host twin
 * on o->threads threads.  count == 0: SUP_OK, nothing written.  A null
 * pointer, n outside [1, 64] or o->walk_log2 outside [0, 31]: SUP_EINVAL.
 * Non-finite input propagates into its own result only.  No device with
 * on_cpu = 0: SUP_ENODEV (no silent CPU fallback).
 * st: kernel_ms (max over devices of the summed prepare, walk and fold kernel
 * time), wall_ms, leaves = count, gray_steps = count 2^(n-1), devices_used,
 * lane_bits, walk_bits, grid (last launch on the first device),
 * est_ops_per_step = 6n. */
int sup_perman_complex_batch(const double* mats, int n, uint64_t count, const sup_opts* o,
                             int on_cpu, double* out, sup_stats* st);
/* count permanents of n x n submatrices of one R x C complex matrix U
 * (row-major interleaved): matrix k has entry (j, c) =
 * U[rows[k*n + j]][cols[k*n + c]]; indices may repeat (photon collisions).
 * On the device U goes up once and the gather happens where the tables are
 * written: no submatrix is materialised.  Everything else as
 * sup_perman_complex_batch (result k = sup_perman_complex of the gathered
 * matrix, bit for bit).  R or C < 1, or an index outside [0, R) / [0, C):
 * SUP_EINVAL — the message names k, the position and the value — before any
 * device work. */
int sup_perman_complex_submatrices(const double* U, int R, int C, const int32_t* rows,
                                   const int32_t* cols, int n, uint64_t count, const sup_opts* o,
                                   int on_cpu, double* out, sup_stats* st);

/* Collision-aware form of sup_perman_complex_submatrices (ABI 14): the same
 * arguments, index checks and errors (it drops in where that call is used),
 * but equal indices are not only gathered.  Equal indices on one side make
 * equal columns (rows) of the gathered matrix A, and subsets that take the
 * same number of copies from every group give the same term: with distinct
 * columns b_k of multiplicities t_k (order of first appearance), one copy of
 * the rarest group held (the first on a tie; t'_k = t_k - 1 there, t_k else),
 *   per(A) = 2 sum_{0 <= v_k <= t'_k} (-1)^(sum v) prod_k C(t'_k, v_k) prod_j x_j(v),
 *   x_j(v) = 1/2 sum_k (t_k - 2 v_k) b_k[j],
 * T = prod (t'_k + 1) terms instead of 2^(n-1) (n = 24 with six groups of
 * four: 12,500 instead of 8.4 million).  The side with the smaller T is
 * collapsed (columns on a tie, the rows through the transposed gather); the
 * other side stays expanded.  Without repeats T = 2^(n-1).
 * Result k equals the permanent of gathered matrix k but does NOT have
 * sup_perman_complex's (so sup_perman_complex_submatrices') bits: the sum, its
 * order and its scale differ.  It is a function of (U, rows[k], cols[k]) only:
 * bit-identical on the GPU (per slab three launches: tables and start
 * vectors written on the device from U and the lists, walk_cplxf.hip over one
 * queue of the wave-chunks of all its matrices, a per-matrix fold; the
 * grouping is host work on o->threads threads), on any device count, for any
 * slab size (256 MiB of tables and partials; the environment variable
 * SUP_CPLX_FOCK_SLAB=<matrices> overrides it, for tests) and on o->threads
 * host threads (on_cpu = 1).  o->gpu_num devices from o->device_id take
 * contiguous ranges of matrices.  o->walk_log2 is checked as the submatrix
 * entry checks it and otherwise unused: the layout is a function of the
 * collapsed side's multiplicities alone.  A matrix with more
 * than 2^24 wave-chunks (T above about 2^40): SUP_EUNSUPPORTED before any
 * work.  No device with on_cpu = 0: SUP_ENODEV (no silent CPU fallback).
 * st: leaves = count, gray_steps = count 2^(n-1) (nominal), visited_steps =
 * sum_k T_k, kernel_ms (max over devices of the summed prepare, walk and fold
 * kernel time), wall_ms, devices_used, grid, est_ops_per_step = 6n (per visited
 * step: 2n column adds, 4(n-1) for the product, 4 for acc += w term). */
int sup_perman_complex_fock(const double* U, int R, int C, const int32_t* rows,
                            const int32_t* cols, int n, uint64_t count, const sup_opts* o,
                            int on_cpu, double* out, sup_stats* st);
/* What sup_perman_complex_fock would do with these lists, host only (no
 * device): per matrix the terms T (terms[k]) and the side collapsed (side[k]:
 * 0 columns, 1 rows).  Either output may be NULL.  Null lists or n outside
 * [1, 64]: SUP_EINVAL.  Indices are only compared, not range-checked. */
int sup_perman_complex_fock_plan(const int32_t* rows, const int32_t* cols, int n,
                                 uint64_t count, uint64_t* terms, int* side);

/* One-walk permanent minors (ABI 15).  B is n x (n-1) complex; "minor j" is B
 * without row j, (n-1) x (n-1).  The exact boson sampler (sup_boson_sample)
 * needs, per stage, the permanents of all n minors of one matrix, and they are
 * the gradient of a permanent with respect to a row.  n calls of
 * sup_perman_complex walk the same 2^(n-3) Gray states with the same row sums
 * n times; here all n fall out of one walk: with q = n - 1, the
 * layout and enumeration of order q (o->walk_log2 honoured; engine bit e =
 * column e, column q - 1 held) and the Nijenhuis-Wilf vector over all n rows,
 *   x_i(S) = b_i,q-1 - 1/2 sum_c b_ic + sum_{e in S} b_ie
 *   per(minor j) = (4(q&1) - 2) sum_S (-1)^|S| prod_{i != j} x_i(S),
 * every state's n products formed from prefix and suffix products (cxm.hpp):
 * 16n - 24 fp64 operations per Gray step for n results, against n (6(n-1) - 2).
 * count x n minors: matrix k is B[j][c] = U[rows[k*n + j]][cols[k*(n-1) + c]]
 * (n rows, n-1 columns, indices may repeat; never materialised on the device);
 * out[2*(k*n + j)], [.. + 1] = per(B without row j).
 * n = 1: the one minor is the empty matrix, 1 + 0i, no device work (cols may
 * be NULL only here).  n <= 32: the one walk (walk_cplxm.hip).  Result (k, j)
 * is then a function of (gathered B, o->walk_log2) only: bit-identical on the
 * GPU, for any device count and slab size, and on any number of host threads
 * (on_cpu = 1); it does NOT have sup_perman_complex's bits on the materialised
 * minor (the product order differs).  n in 33..64: every minor materialised
 * and run through sup_perman_complex's walk, on the device or the host as
 * on_cpu says, with that entry's bits.
 * Everything else as sup_perman_complex_submatrices: the same index checks and
 * messages (k, the position and the value) before any device work, count == 0
 * is SUP_OK, a null pointer or o->walk_log2 outside [0, 31] SUP_EINVAL, no
 * device with on_cpu = 0 SUP_ENODEV (no silent CPU fallback), NaN stays inside
 * its own matrix, o->gpu_num devices take contiguous ranges of matrices, slabs
 * of 256 MiB (three launches and one download each) with the environment
 * variable SUP_CPLX_MINORS_SLAB=<matrices> as the test override.
 * st: as the batch entry's with leaves = count n, gray_steps = count 2^(n-2),
 * est_ops_per_step = 16n - 24. */
int sup_perman_complex_minors(const double* U, int R, int C, const int32_t* rows, const int32_t* cols,
                              int n, uint64_t count, const sup_opts* o, int on_cpu, double* out, sup_stats* st);
/* One raw n x (n-1) matrix (row-major interleaved), wave-chunks [c0, c1) of the
 * order-(n-1) plan, per output the pairwise tree over c - c0, NOT scaled by
 * 4((n-1)&1) - 2: out = 2n doubles.  Aligned power-of-two ranges folded
 * pairwise in order, then scaled, reproduce sup_perman_complex_minors' bits.
 * n outside [2, 32]: SUP_EUNSUPPORTED.  Errors and st otherwise as
 * sup_perman_complex_range (est_ops_per_step = 16n - 24). */
int sup_perman_complex_minors_range(const double* mat, int n, uint64_t c0, uint64_t c1, const sup_opts* o,
                                    int on_cpu, double* out, sup_stats* st);
/* nsamples exact boson-sampling outcomes (Clifford & Clifford 2018, algorithm
 * A): n photons enter the M x M unitary U (row-major interleaved) in the
 * distinct modes inputs[0..n); out = nsamples x n output modes, ascending per
 * sample (a mode repeats where photons collide).  Stage k = 1..n is one
 * sup_perman_complex_minors call of order parameter k over all samples (on
 * U^T, rows = the first k of the sample's permuted inputs alpha, cols = its
 * k - 1 modes drawn so far), then on o->threads host threads the weights
 *   w_i = |sum_l U[i][alpha_l] minor_l|^2, i < M,
 * and the draw, for both on_cpu values: the device and the host twin draw
 * identical samples, and sample s depends on (U, inputs, seed, s) only, not on
 * nsamples, threads, devices or slab size.
 * Randomness: Philox4x32-10 with counter (s, step) keyed by seed; w64 = word 0
 * | word 1 << 32 of that draw.  Shuffle: alpha starts as inputs; for t = 0 ..
 * n-2, i = n-1-t: swap(alpha[i], alpha[floor(w64(step t) (i+1) / 2^64)]).
 * Stage k: u = (w64(step 64 + k) >> 11) 2^-53; r_k = the first i whose running
 * sum of w (ascending) exceeds u sum(w); an i with w_i = 0 is never chosen.
 * n in [1, 32] (larger: SUP_EUNSUPPORTED); M >= 1 and inputs in [0, M), else
 * SUP_EINVAL; a repeated input mode is SUP_EINVAL (the message names the
 * position): the algorithm's marginals need orthonormal columns; likewise the
 * n used columns A of U must satisfy |A^dagger A - I| <= 1e-8 entrywise.
 * nsamples == 0: SUP_OK.  No device with on_cpu = 0: SUP_ENODEV.
 * st: kernel_ms (summed over the stages), wall_ms, leaves = nsamples,
 * gray_steps = nsamples sum_k 2^(k-2), devices_used, est_ops_per_step =
 * 16n - 24, partials[0] / [1] = wall ms in the minors calls / in the host pmf
 * stage. */
int sup_boson_sample(const double* U, int M, const int32_t* inputs, int n, uint64_t nsamples, uint64_t seed,
                     const sup_opts* o, int on_cpu, int32_t* out /* nsamples x n, ascending modes */, sup_stats* st);

/* Collision-aware form of sup_perman_complex_minors (ABI 17): the same
 * arguments, index checks, messages, count == 0, null-pointer and SUP_ENODEV
 * behaviour, but the repeated columns of B are collapsed as
 * sup_perman_complex_fock collapses them.  B[i][c] =
 * U[rows[k*n + i]][cols[k*(n-1) + c]]; with the distinct columns b_k (vectors
 * over all n rows) of multiplicities t_k (order of first appearance, sum
 * n - 1), one copy of the rarest group held (the first on a tie; t'_k =
 * t_k - 1 there, t_k else),
 *   x_i(v) = 1/2 sum_k (t_k - 2 v_k) b_k[i]
 *   per(B without row j) = 2 sum_{0 <= v_k <= t'_k} (-1)^(sum v) prod_k C(t'_k, v_k) prod_{i != j} x_i(v),
 * T = prod (t'_k + 1) terms instead of 2^(n-2), and since x_i(v) depends on row
 * i only, one walk serves all n minors: 16n - 20 fp64 operations per walked
 * state.  Only the column side is collapsed; repeated rows are only gathered.
 * The layout is sup_perman_complex_fock's rule on the column multiplicities.
 * n in [1, 32] (larger: SUP_EUNSUPPORTED; n < 1: SUP_EINVAL); n = 1: the one
 * minor is 1 + 0i, no device work (cols may be NULL only here).
 * Result (k, j) is a function of (U, rows[k], cols[k]) only: bit-identical on
 * the GPU (per slab three launches and one download: tables and start vectors
 * written on the device, walk_cplxfm.hip over one queue of the wave-chunks of
 * all its matrices, a fold per output), on any device count, for any slab size
 * (256 MiB; the environment variable SUP_CPLX_FOCK_MINORS_SLAB=<matrices>
 * overrides it, for tests) and on o->threads host threads (on_cpu = 1).  It
 * does NOT have sup_perman_complex_minors' bits.  o->gpu_num devices from
 * o->device_id take contiguous ranges of matrices; o->walk_log2 is checked and
 * otherwise unused.
 * st: leaves = count n, gray_steps = count 2^(n-2) (nominal; 0 at n = 1),
 * visited_steps = sum_k T_k (0 at n = 1: nothing is walked), kernel_ms,
 * wall_ms, devices_used, grid, est_ops_per_step = 16n - 20. */
int sup_perman_complex_fock_minors(const double* U, int R, int C, const int32_t* rows, const int32_t* cols,
                                   int n, uint64_t count, const sup_opts* o, int on_cpu, double* out,
                                   sup_stats* st);
/* The terms T of that sum per matrix, host only: cols = count x (n-1) (indices
 * only compared, not range-checked), terms[k] = T_k (1 at n = 1 and n = 2).
 * n < 1, null terms, or null cols with n != 1: SUP_EINVAL; n > 32:
 * SUP_EUNSUPPORTED. */
int sup_perman_complex_fock_minors_plan(const int32_t* cols, int n, uint64_t count, uint64_t* terms);
/* sup_boson_sample with every stage's minors from
 * sup_perman_complex_fock_minors: the same arguments, checks, randomness, pmf
 * stage and stats, except that visited_steps is the sum over the stages of
 * that entry's (gray_steps stays the nominal nsamples sum_k 2^(k-2)) and
 * est_ops_per_step = 16n - 20.  The weights differ from sup_boson_sample's in
 * their last bits only, so a draw can differ only where u sum(w) lies within
 * rounding of a running sum.  The device and the host twin draw identical
 * samples, and sample s depends on (U, inputs, seed, s) only. */
int sup_boson_sample_fock(const double* U, int M, const int32_t* inputs, int n, uint64_t nsamples, uint64_t seed,
                          const sup_opts* o, int on_cpu, int32_t* out /* nsamples x n, ascending modes */,
                          sup_stats* st);

/* Hafnians and loop hafnians with repeats (ABI 20): the amplitudes of Gaussian
 * boson sampling.  A is M x M complex (row-major, interleaved re, im) and
 * symmetric bit for bit; matrix k is the n x n gather A[idx[k n + i]][idx[k n
 * + j]], 1 <= n <= 64, the list may repeat (one index per detected photon).
 * With the K distinct values of the list (multiplicities s_k, order of first
 * appearance; two copies of one value may pair: the diagonal of A counts), one
 * copy of the rarest group held (s'_k) and h_k = s_k / 2 - v_k,
 *   haf = 2 / (n/2)!  sum_{0 <= v_k <= s'_k} (-1)^(sum v) prod C(s'_k, v_k) (q(v) / 2)^(n/2)
 *   q(v) = sum_kl h_k A_kl h_l
 * has T = prod (s'_k + 1) terms (2^(n-1) without repeats); odd n
 * gives exactly 0 and walks nothing.  The layout (walk digits, Tw, H) is
 * sup_perman_complex_fock's rule on the multiplicity vector.  out[2k],
 * out[2k + 1] = Re, Im of result k: a function of (A, mu, idx[k]) only,
 * bit-identical on the device (walk_haf.hip), on any device count (o->gpu_num
 * devices take contiguous ranges of matrices), for any slab size and on host
 * threads (on_cpu = 1).  It is not bit-identical to a permanent entry on the
 * bipartite embedding.  Without repeats the cost is 2^(n-1) states: the entry
 * is meant for patterns with collisions and for small orders.
 * Errors, all before any device work: a null pointer, n outside [1, 64], an
 * index outside [0, M), a pair A[i][j], A[j][i] that differs: SUP_EINVAL with a
 * message naming the place; a matrix of more than 2^24 wave-chunks:
 * SUP_EUNSUPPORTED; no device with on_cpu = 0: SUP_ENODEV (no CPU fallback).
 * st: leaves = count, gray_steps = count 2^(n-1) (nominal), visited_steps =
 * sum_k T_k, kernel_ms, wall_ms, devices_used, grid, est_ops_per_step = the op
 * census of DESIGN.md 8h (the T-weighted mean over the matrices). */
int sup_hafnian_complex(const double* A, int M, const int32_t* idx, int n, uint64_t count, const sup_opts* o,
                        int on_cpu, double* out, sup_stats* st);
/* The loop hafnian of the same gathers: mu (M complex, interleaved) replaces
 * the diagonal on self-loops, mu_k = mu[idx value k].  With r(v) = sum_k mu_k h_k
 *   lhaf = 2 sum_v (-1)^(sum v) prod C(s'_k, v_k) sum_{j <= n/2} (q/2)^j / j! r^(n-2j) / (n-2j)!
 * for even and odd n.  Arguments, errors, bits and stats as sup_hafnian_complex. */
int sup_loop_hafnian_complex(const double* A, int M, const double* mu, const int32_t* idx, int n, uint64_t count,
                             const sup_opts* o, int on_cpu, double* out, sup_stats* st);
/* The terms T of each matrix's sum, host only (no device).  terms may be NULL.
 * A null list or n outside [1, 64]: SUP_EINVAL.  Indices are only compared. */
int sup_hafnian_complex_plan(const int32_t* idx, int n, uint64_t count, uint64_t* terms);

/* Double-double hafnians and loop hafnians (ABI 29): the gathers, the sum, the
 * layout, the slabs (SUP_HAFNIAN_SLAB) and the split over o->gpu_num devices of
 * sup_hafnian_complex / sup_loop_hafnian_complex, with every running value a
 * complex double-double (~106 bits per part; walk_hafdd.hip): the
 * truth the fp64 hafnian entries are judged against on matrices that are not
 * Gaussian integers.  The inputs are doubles; every weight prod C(s'_k, v_k) is
 * converted from the exact integer, so groups of 58 and more copies keep the
 * full precision.  out[4k .. 4k + 3] = re_hi, re_lo, im_hi, im_lo of result k,
 * each (hi, lo) a normalised pair (hi = fl(hi + lo)); odd n without loop gives
 * four exact zeros and walks nothing.  The error of hi + lo is bounded by a
 * polynomial in n, Tw and K times 2^-103 times the sum of the 1-norms of the
 * weighted terms (DESIGN.md 8q states it; tests/test_hafnian_quad.py asserts
 * it).  A function of (A, mu, idx[k]) only: bit-identical on the device, on any
 * device count, for any slab size and on host threads (on_cpu = 1).
 * Checks, their order, errors and messages as sup_hafnian_complex (SUP_ENODEV
 * without a device, no CPU fallback); n above SUP_HAFNIAN_QUAD_MAX_DEVICE_N,
 * the largest order the device kernel serves with no scratch, no spilled VGPR
 * and two waves per SIMD, with on_cpu = 0: SUP_EUNSUPPORTED on any machine,
 * before the device is looked for (host threads serve n <= 64).
 * st as sup_hafnian_complex's, with est_ops_per_step = the T-weighted mean of
 *   hafdd_ops(W, n, loop) = 116 + g + 68 (floor(log2 m) + popcount(m) - 1)      plain, m = n / 2
 *                         = 202 + g + (m ? 190 m - 68 : 0) + (n odd ? 68 : 0)   loop
 * g = 72 for W <= 4 walk digits, else 180, in dd.hpp's nominal counts (dd_add
 * 20, dd_add_d 9, dd_mul 7, cxdd_mul 68, cxdd_add 40). */
#define SUP_HAFNIAN_QUAD_MAX_DEVICE_N 64
int sup_hafnian_complex_quad(const double* A, int M, const int32_t* idx, int n, uint64_t count, const sup_opts* o,
                             int on_cpu, double* out /* 4 per matrix */, sup_stats* st);
int sup_loop_hafnian_complex_quad(const double* A, int M, const double* mu, const int32_t* idx, int n, uint64_t count,
                                  const sup_opts* o, int on_cpu, double* out /* 4 per matrix */, sup_stats* st);

/* Ragged loop hafnians with a displacement per item (ABI 26): the batch one
 * chain-rule step of a PNR Gaussian boson sampler needs.  A as above; mu holds
 * nmu rows of M complex; item k, k < count, is the loop hafnian of the gather of
 * A by idx[k stride .. k stride + n[k]) with row mu_of[k] of mu on the diagonal
 * (mu_of NULL: row k), 0 <= n[k] <= 64 and stride >= max n[k] (entries past
 * n[k] are not read).  Item k with n[k] >= 1 has the bits of
 * sup_loop_hafnian_complex(A, M, mu + 2 M mu_of[k], idx + stride k, n[k], 1, ..);
 * an item with n[k] = 0 is exactly 1 + 0i and walks nothing.  The whole call
 * is one slab queue (slabs as sup_hafnian_complex; SUP_HAFNIAN_SLAB): items of
 * different order sit next to each other in the wave-chunk queue, and the
 * kernel (walk_lhafe.hip) reads the order, the Horner bound and the
 * coefficient row per matrix.  Bit-identical on the device, on
 * any device count, for any slab size and queue group and on host threads.
 * Errors, all before any device work: a null pointer (mu_of alone may be NULL),
 * M < 1, a pair A[i][j], A[j][i] that differs, n[k] outside [0, 64], stride <
 * n[k], mu_of[k] (or k) outside [0, nmu), an index outside [0, M): SUP_EINVAL
 * with a message naming the place; an item of more than 2^24 wave-chunks:
 * SUP_EUNSUPPORTED; no device with on_cpu = 0: SUP_ENODEV (no CPU fallback).
 * st: leaves = count, gray_steps = sum_k 2^(n[k]-1) (nominal, saturating),
 * visited_steps = sum_k T_k, kernel_ms, wall_ms, devices_used, grid,
 * est_ops_per_step = the T-weighted census of DESIGN.md 8h over the items. */
int sup_loop_hafnian_complex_each(const double* A, int M,
                                  const double* mu, uint64_t nmu, /* nmu x M complex rows            */
                                  const int32_t* mu_of,           /* count; NULL: item k uses row k  */
                                  const int32_t* idx, int stride, /* count x stride, first n[k] used */
                                  const int32_t* n,               /* count, each in [0, 64]          */
                                  uint64_t count, const sup_opts* o, int on_cpu, double* out, sup_stats* st);
/* A photon-number-resolving Gaussian boson sampler for pure states (ABI 26):
 * the chain rule of Bulmer et al. 2022 on the entry above (gbs.cpp, DESIGN.md
 * 8n).  B (M x M complex, symmetric bit for bit) and zeta[s] (M complex per
 * sample) describe the state: <n|psi> is proportional to lhaf(B gathered with
 * n_i copies of i, zeta on the diagonal) / sqrt(prod n_i!).  het[s] holds the
 * heterodyne outcomes alpha_0 .. alpha_{M-1} of sample s, drawn by the caller
 * from N(mean, V + (hbar/2) I): this entry draws nothing Gaussian and is
 * deterministic.  For mode k = 0 .. M-1 of sample s
 *   z_i = zeta_i + sum_{j > k} B_ij conj(alpha_j), i <= k   (j ascending, fma per part)
 *   w_c = |lhaf(B; the outcomes so far, then c copies of k; z)|^2 / c!,  c <= cutoff
 *   u   = (w64(seed, sample0 + s, step k) >> 11) 2^-53      (sup_boson_sample's w64)
 *   n_k = the first c whose running sum of w exceeds u sum(w); a zero weight
 *         is never chosen
 * and every step is one sup_loop_hafnian_complex_each call per batch of
 * samples.  A candidate whose order would exceed 64 has weight 0.  When the
 * weights of a sample sum to zero or to a non-finite value, that mode and every
 * later one are -1.  Renormalising over c <= cutoff is the only approximation:
 * the law is exact as cutoff grows.  Sample s depends on (B, zeta[s], het[s],
 * cutoff, seed, sample0 + s) only; the device and on_cpu = 1 draw identical
 * samples.
 * Errors: null B, M outside [1, 64], cutoff outside [0, 64], B not symmetric:
 * SUP_EINVAL; then nsamples = 0 returns SUP_OK; a null zeta, het or out:
 * SUP_EINVAL; no device with on_cpu = 0: SUP_ENODEV.
 * st: leaves = nsamples, visited_steps = gray_steps = the sum of the calls'
 * visited_steps, kernel_ms summed over the steps, est_ops_per_step (T-weighted
 * over all calls), partials[0] / [1] = wall ms in the each-calls / in the host
 * stage, partials[2] = samples that ended in -1. */
int sup_gbs_sample(const double* B, int M,
                   const double* zeta, const double* het, /* nsamples x M complex each */
                   int cutoff, uint64_t nsamples, uint64_t sample0, uint64_t seed,
                   const sup_opts* o, int on_cpu, int32_t* out /* nsamples x M */, sup_stats* st);

/* Loop-hafnian tables (ABI 27): every Fock amplitude up to a cutoff from one
 * recurrence instead of one walk per pattern (lhaftab.hip, lhaf_table.cpp,
 * lhaftab.hpp).  A is M x M complex, symmetric bit for bit, its
 * diagonal counting pairs of copies of one mode; mu holds M complex loop
 * weights on self-loops only (sup_loop_hafnian_complex's convention), NULL
 * meaning zero: the plain hafnian table, whose entries of odd photon total are
 * zero.  dims[i] = d_i in [1, 65] and n_i in [0, d_i).  With
 *   t(n) = lhaf(A gathered with n_i copies of i, mu) / sqrt(prod n_i!)
 * out holds t as (re, im) pairs at index x = sum_i n_i prod_{k<i} d_k (mode 0
 * fastest): 2 prod d_i doubles.  out[0] = 1 + 0i exactly.  For x > 0, with p the
 * highest occupied mode and m = n - e_p,
 *   t(n) = [ mu_p t(m) + sum_{j <= p, m_j > 0} sqrt(m_j) A_pj t(m - e_j) ] / sqrt(n_p)
 * j ascending, every complex multiply-add one fixed sequence of fmas per part,
 * sqrt(k) and 1 / sqrt(k) from two host-made tables (lhaftab.hpp states each
 * operation).  Row p of A is read up to column p.  An entry is a function of
 * earlier entries only, so the device (one kernel for the prefix that fits a
 * work-group's LDS, then one launch per slab n_p = c of each further mode p) and
 * on_cpu = 1 (host threads, slab by slab) give the same bits, whatever the
 * launch shape or thread count; a non-finite value reaches exactly the entries
 * whose recurrence reads it.  SUP_LHAF_TABLE_LOW=E (read per call, 1 <= E <=
 * 4096) makes the first kernel take at most E entries; the bits do not change.
 * Errors, all before any device work: null A, dims or out, M outside [1, 64], a
 * d_i outside [1, 65], an asymmetric pair, o->gpu_num > 1 (a table is one
 * device's: o->device_id), a bad SUP_LHAF_TABLE_LOW: SUP_EINVAL; prod d_i above
 * SUP_LHAF_TABLE_MAX_ENTRIES on either path: SUP_EUNSUPPORTED; no device with
 * on_cpu = 0: SUP_ENODEV (no CPU fallback).  A table above 256 MiB is given
 * back to the device after the call.
 * st: leaves = 1, gray_steps = visited_steps = prod d_i, kernel_ms, grid = the
 * work-groups of the largest launch, devices_used = 1 (0 with on_cpu),
 * est_ops_per_step = the fp64 operations per entry (an fma counts once; the
 * plan entry's figure), partials[0] = the kernel launches. */
#define SUP_LHAF_TABLE_MAX_ENTRIES (1ull << 27)   /* 2 GiB of complex results, as ABI 25's cap */
int sup_loop_hafnian_table(const double* A, int M, const double* mu /* NULL: hafnian table */,
                           const int32_t* dims, const sup_opts* o, int on_cpu,
                           double* out /* 2 * prod dims */, sup_stats* st);
/* Host only: prod d_i (saturating at 2^64 - 1), the kernel launches of the
 * device path (under SUP_LHAF_TABLE_LOW as set) and the operations per entry
 * (0 when the product saturated).  Any output may be NULL.  Errors: null dims,
 * M outside [1, 64], a d_i outside [1, 65], a bad SUP_LHAF_TABLE_LOW: SUP_EINVAL. */
int sup_loop_hafnian_table_plan(const int32_t* dims, int M, uint64_t* entries, uint64_t* launches,
                                double* ops_per_entry);

/* Exact hafnians and loop hafnians of Gaussian-integer matrices (ABI 23): the
 * integer truth the floating hafnian entries are judged against, and exact
 * counts of (weighted) perfect matchings.  A, idx, n, count and the gathers as
 * sup_hafnian_complex; mu NULL: the plain hafnian, else the loop hafnian.
 * Every part of A and mu must be an integer with |part| < 2^31.  With the
 * integers H_k = s_k - 2 v_k, q' = H^T Abar H, r' = mubar . H, m = floor(n/2),
 *   T = sum_v (-1)^(sum v) prod C(s'_k, v_k) q'^m               haf  = 2 T / (m! 8^m)
 *   L = sum_v (...) sum_{j <= m} c_j q'^j r'^(n-2j)              lhaf = 2 L / (n! 2^(n+m))
 *   c_j = n! / (j! (n-2j)!) 2^(m-j)
 * over the same multiplicity vectors, layout and Gray order as
 * sup_hafnian_complex.  q', r' and the step are exact in fp64;
 * the power, the polynomial and every weight are formed in (Z/p)[i] for primes
 * p < 2^25 (residue times residue: 2.25 p^2 < 2^52, hafexact.hpp), taken until
 * their product exceeds 8 times the bound 2^(n-1) R^m (plain) or 2^(n-1) sum_j
 * c_j R^j R_mu^(n-2j) (loop), R, R_mu = the sums of |Re| + |Im| over the
 * gathered matrix and mu (the largest over the call's matrices).  The residues
 * of Re and Im are joined separately by CRT; 2T must be divisible by m! 8^m
 * and 2L by n! 2^(n+m): a built-in self-check (a failure is SUP_EHIP with a
 * message, never a wrong number).  Plain form, odd n: "0", "0", nothing walked.
 * The device walk (walk_hafexact.hip) serves every n <= 64, kHafxPrimes primes
 * per launch (hafexact.hpp; more primes take more launches over the same tables);
 * on_cpu = 1 runs the same residue operations on o->threads host threads, and
 * the two agree residue for residue.  o->gpu_num devices take contiguous
 * ranges of matrices.
 * Result k: signed decimal integers, NUL-terminated, at out_re + k out_len and
 * out_im + k out_len; a buffer too short for a result is SUP_EINVAL with the
 * length needed in the message (768 bytes always suffice).
 * Errors, all before any device work and in this order: a null pointer, n
 * outside [1, 64], M < 1, a pair A[i][j], A[j][i] that differs, an index
 * outside [0, M), a part of A or mu that is not an integer or has |part| >=
 * 2^31: SUP_EINVAL with a message naming the place (row, column, part); a
 * matrix of more than 2^24 wave-chunks: SUP_EUNSUPPORTED; no device with
 * on_cpu = 0: SUP_ENODEV (no CPU fallback).
 * st: leaves = count, gray_steps = count 2^(n-1) (nominal), visited_steps =
 * sum_k T_k, kernel_ms, wall_ms, devices_used, grid, seg_cached_bits = the
 * primes of the call, seg_pair_bits = the walk launches of a slab,
 * est_ops_per_step = the census hafx_ops (fp64 instructions per
 * state and lane summed over the launches, T-weighted mean over the matrices). */
int sup_hafnian_complex_exact(const double* A, int M, const double* mu /* NULL: plain hafnian */, const int32_t* idx,
                              int n, uint64_t count, const sup_opts* o, int on_cpu, char* out_re, char* out_im,
                              size_t out_len /* per matrix */, sup_stats* st);

/* Power-trace hafnians and loop hafnians (ABI 21): the same gathers and the
 * same mathematical values as sup_hafnian_complex / sup_loop_hafnian_complex by
 * a second, independent algorithm (Bjorklund, Gupt, Quesada) whose cost does
 * not depend on repeats: with n' = n + (n odd, loop form: one virtual index
 * with a zero row and column and mu = 1), m = n' / 2, the sum runs over the
 * non-empty subsets z of the m index pairs (2i, 2i + 1),
 *   haf = sum_{z in [1, 2^m)} (-1)^(m - |z|) f(z),   f(z) = g_m,
 *   g_0 = 1,  g_s = (1 / s) sum_{j=1..s} (j c_j) g_(s-j),
 *   c_j = tr (N_z X)^j / (2j) + (d_z X (N_z X)^(j-1) d_z) / 2
 * (N_z: the rows and columns of the pairs of z, X: the pair swap, d = mu on
 * the list, the second term in the loop form only); 2^(n/2) subsets of
 * n^3-sized work instead of 2^(n-1) states (the order of every
 * operation is superman_amd/csrc/hafpt.hpp's).  Odd n in the plain form gives
 * exactly 0 and visits nothing.  out[2k], out[2k + 1] = Re, Im of result k: a
 * function of (A, mu, idx[k]) only, bit-identical on the device
 * (walk_hafpt.hip), on any device count (o->gpu_num devices take contiguous
 * ranges of matrices), for any queue group and on host threads (on_cpu = 1).
 * It is NOT bit-identical to sup_hafnian_complex: the two check each other to
 * rounding.
 * Errors, all before any device work: a null pointer, n outside [1, 64], an
 * index outside [0, M), a pair A[i][j], A[j][i] that differs: SUP_EINVAL with a
 * message naming the place; on_cpu = 0 and n above
 * SUP_HAFNIAN_PT_MAX_DEVICE_N: SUP_EUNSUPPORTED (on any machine; host threads
 * serve every n <= 64); no device with on_cpu = 0: SUP_ENODEV (no CPU
 * fallback).  The cap is the largest order whose kernel uses no scratch memory
 * and whose LDS tile (n'^2 + 163 complex values) fits one 64 KiB workgroup
 * allocation, two of which share a compute unit.
 * st: leaves = count, gray_steps = count 2^(n-1) (nominal, as the Kan
 * entries'), visited_steps = the subsets visited, kernel_ms, wall_ms,
 * devices_used, grid, est_ops_per_step = fp64 operations per subset (the
 * census hafpt_ops(m, loop) of DESIGN.md 8i, binomial mean over |z|). */
#define SUP_HAFNIAN_PT_MAX_DEVICE_N 62
int sup_hafnian_complex_pt(const double* A, int M, const int32_t* idx, int n, uint64_t count, const sup_opts* o,
                           int on_cpu, double* out, sup_stats* st);
int sup_loop_hafnian_complex_pt(const double* A, int M, const double* mu, const int32_t* idx, int n, uint64_t count,
                                const sup_opts* o, int on_cpu, double* out, sup_stats* st);
/* One matrix (one list of n indices), the subsets z in [max(1, z_begin), z_end)
 * only; mu non-null: the loop form.  A wave-chunk is 2^max(0, m - 18)
 * consecutive z; its partial is the ascending-z sum of the signed f(z) of the
 * range that fall in it, and out[0], out[1] = the fold of the partials of the
 * chunks the range touches, by the pairwise tree over (chunk - first chunk).
 * Ranges cut where such trees meet (aligned power-of-two runs of chunks)
 * added pairwise in order reproduce the whole range's bits, and the whole
 * range [0, 2^m) has the batch entries' bits.  z_begin > z_end or z_end > 2^m:
 * SUP_EINVAL; an empty range, or odd n in the plain form: zeros.  One device
 * (o->device_id) or host threads; the other errors as above.
 * st: visited_steps = the subsets of the range, gray_steps = 2^(n-1). */
int sup_hafnian_complex_pt_range(const double* A, int M, const double* mu_or_null, const int32_t* idx, int n,
                                 uint64_t z_begin, uint64_t z_end, const sup_opts* o, int on_cpu, double* out,
                                 sup_stats* st);
/* The subsets one matrix of order n visits (2^m - 1; 0 for odd n in the plain
 * form) and the census' fp64 operations per subset.  Host only; either output
 * may be NULL.  n outside [1, 64]: SUP_EINVAL. */
int sup_hafnian_complex_pt_plan(int n, int loop, uint64_t* subsets, double* est_ops);

/* Torontonians (ABI 22): the probabilities of click patterns of Gaussian boson
 * sampling with threshold detectors.  O is 2M x 2M complex Hermitian, row-major
 * pairs, in thewalrus' ordering (row i: mode i, row i + M: its conjugate
 * partner).  Only its lower triangle and the real parts of its diagonal are
 * read, as LAPACK does: a matrix that is Hermitian only to rounding is not
 * refused.  A list of n DISTINCT modes s selects the 2n rows and columns {s_b,
 * s_b + M}; bit b of z in [0, 2^n) selects list position b:
 *   tor(O, s) = sum_z (-1)^(n - |z|) f(z),  f(z) = 1 / sqrt det(I - O_z),  f(0) = 1
 * with O_z the principal submatrix of the selected positions; f(z) is the
 * product of the reciprocal pivots of a Cholesky factorisation whose row order
 * and operation order superman_amd/csrc/tor.hpp fixes, so that
 * subsets sharing their high bits share the leading rows of the factor.
 * modes: count lists of n (int32); out: count doubles (the result is real).
 * out[k] is a function of (O, modes[k]) only, bit-identical on the device
 * (walk_tor.hip), on any device count (o->gpu_num devices take contiguous
 * ranges of lists), for any queue group and on host threads (on_cpu = 1).
 * A pivot that is not positive (I - O_z not positive definite) is no error
 * code: that list's result is NaN.
 * Errors, all before any device work: a null pointer, n outside [1, 32], a
 * mode outside [0, M), a mode named twice in a list: SUP_EINVAL with a message
 * naming the place; on_cpu = 0 and n above SUP_TORONTONIAN_MAX_DEVICE_N:
 * SUP_EUNSUPPORTED (the cap is 32: every n the entry takes); no device with
 * on_cpu = 0: SUP_ENODEV (no CPU fallback).
 * st: leaves = count, gray_steps = count 2^n, visited_steps = the subsets
 * visited, kernel_ms, wall_ms, devices_used, grid, est_ops_per_step = fp64
 * operations per subset (the census tor_ops(n) of DESIGN.md 8j). */
#define SUP_TORONTONIAN_MAX_DEVICE_N 32
int sup_torontonian(const double* O, int M, const int32_t* modes, int n, uint64_t count, const sup_opts* o, int on_cpu,
                    double* out, sup_stats* st);
/* One list, the subsets z in [z_begin, z_end) only.  A wave-chunk is
 * 2^max(6, min(n, 9), n - 15) consecutive z; its partial adds its 64-aligned
 * groups of signed f(z) in ascending order, and out[0] = the fold of the
 * partials of the chunks the range touches, by the pairwise tree over (chunk -
 * first chunk).  Ranges cut where such trees meet (aligned power-of-two runs
 * of chunks) added pairwise in order reproduce the whole range's bits, and the
 * whole range [0, 2^n) has sup_torontonian's bits; a cut inside a chunk agrees
 * to rounding only.  z_begin > z_end or z_end > 2^n: SUP_EINVAL; an empty
 * range: zero.  One device (o->device_id) or host threads; the other errors as
 * above.  st: visited_steps = the subsets of the range, gray_steps = 2^n. */
int sup_torontonian_range(const double* O, int M, const int32_t* modes, int n, uint64_t z_begin, uint64_t z_end,
                          const sup_opts* o, int on_cpu, double* out, sup_stats* st);
/* The subsets one list of n modes visits (2^n) and the census' fp64 operations
 * per subset.  Host only; either output may be NULL.  n outside [1, 32]:
 * SUP_EINVAL. */
int sup_torontonian_plan(int n, uint64_t* subsets, double* est_ops);

/* Loop torontonians (ABI 24): click patterns of DISPLACED Gaussian states on
 * threshold detectors (thewalrus' ltor).  O, M, modes, n and z are the
 * torontonian's; gamma is any complex vector of length 2M (interleaved pairs;
 * entry i: mode i, entry i + M: its partner), gathered with the same rows:
 *   ltor(O, gamma, s) = sum_z (-1)^(n - |z|) f(z),
 *   f(z) = exp(1/2 gamma_z^H (I - O_z)^-1 gamma_z) / sqrt det(I - O_z),  f(0) = 1
 * The quadratic form is the diagonal chain of one more row of the
 * torontonian's factor, and the exponential is built from fma, multiply, rint
 * and exponent-field arithmetic only (superman_amd/csrc/ltor.hpp, DESIGN.md
 * 8l): out[k] is a function of (O, gamma, modes[k]) only, bit-identical on the
 * device (walk_ltor.hip), on any device count, for any queue group and on host
 * threads (on_cpu = 1).  gamma = 0 gives sup_torontonian's bits.  A pivot that
 * is not positive gives NaN, an exponent beyond the fp64 range inf or NaN:
 * neither is an error code.
 * Errors and st as sup_torontonian's, with a null gamma among the null
 * pointers; the cap is SUP_LOOP_TORONTONIAN_MAX_DEVICE_N; est_ops_per_step =
 * the census ltor_ops(n). */
#define SUP_LOOP_TORONTONIAN_MAX_DEVICE_N 32
int sup_loop_torontonian(const double* O, int M, const double* gamma, const int32_t* modes, int n, uint64_t count,
                         const sup_opts* o, int on_cpu, double* out, sup_stats* st);
/* One list, the subsets z in [z_begin, z_end) only: sup_torontonian_range's
 * chunks, folds and rules. */
int sup_loop_torontonian_range(const double* O, int M, const double* gamma, const int32_t* modes, int n,
                               uint64_t z_begin, uint64_t z_end, const sup_opts* o, int on_cpu, double* out,
                               sup_stats* st);
/* The subsets one list of n modes visits (2^n) and the census' fp64 operations
 * per subset.  Host only; either output may be NULL.  n outside [1, 32]:
 * SUP_EINVAL. */
int sup_loop_torontonian_plan(int n, uint64_t* subsets, double* est_ops);
/* The exponential of the loop torontonian's terms (ltor.hpp ltor_exp), exported
 * for the test harness: on the host, and elementwise on device device_id
 * (out[i] = ltor_exp(x[i]); a null pointer: SUP_EINVAL, no device: SUP_ENODEV;
 * count = 0 does nothing).  The two agree bit for bit. */
double sup_ltor_exp(double x);
int sup_ltor_exp_device(const double* x, uint64_t count, double* out, int device_id);

/* Ragged loop torontonians with a displacement per item (ABI 28): the batch one
 * chain-rule step of a threshold-detector sampler needs.  O as above; gamma
 * holds ngamma rows of 2M complex; item k, k < count, is the loop torontonian
 * of the list modes[k stride .. k stride + n[k]) with row gamma_of[k] of gamma
 * (gamma_of NULL: row k), 0 <= n[k] <= 32 and stride >= max n[k] (entries past
 * n[k] are not read).  Item k with n[k] >= 1 has the bits of
 * sup_loop_torontonian(O, M, gamma + 4 M gamma_of[k], modes + stride k, n[k], 1, ..);
 * an item with n[k] = 0 is exactly 1.0 and walks nothing.  The items of a call
 * share slabs (by bytes, under 2^31 wave-chunks; SUP_LTOR_EACH_SLAB, read per
 * call, caps the items of a slab): items of different order sit next to each
 * other in one wave-chunk queue, and the kernel (walk_ltore, walk_ltor.hip)
 * reads the order, the padded order, the chunk size and the place of the
 * item's matrix per item.  o->gpu_num devices take contiguous
 * ranges of the walking items.  Bit-identical on the device, on any device
 * count, for any slab size and queue group and on host threads.  A pivot that
 * is not positive makes that item NaN and no other.
 * Errors, all before any device work: a null pointer (gamma_of alone may be
 * NULL), M < 1, n[k] outside [0, 32], stride < n[k], gamma_of[k] (or k) outside
 * [0, ngamma), a mode outside [0, M) or named twice in a list, a
 * SUP_LTOR_EACH_SLAB that is no positive integer: SUP_EINVAL with a message
 * naming the place; no device with on_cpu = 0: SUP_ENODEV (no CPU fallback).
 * st: leaves = count, gray_steps = visited_steps = sum_k 2^n[k] over the items
 * with n[k] >= 1, kernel_ms, wall_ms, devices_used, grid, est_ops_per_step =
 * the census ltor_ops(n[k]) weighted by 2^n[k]. */
int sup_loop_torontonian_each(const double* O, int M,
                              const double* gamma, uint64_t ngamma, /* ngamma x 2M complex rows        */
                              const int32_t* gamma_of,              /* count; NULL: item k uses row k  */
                              const int32_t* modes, int stride,     /* count x stride, first n[k] used */
                              const int32_t* n,                     /* count, each in [0, 32]          */
                              uint64_t count, const sup_opts* o, int on_cpu, double* out, sup_stats* st);
/* A threshold-detector Gaussian boson sampler for pure states (ABI 28):
 * sup_gbs_sample's chain rule with click / no-click outcomes on the entry
 * above (threshold_sample.cpp).  B, zeta, het, seed and sample0
 * are sup_gbs_sample's.  One matrix O = [[0, B], [conj B, 0]] serves every step
 * and sample.  For mode k = 0 .. M-1 of sample s, with C the modes below k that
 * clicked, ascending,
 *   z_i = zeta_i + sum_{j > k} B_ij conj(alpha_j), i <= k   (sup_gbs_sample's fmas)
 *   gamma = (z, conj z), zero above k
 *   w_0 = ltor(O, gamma, C),  w_1 = ltor(O, gamma, C + [k])
 *         (a weight that is negative or -0 counts as +0)
 *   u   = (w64(seed, sample0 + s, step k) >> 11) 2^-53
 *   out[s][k] = the first c whose running sum of w exceeds u (w_0 + w_1); a
 *         zero weight is never chosen
 * and every step is one sup_loop_torontonian_each call of two items per sample
 * of a batch.  When w_0 + w_1 is zero or not finite, or the list with k would
 * pass 32 modes, that mode and every later one are -1.  weights (NULL, or
 * nsamples x M x 2 doubles) receives (w_0, w_1) as used, zeros for the modes a
 * failed sample did not reach.  Sample s depends on (B, zeta[s], het[s], seed,
 * sample0 + s) only; the device and on_cpu = 1 draw identical samples.
 * Errors: null B, M outside [1, 64], B not symmetric: SUP_EINVAL; then
 * nsamples = 0 returns SUP_OK; a null zeta, het or out: SUP_EINVAL; no device
 * with on_cpu = 0: SUP_ENODEV.
 * st: as sup_gbs_sample's (kernel_ms summed over the steps, partials[0] / [1] =
 * wall ms in the each-calls / in the host stage, partials[2] = samples that
 * ended in -1). */
int sup_threshold_sample(const double* B, int M,
                         const double* zeta, const double* het, /* nsamples x M complex each */
                         uint64_t nsamples, uint64_t sample0, uint64_t seed,
                         const sup_opts* o, int on_cpu, int32_t* out /* nsamples x M */,
                         double* weights /* NULL or nsamples x M x 2 */, sup_stats* st);

/* Torontonian tables (ABI 25): every click pattern of one list of n distinct
 * modes from one walk.  f(z) depends on the selected positions only, so for
 * every sub-list S of the list tor(O, S) = sum_{Z in S} (-1)^(|S| - |Z|) f(Z):
 * the walk stores raw[z] = f(z) (unsigned, bit b of z = list position b, the
 * bits of sup_torontonian_range(.., z, z + 1) up to its sign) and the subset
 * Moebius transform, in place and bits ascending,
 *   for b = 0 .. n-1: for every z with bit b set: t[z] = t[z] - t[z ^ (1 << b)]
 * (one IEEE subtraction each; superman_amd/csrc/tortab.hpp)
 * turns the table into all 2^n torontonians for the price of one.
 * out: 2^n doubles.  transform = 0: out = raw.  transform != 0: out[mask] =
 * the (loop) torontonian of the sub-list of the positions in mask, out[0] = 1.
 * Bit-identical on the device (the table forms of walk_tor.hip / walk_ltor.hip,
 * then mobius.hip), for any queue group, any pass shape and on host threads
 * (on_cpu = 1).  A pivot that is not positive makes raw[z] NaN, which reaches
 * exactly the masks that contain z.
 * Errors, all before any device work: a null pointer, n outside [1, 32], a
 * mode outside [0, M) or named twice, o->gpu_num > 1 (a table is one device's,
 * o->device_id), a SUP_MOBIUS_BITS the transform was not compiled for:
 * SUP_EINVAL; n above SUP_TORONTONIAN_TABLE_MAX_N on either path:
 * SUP_EUNSUPPORTED; no device with on_cpu = 0: SUP_ENODEV.
 * st: leaves = 1, gray_steps = visited_steps = 2^n, kernel_ms = prepare + walk
 * + transform, est_ops_per_step = the entry's census + n / 2. */
#define SUP_TORONTONIAN_TABLE_MAX_N 28   /* 2 GiB of results */
int sup_torontonian_table(const double* O, int M, const int32_t* modes, int n, int transform, const sup_opts* o,
                          int on_cpu, double* out, sup_stats* st);
int sup_loop_torontonian_table(const double* O, int M, const double* gamma, const int32_t* modes, int n, int transform,
                               const sup_opts* o, int on_cpu, double* out, sup_stats* st);
/* The transform alone on t[0 .. 2^n), in place, n in [0, 28], on device
 * o->device_id or (on_cpu = 1) host threads; exported for the test harness.
 * The environment knob SUP_MOBIUS_BITS=L,K (read per call) forces a smaller
 * tile (2^L doubles per work-group) and fewer bits per further pass (K) than
 * the compiled defaults; the bits do not depend on it. */
int sup_mobius_subsets(double* t, int n, const sup_opts* o, int on_cpu);

/* Nijenhuis-Wilf prologue (gpu_exact_dense.cu:642-652): x0[j] = a[j][n-1] - rowsum_j/2,
 * p0 = prod x0.  Host-only helper, exported for the test harness. */
int sup_nw_start(const void* mat, sup_dtype t, int n, double* x0, double* p0);

/* ------------------------------------------------------------------------ *
 * Reference-signature wrappers: one per GPU exact wrapper of the v1 tree.
 * Arguments keep the reference meaning; grid_dim/block_dim are accepted for
 * signature compatibility (the engine sizes its own launch when they are <= 0
 * or when they do not match its 256-thread wave-chunk layout).
 * ------------------------------------------------------------------------ */

/* gpu_exact_dense.cu:641 gpu_perman64_xshared_coalescing_mshared (-p4) */
int sup_gpu_perman64_xshared_coalescing_mshared(const void* mat, sup_dtype t, int nov,
    int grid_dim, int block_dim, double* out);
/* gpu_exact_dense.cu:702 ..._multigpu (-p5) */
int sup_gpu_perman64_xshared_coalescing_mshared_multigpu(const void* mat, sup_dtype t, int nov,
    int gpu_num, int grid_dim, int block_dim, double* out);
/* gpu_exact_dense.cu:777 ..._multigpucpu_chunks (-p6) */
int sup_gpu_perman64_xshared_coalescing_mshared_multigpucpu_chunks(const void* mat, sup_dtype t,
    int nov, int gpu_num, int cpu, int threads, int grid_dim, int block_dim, double* out);
/* gpu_exact_sparse.cu:854 ..._sparse (-p4 -s) */
int sup_gpu_perman64_xshared_coalescing_mshared_sparse(const void* mat, const int* cptrs,
    const int* rows, const void* cvals, sup_dtype t, int nov, int grid_dim, int block_dim,
    double* out);
/* gpu_exact_sparse.cu:917 ..._multigpu_sparse (-p5 -s) */
int sup_gpu_perman64_xshared_coalescing_mshared_multigpu_sparse(const void* mat, const int* cptrs,
    const int* rows, const void* cvals, sup_dtype t, int nov, int gpu_num, int grid_dim,
    int block_dim, double* out);
/* gpu_exact_sparse.cu:996 ..._multigpucpu_chunks_sparse (-p6 -s) */
int sup_gpu_perman64_xshared_coalescing_mshared_multigpucpu_chunks_sparse(const void* mat,
    const int* cptrs, const int* rows, const void* cvals, sup_dtype t, int nov, int gpu_num,
    int cpu, int threads, int grid_dim, int block_dim, double* out);
/* gpu_exact_dense.cu:914 ..._multigpu_manual_distribution (-p66): 3/8, 3/8, 1/8, 1/8 on 4 devices */
int sup_gpu_perman64_xshared_coalescing_mshared_multigpu_manual_distribution(const void* mat, sup_dtype t,
    int nov, int gpu_num, int grid_dim, int block_dim, double* out);
/* gpu_exact_sparse.cu:1328 ..._multigpu_sparse_manual_distribution (-p66 -s) */
int sup_gpu_perman64_xshared_coalescing_mshared_multigpu_sparse_manual_distribution(const void* mat,
    const int* cptrs, const int* rows, const void* cvals, sup_dtype t, int nov, int gpu_num, int grid_dim,
    int block_dim, double* out);
/* gpu_exact_sparse.cu:1124 ..._skipper (-p7 -s) */
int sup_gpu_perman64_xshared_coalescing_mshared_skipper(const void* mat, const int* rptrs,
    const int* cols, const int* cptrs, const int* rows, const void* cvals, sup_dtype t, int nov,
    int grid_dim, int block_dim, double* out);
/* gpu_exact_sparse.cu:1193 ..._multigpucpu_chunks_skipper (-p8 -s) */
int sup_gpu_perman64_xshared_coalescing_mshared_multigpucpu_chunks_skipper(const void* mat,
    const int* rptrs, const int* cols, const int* cptrs, const int* rows, const void* cvals,
    sup_dtype t, int nov, int gpu_num, int cpu, int threads, int grid_dim, int block_dim,
    double* out);

/* ------------------------------------------------------------------------ *
 * Host preprocessing (hot-path inputs).
 * ------------------------------------------------------------------------ */

/* v1 matrix file: header "n nnz type", then 0-based "i j v" lines; malformed
 * lines skipped; binary => every listed entry is 1 (util.h:343-358,
 * main.cu:494-498).  *mat is allocated with malloc (free with sup_free). */
int sup_read_matrix(const char* path, int binary, void** mat, sup_dtype* t, int* n, int* nnz_header);
void sup_free(void* p);

/* CSR + CSC of a dense row-major matrix; nonzero test is != 0 (the reference
 * uses > 0 at util.h:537,542 and silently drops negative entries).  Arrays
 * are caller-allocated: cptrs/rptrs n+1, rows/cols/vals nnz (query nnz with
 * sup_count_nnz).  (util.h:522-551) */
int sup_count_nnz(const void* mat, sup_dtype t, int n, int* nnz);
int sup_compress(const void* mat, sup_dtype t, int n, int* cptrs, int* rows, void* cvals,
                 int* rptrs, int* cols, void* rvals);
/* SortOrder: stable ascending column nnz; rewrites mat in place and fills
 * colperm (new column c = old column colperm[c]).  (util.h:553-619) */
int sup_sort_order(void* mat, sup_dtype t, int n, int* colperm);
/* SkipOrder: greedy min-degree column order, rows in first-touch order;
 * rewrites mat in place.  (util.h:621-684) */
int sup_skip_order(void* mat, sup_dtype t, int n, int* rowperm, int* colperm);

/* MatrixMarket coordinate file (revised_perman/read_matrix.hpp:11-157 and
 * main.cpp:1515-1580): banner "%%MatrixMarket matrix coordinate <type>
 * <symmetry>", '%' comments, "M N nz", 1-based "i j [v]" entries.  real ->
 * SUP_FLOAT64; integer / pattern (or binary) -> SUP_INT32; pattern or binary
 * entries are 1; symmetric and skew-symmetric files mirror every off-diagonal
 * entry with the SAME value (as the reference does); complex, array format
 * and non-square matrices are rejected (SUP_EIO).  nnz_lines = nz from the
 * size line.  n may be up to SUP_MAX_READ_N (for sup_perman_reduced).
 * sup_read_matrix also accepts MatrixMarket files (detected by the banner),
 * so the CLI's -f takes either format. */
int sup_read_mtx(const char* path, int binary, void** mat, sup_dtype* t, int* n, int* nnz_lines);
/* MatrixMarket coordinate file whose field is `complex`: "i j re im" entries
 * (ABI 11).  *mat: n x n row-major interleaved (re, im) doubles (sup_free).
 * general: as written; symmetric: off-diagonal entries mirrored with the same
 * value; hermitian: mirrored with the conjugate, and a diagonal entry's
 * imaginary part must be 0.  skew-symmetric, other fields, array format,
 * non-square, truncated or out-of-range entries: SUP_EIO.  Later duplicates
 * win.  n up to SUP_MAX_N only (there are no complex reductions). */
int sup_read_mtx_complex(const char* path, double** mat, int* n, int* nnz_lines);

/* ------------------------------------------------------------------------ *
 * Reductions in front of the engine (reference v2
 * -o / -u, revised_perman/main.cpp:993-1264, util.h:1138-1593).
 * ------------------------------------------------------------------------ */
typedef struct {
  int compress;           /* -o: remove degree-1/2 rows+columns, then expand rows/columns of
                             degree < max_deg while n > min_n (d1/d2/d34 recursion)            */
  double scale_threshold; /* -u <t>: scale rows/columns to sums t before each permanent and
                             divide the factors out afterwards; <= 0 = off                      */
  int min_n;              /* recursion stops at n <= min_n (reference: 30)                      */
  int max_deg;            /* expand only while the minimum degree < max_deg (reference: 5)      */
  int preprocessing;      /* -r applied to every leaf: 0 none, 1 SortOrder, 2 SkipOrder         */
} sup_reduce_opts;
void sup_reduce_opts_init(sup_reduce_opts* r);

/* Leaf permanent callback: perm of the n x n fp64 row-major matrix a. */
typedef int (*sup_leaf_fn)(const double* a, int n, void* user, double* out_perm);

/* Reduce `mat` and combine fn(leaf) over the expansion tree (left + right,
 * scale factors divided out).  No device work of its own: fn decides how each
 * leaf is computed.  *n_leaves = number of fn calls.  n <= SUP_MAX_READ_N;
 * a leaf larger than SUP_MAX_N fails with SUP_EUNSUPPORTED. */
int sup_decompose(const void* mat, sup_dtype t, int n, const sup_reduce_opts* r, sup_leaf_fn fn, void* user,
                  double* out, int* n_leaves);

/* sup_decompose with every leaf computed by the engine: sup_perman (on_cpu =
 * 0) or sup_perman_cpu (on_cpu = 1, o->threads threads) after r->preprocessing.
 * st accumulates over the leaves (kernel_ms, wall_ms, gray_steps, visited_steps,
 * leaves); the other fields describe the last leaf. */
int sup_perman_reduced(const void* mat, sup_dtype t, int n, sup_kernel kernel, sup_sched sched, const sup_opts* o,
                       int on_cpu, const sup_reduce_opts* r, double* out, sup_stats* st);

/* sup_perman_exact after the -o reductions (d1/d2/d34, as sup_perman_reduced
 * with r->compress; scaling is refused: not exact).  The tree folds every
 * coefficient into its leaves, so the permanent is the exact sum of the exact
 * leaf permanents (a big integer; up to 4096 x 4096 input, leaves <= 64).
 * st (optional): kernel_ms summed over leaves, leaves, wall_ms. */
int sup_perman_reduced_exact(const void* mat, sup_dtype t, int n, const sup_opts* o, int on_cpu,
                             const sup_reduce_opts* r, char* out, size_t out_len, sup_stats* st);

/* sup_perman_quad after the -o / -u reductions (as sup_perman_reduced):
 * every leaf by the double-double walk, the tree combined (sums, and the
 * scaling factors divided out) in double-double.  The leaf matrices are
 * formed in fp64 as in the reference; the fp64 walk's cancellation, which
 * costs the reduced sum its digits (HISTORY.md §7), is gone.  st->leaves = the
 * leaf count. */
int sup_perman_reduced_quad(const void* mat, sup_dtype t, int n, const sup_opts* o, int on_cpu,
                            const sup_reduce_opts* r, double* out_hi, double* out_lo, sup_stats* st);



/* ------------------------------------------------------------------------ *
 * Randomized estimators (reference -a, main.cu:77-103,
 * 156-183, 193-243).  Both estimate the permanent of the 0/1 nonzero pattern,
 * as the reference's do.  method 0: Rasmussen (kernel_rasmussen,
 * gpu_approximation_dense.cu:155-229; CPU algo.h:270-366); method 1:
 * scaling-guided importance sampling (kernel_approximation,
 * gpu_approximation_dense.cu:231-371; CPU algo.h:472-560) with Sinkhorn
 * passes every scale_intervals steps (-y, default 4), scale_times passes each
 * (-z, default 5).  `samples` (-x, default 100000) is rounded up to a multiple
 * of 64.  Randomness is Philox4x32-10 keyed by `seed`, counter (sample, step):
 * the estimate is a function of (matrix, method, samples, seed) only — the same
 * on the CPU (on_cpu = 1, o->threads threads), on one GPU or on o->gpu_num
 * GPUs (+ o->cpu_worker), which is how the reference's _multigpucpu_chunks
 * forms (gpu_approximation_dense.cu:411-525, 573-700) map here.  n <= 1024.
 * ------------------------------------------------------------------------ */
typedef struct {
  double   mean;           /* the estimate                                      */
  double   std_error;      /* sample standard deviation / sqrt(samples)         */
  double   zero_fraction;  /* samples that hit a dead end (estimate 0)          */
  uint64_t samples;        /* samples drawn (multiple of 64)                    */
  double   kernel_ms;      /* device time (max over devices)                    */
  double   wall_ms;
  int      devices;
  int      reserved_;
  int64_t  cpu_blocks;     /* 64-sample blocks computed on host threads         */
} sup_approx_result;

int sup_approx(const void* mat, sup_dtype t, int n, int method, uint64_t samples, int scale_intervals,
               int scale_times, uint64_t seed, const sup_opts* o, int on_cpu, sup_approx_result* res);

/* Grid graph of the -i mode (util.h:403-520 gridGraph2compressed): the
 * bipartite adjacency (nov = m*n/2, one of m, n even) whose permanent is the
 * number of domino tilings of the m x n board; *mat from malloc (sup_free). */
int sup_grid_graph(int m, int n, int** mat, int* nov);

#ifdef __cplusplus
}
#endif
#endif /* SUPERMAN_H */
