"""superman_amd — MI355X-native exact matrix permanent (Ryser / Gray code).

Host-side mirror of the reference's operator interface (kamerkaya/SUPerman
v1): ``RunAlgo<T>``'s algorithm-id dispatch (main.cu:20-248) and the GPU
wrapper functions (gpu_exact_dense.cu:641-990, gpu_exact_sparse.cu:854-1408),
over the C ABI of ``libsuperman_hip.so`` (include/superman.h).  All compute
runs in the gfx950 HIP kernels of ``superman_amd/csrc``; the GPU functions
raise ``SupError`` (SUP_ENODEV) when no device is present — there is no CPU
fallback.  ``perman_cpu`` is the explicit CPU algorithm of the CLI's ``-c``.
"""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np

from . import _lib
from ._lib import (KERNEL_DENSE, KERNEL_SKIPPER, KERNEL_SPARYSER, LEAF_FN, SCHED_CHUNKS, SCHED_MANUAL, SCHED_SINGLE,
                   SCHED_STATIC, SupApproxResult, SupError, SupOpts, SupReduceOpts, SupStats)

__all__ = [
    "perman", "perman_cpu", "perman_exact", "perman_exact_range", "perman_quad", "perman_quad_range", "perman_complex", "perman_complex_range", "perman_complex_quad", "perman_complex_quad_range", "COMPLEX_QUAD_MAX_DEVICE_N", "perman_complex_exact", "perman_complex_exact_range", "COMPLEX_EXACT_MAX_DEVICE_N", "perman_complex_batch", "perman_complex_submatrices", "perman_complex_fock", "perman_complex_fock_plan", "perman_complex_fock_minors", "perman_complex_fock_minors_submatrices",
           "hafnian", "loop_hafnian", "hafnian_repeated", "hafnian_batch", "hafnian_plan",
           "hafnian_exact", "loop_hafnian_exact", "hafnian_exact_repeated", "hafnian_exact_batch",
           "hafnian_quad", "loop_hafnian_quad", "hafnian_quad_repeated", "hafnian_quad_batch", "HAFNIAN_QUAD_MAX_DEVICE_N",
           "hafnian_powertrace", "loop_hafnian_powertrace", "hafnian_powertrace_batch", "hafnian_powertrace_range",
           "hafnian_powertrace_plan", "HAFNIAN_PT_MAX_DEVICE_N",
           "torontonian", "torontonian_batch", "torontonian_range", "torontonian_plan", "TORONTONIAN_MAX_DEVICE_N",
           "loop_torontonian", "loop_torontonian_batch", "loop_torontonian_range", "loop_torontonian_plan",
           "LOOP_TORONTONIAN_MAX_DEVICE_N", "ltor_exp", "threshold_detection_prob", "threshold_detection_probs",
           "torontonian_table", "loop_torontonian_table", "subset_mobius", "TORONTONIAN_TABLE_MAX_N",
           "MOBIUS_TILE_BITS", "MOBIUS_PASS_BITS", "threshold_detection_distribution", "threshold_detection_sample",
           "loop_hafnian_each", "gbs_pure_state", "pnr_detection_prob", "pnr_detection_probs", "gbs_sample",
           "gbs_sample_chain", "loop_torontonian_each", "threshold_sample_chain", "threshold_sample", "loop_hafnian_table", "loop_hafnian_table_plan", "LHAF_TABLE_MAX_ENTRIES",
           "gbs_state_vector", "gbs_density_matrix", "pnr_detection_distribution",
           "pnr_detection_sample",
           "perman_complex_fock_minors_plan","perman_complex_minors", "perman_complex_minors_submatrices", "perman_complex_minors_range", "boson_sample", "read_mtx_complex", "partial", "perman_shard", "plan_info", "plan_census", "CENSUS_CLASSES", "plan_key", "prepare", "read_matrix", "read_mtx", "sort_order",
    "skip_order", "compress", "decompose", "perman_reduced", "approx", "grid_graph", "ALGOS_APPROX",
    "nw_start", "device_count", "rccl_devices", "layout", "ShardCall", "SupError", "ALGOS_DENSE", "ALGOS_SPARSE",
    "gpu_perman64_xshared_coalescing_mshared",
    "gpu_perman64_xshared_coalescing_mshared_multigpu",
    "gpu_perman64_xshared_coalescing_mshared_multigpucpu_chunks",
    "gpu_perman64_xshared_coalescing_mshared_sparse",
    "gpu_perman64_xshared_coalescing_mshared_multigpu_sparse",
    "gpu_perman64_xshared_coalescing_mshared_multigpucpu_chunks_sparse",
    "gpu_perman64_xshared_coalescing_mshared_skipper",
    "gpu_perman64_xshared_coalescing_mshared_multigpucpu_chunks_skipper",
]

_DT = {np.dtype(np.int32): _lib.SUP_INT32, np.dtype(np.float32): _lib.SUP_FLOAT32,
       np.dtype(np.float64): _lib.SUP_FLOAT64}
_NP = {_lib.SUP_INT32: np.int32, _lib.SUP_FLOAT32: np.float32, _lib.SUP_FLOAT64: np.float64}
_TYPE_NAME = {_lib.SUP_INT32: "int", _lib.SUP_FLOAT32: "float", _lib.SUP_FLOAT64: "double"}

# main.cu:30-143 GPU exact dispatch: algo id -> (name, kernel, schedule)
ALGOS_DENSE = {
    0: ("gpu_perman64_xglobal", KERNEL_DENSE, SCHED_SINGLE),
    1: ("gpu_perman64_xlocal", KERNEL_DENSE, SCHED_SINGLE),
    2: ("gpu_perman64_xshared", KERNEL_DENSE, SCHED_SINGLE),
    3: ("gpu_perman64_xshared_coalescing", KERNEL_DENSE, SCHED_SINGLE),
    4: ("gpu_perman64_xshared_coalescing_mshared", KERNEL_DENSE, SCHED_SINGLE),
    5: ("gpu_perman64_xshared_coalescing_mshared_multigpu", KERNEL_DENSE, SCHED_STATIC),
    6: ("gpu_perman64_xshared_coalescing_mshared_multigpucpu_chunks", KERNEL_DENSE, SCHED_CHUNKS),
    66: ("gpu_perman64_xshared_coalescing_mshared_multigpu_manual_distribution", KERNEL_DENSE, SCHED_MANUAL),
}
ALGOS_SPARSE = {
    1: ("gpu_perman64_xlocal_sparse", KERNEL_SPARYSER, SCHED_SINGLE),
    2: ("gpu_perman64_xshared_sparse", KERNEL_SPARYSER, SCHED_SINGLE),
    3: ("gpu_perman64_xshared_coalescing_sparse", KERNEL_SPARYSER, SCHED_SINGLE),
    4: ("gpu_perman64_xshared_coalescing_mshared_sparse", KERNEL_SPARYSER, SCHED_SINGLE),
    5: ("gpu_perman64_xshared_coalescing_mshared_multigpu_sparse", KERNEL_SPARYSER, SCHED_STATIC),
    6: ("gpu_perman64_xshared_coalescing_mshared_multigpucpu_chunks_sparse", KERNEL_SPARYSER, SCHED_CHUNKS),
    7: ("gpu_perman64_xshared_coalescing_mshared_skipper", KERNEL_SKIPPER, SCHED_SINGLE),
    8: ("gpu_perman64_xshared_coalescing_mshared_multigpucpu_chunks_skipper", KERNEL_SKIPPER, SCHED_CHUNKS),
    66: ("gpu_perman64_xshared_coalescing_mshared_multigpu_sparse_manual_distribution", KERNEL_SPARYSER,
         SCHED_MANUAL),
}
_KERNELS = {"dense": KERNEL_DENSE, "sparse": KERNEL_SPARYSER, "spa": KERNEL_SPARYSER,
            "skipper": KERNEL_SKIPPER, "skip": KERNEL_SKIPPER, "dense_plain": _lib.KERNEL_DENSE_PLAIN,
            "seg": _lib.KERNEL_SEGMENTED, "segmented": _lib.KERNEL_SEGMENTED,
            "dense_lds": _lib.KERNEL_DENSE_LDS}
WALK_NAMES = {0: "dense", 1: "sparse", 2: "skip", 3: "seg", 4: "lds"}


def _mat(a, max_n: int = 64) -> tuple[np.ndarray, int, int]:
    a = np.asarray(a)
    if a.dtype not in _DT:
        a = a.astype(np.float64)
    a = np.ascontiguousarray(a)
    if a.ndim != 2 or a.shape[0] != a.shape[1]:
        raise ValueError(f"expected a square matrix, got shape {a.shape}")
    n = a.shape[0]
    if not 1 <= n <= max_n:
        raise ValueError(f"n = {n} outside [1, {max_n}]" + (" (64-bit Gray index)" if max_n == 64 else ""))
    return a, _DT[a.dtype], n


def _opts(gpu_num=1, device_id=0, threads=16, cpu=False, walk_log2=0, chunk_log2=0, use_rccl=False,
          verbose=False, jit=0, checkpoint=None) -> SupOpts:
    lib = _lib.load()
    o = SupOpts()
    lib.sup_opts_init(C.byref(o))
    o.gpu_num, o.device_id, o.threads = int(gpu_num), int(device_id), int(threads)
    o.cpu_worker, o.walk_log2, o.chunk_log2 = int(bool(cpu)), int(walk_log2), int(chunk_log2)
    o.use_rccl, o.verbose = int(use_rccl), int(bool(verbose))  # use_rccl=2: RCCL even on one device
    o.jit = int(jit)  # segmented walk: -1 never, 0 auto, 1 whenever its cost model wins
    # chunk queue (-p6/-p8): record / resume finished items (the struct keeps the bytes alive via _objects)
    o.checkpoint = os.fsencode(checkpoint) if checkpoint else None
    return o


def device_count() -> int:
    lib = _lib.load()
    c = C.c_int(0)
    rc = lib.sup_device_count(C.byref(c))
    return c.value if rc == 0 else 0


def rccl_devices(ndev: int) -> list:
    """Physical devices the -R RCCL combine uses for logical devices
    0..ndev-1 (SUP_DEVICE_MAP); raises SupError when two share a GPU."""
    lib = _lib.load()
    out = (C.c_int * max(1, ndev))()
    _lib.check(lib.sup_rccl_devices(ndev, out), "rccl_devices")
    return list(out[:ndev])


def layout(n: int) -> tuple[int, int, int]:
    """Engine layout (lane bits L, walk bits m, wave-chunk bits h) for order n."""
    nb = n - 1
    L = min(6, nb)
    rest = nb - L
    m = min(rest, 10)
    if rest - m < 13:  # small n: shorter walks, 2^13 wave-chunks (plan.cpp default_layout)
        m = max(min(rest, 6), rest - 13)
    m = min(max(m, rest - 20), 31)
    return L, m, rest - m


def perman(mat, algo: int = 4, sparse: bool = False, gpu_num: int = 1, cpu: bool = False,
           threads: int = 16, device_id: int = 0, use_rccl: bool = False, walk_log2: int = 0,
           chunk_log2: int = 0, return_stats: bool = False, jit: int = 0, kernel: str | None = None,
           checkpoint: str | None = None):
    """GPU exact permanent, dispatched by the reference algorithm id (main.cu:30-143).

    ``sparse`` selects the sparse table (SpaRyser ids 1-6, SkipPer 7/8).  Apply
    ``sort_order``/``skip_order`` first to mirror ``-r1``/``-r2``.  ``jit``:
    pattern-specialised segmented walk (-1 never, 0 auto, 1 when it is cheaper).
    ``kernel`` overrides the algorithm id's walk family ("dense", "sparse",
    "skip", "dense_plain", "seg") and keeps its device schedule.
    ``checkpoint`` (chunk-queue ids 6 / 8 only): a file recording each finished
    queue item; a later call with the same file resumes from it (same bits).
    """
    table = ALGOS_SPARSE if sparse else ALGOS_DENSE
    if algo not in table:
        raise SupError(-7, "perman", f"unknown algorithm id {algo}")
    _, kern, sched = table[algo]
    if kernel is not None:
        kern = _KERNELS[kernel]
    if algo == 66 and gpu_num == 1:
        gpu_num = 4  # main.cu:71,150 pass 4 devices; the pieces wrap round a smaller gpu_num
    if sched == SCHED_SINGLE:
        gpu_num = 1
    a, dt, n = _mat(mat)
    lib = _lib.load()
    o = _opts(gpu_num, device_id, threads, cpu, walk_log2, chunk_log2, use_rccl, jit=jit, checkpoint=checkpoint)
    out, st = C.c_double(0.0), SupStats()
    _lib.check(lib.sup_perman(a.ctypes.data, dt, n, kern, sched, C.byref(o), C.byref(out), C.byref(st)),
               table[algo][0])
    return (out.value, st.as_dict()) if return_stats else out.value


def perman_cpu(mat, kernel: str = "dense", threads: int = 16, return_stats: bool = False):
    """The CLI's explicit CPU algorithm (-c): same walk on host threads."""
    a, dt, n = _mat(mat)
    lib = _lib.load()
    out, st = C.c_double(0.0), SupStats()
    _lib.check(lib.sup_perman_cpu(a.ctypes.data, dt, n, _KERNELS[kernel], int(threads), C.byref(out),
                                  C.byref(st)), "perman_cpu")
    return (out.value, st.as_dict()) if return_stats else out.value


def perman_exact(mat, gpu_num: int = 1, device_id: int = 0, cpu: bool = False, threads: int = 16,
                 return_stats: bool = False, cpu_worker: bool = False, chunk_log2: int = 0):
    """Exact permanent (Python int) of an integer matrix: the Ryser / Gray walk
    of 2A in residue arithmetic modulo primes, joined by CRT (sup_perman_exact).
    The reference's int / -b path is fp64; this one is exact.  ``cpu`` runs on
    host threads only; ``cpu_worker`` adds a host worker to the devices' chunk
    queue (items of 2^chunk_log2 wave-chunks, 0 = automatic)."""
    a, dt, n = _mat(mat)
    lib = _lib.load()
    o = _opts(gpu_num=gpu_num, device_id=device_id, threads=threads, cpu=cpu_worker, chunk_log2=chunk_log2)
    buf = C.create_string_buffer(1024)
    st = SupStats()
    _lib.check(lib.sup_perman_exact(a.ctypes.data, dt, n, C.byref(o), int(bool(cpu)), buf, len(buf), C.byref(st)),
               "perman_exact")
    v = int(buf.value.decode())
    return (v, st.as_dict()) if return_stats else v


def perman_quad(mat, gpu_num: int = 1, device_id: int = 0, cpu: bool = False, threads: int = 16,
                return_stats: bool = False):
    """The permanent in double-double (~106 bits; the reference's `-q` quad
    calculation, revised_perman/main.cpp:141-142) as (hi, lo), perm = hi + lo:
    the dense walk with double-double values (walk_dd.hip), on gpu_num devices
    or (cpu=True) on host threads — bit-identical either way."""
    a, dt, n = _mat(mat)
    lib = _lib.load()
    o = _opts(gpu_num=gpu_num, device_id=device_id, threads=threads)
    hi, lo, st = C.c_double(0.0), C.c_double(0.0), SupStats()
    _lib.check(lib.sup_perman_quad(a.ctypes.data, dt, n, C.byref(o), int(bool(cpu)), C.byref(hi), C.byref(lo),
                                   C.byref(st)), "perman_quad")
    return ((hi.value, lo.value), st.as_dict()) if return_stats else (hi.value, lo.value)


def _range_info(st: SupStats, colmap: np.ndarray, n: int) -> dict:
    return {"L": st.lane_bits, "m": st.walk_bits, "colmap": [int(c) for c in colmap[: n - 1]],
            "walk_kind": st.walk_kind, "gray_steps": st.gray_steps, "kernel_ms": st.kernel_ms,
            "devices_used": st.devices_used, "leaves": st.leaves, "est_ops_per_step": st.est_ops_per_step}


def perman_exact_range(mat, c0: int, c1: int, cpu: bool = False, threads: int = 16, device_id: int = 0,
                       walk_log2: int = 0, form: int = 0, group: int = 0, cap: int = 128):
    """Wave-chunks [c0, c1) of perman_exact's walk of 2A (sup_perman_exact_range):
    (residues, info).  residues[q] is the sum of the range's terms modulo
    info["primes"][q], in [0, p); info also holds L, m, colmap (engine bit e =
    matrix column colmap[e]), G (rows multiplied exactly before each
    reduction) and walk_kind (0 the dense kernel, 1 the prefix-blocked one).
    ``form``: 0 the planner's choice, 1 dense, 2 prefix-blocked; ``group``: 0
    the cost model's G, or 1, 2, 4; ``walk_log2``: walk bits (0 = default
    layout).  One device, or (cpu=True) host threads: the same residues."""
    a, dt, n = _mat(mat)
    lib = _lib.load()
    o = _opts(device_id=device_id, threads=threads, walk_log2=walk_log2)
    size = max(int(cap), 1)
    primes, res = np.zeros(size, np.uint64), np.zeros(size, np.uint64)
    colmap, np_out, st = np.zeros(max(n - 1, 1), np.int32), C.c_int(0), SupStats()
    _lib.check(lib.sup_perman_exact_range(a.ctypes.data, dt, n, int(c0), int(c1), C.byref(o), int(bool(cpu)),
                                          int(form), int(group), primes.ctypes.data, res.ctypes.data, int(cap),
                                          C.byref(np_out), colmap.ctypes.data, C.byref(st)), "perman_exact_range")
    info = _range_info(st, colmap, n)
    info["primes"] = [int(p) for p in primes[: np_out.value]]
    info["G"] = int(st.seg_pair_bits)
    return [int(r) for r in res[: np_out.value]], info


def perman_quad_range(mat, c0: int, c1: int, cpu: bool = False, threads: int = 16, device_id: int = 0,
                      walk_log2: int = 0, form: int = 0):
    """Wave-chunks [c0, c1) of perman_quad's walk (sup_perman_quad_range):
    ((hi, lo), info), the double-double chunk partials folded pairwise over
    c - c0 and not scaled by 4(n&1)-2.  info: L, m, colmap, walk_kind as
    perman_exact_range's.  One device, or (cpu=True) host threads —
    bit-identical."""
    a, dt, n = _mat(mat)
    lib = _lib.load()
    o = _opts(device_id=device_id, threads=threads, walk_log2=walk_log2)
    hi, lo, st = C.c_double(0.0), C.c_double(0.0), SupStats()
    colmap = np.zeros(max(n - 1, 1), np.int32)
    _lib.check(lib.sup_perman_quad_range(a.ctypes.data, dt, n, int(c0), int(c1), C.byref(o), int(bool(cpu)),
                                         int(form), C.byref(hi), C.byref(lo), colmap.ctypes.data, C.byref(st)),
               "perman_quad_range")
    return (hi.value, lo.value), _range_info(st, colmap, n)


def _cmat(mat) -> tuple[np.ndarray, int]:
    a = np.ascontiguousarray(np.asarray(mat, dtype=np.complex128))
    if a.ndim != 2 or a.shape[0] != a.shape[1]:
        raise ValueError(f"expected a square matrix, got shape {a.shape}")
    n = a.shape[0]
    if not 1 <= n <= 64:
        raise ValueError(f"n = {n} outside [1, 64] (64-bit Gray index)")
    return a, n  # complex128, C order: interleaved (re, im) doubles


def perman_complex(mat, gpu_num: int = 1, device_id: int = 0, cpu: bool = False, threads: int = 16,
                   walk_log2: int = 0, return_stats: bool = False):
    """The permanent of a complex matrix (anything np.asarray(..., dtype=complex128)
    accepts; real input gets a zero imaginary part) as a Python complex: the
    dense Ryser / Gray walk with complex fp64 values (walk_cplx.hip) on gpu_num
    devices, or (cpu=True) its host twin on `threads` threads — bit-identical
    either way, for any device or thread count.  ``walk_log2``: walk bits (0 =
    default layout); the result is a function of (matrix, walk bits) only."""
    a, n = _cmat(mat)
    lib = _lib.load()
    o = _opts(gpu_num=gpu_num, device_id=device_id, threads=threads, walk_log2=walk_log2)
    re, im, st = C.c_double(0.0), C.c_double(0.0), SupStats()
    _lib.check(lib.sup_perman_complex(a.ctypes.data, n, C.byref(o), int(bool(cpu)), C.byref(re), C.byref(im),
                                      C.byref(st)), "perman_complex")
    v = complex(re.value, im.value)
    return (v, st.as_dict()) if return_stats else v


def perman_complex_range(mat, c0: int, c1: int, cpu: bool = False, threads: int = 16, device_id: int = 0,
                         walk_log2: int = 0, return_stats: bool = False):
    """The part of perman_complex's sum from wave-chunks [c0, c1) of its plan,
    folded pairwise over c - c0 and not scaled by 4(n&1)-2: aligned
    power-of-two ranges folded pairwise in order, then scaled, reproduce
    perman_complex's bits.  One device, or (cpu=True) host threads."""
    a, n = _cmat(mat)
    lib = _lib.load()
    o = _opts(device_id=device_id, threads=threads, walk_log2=walk_log2)
    re, im, st = C.c_double(0.0), C.c_double(0.0), SupStats()
    _lib.check(lib.sup_perman_complex_range(a.ctypes.data, n, int(c0), int(c1), C.byref(o), int(bool(cpu)),
                                            C.byref(re), C.byref(im), C.byref(st)), "perman_complex_range")
    v = complex(re.value, im.value)
    return (v, st.as_dict()) if return_stats else v


# Largest order the device walk of perman_complex_quad serves (SUP_CPLX_QUAD_MAX_DEVICE_N).
COMPLEX_QUAD_MAX_DEVICE_N = 40


def perman_complex_quad(mat, gpu_num: int = 1, device_id: int = 0, cpu: bool = False, threads: int = 16,
                        walk_log2: int = 0, return_stats: bool = False):
    """The permanent of a complex matrix in double-double (~100 bits per part):
    ``((re_hi, re_lo), (im_hi, im_lo))``, Re = re_hi + re_lo, Im = im_hi + im_lo.
    perman_complex's plan and wave-chunks with every value a complex
    double-double (walk_cplxdd.hip) on gpu_num devices, or (cpu=True) its host
    twin on `threads` threads — bit-identical either way, for any device or
    thread count.  The device serves n <= COMPLEX_QUAD_MAX_DEVICE_N; above it
    SupError (SUP_EUNSUPPORTED) unless cpu=True (the host twin serves n <= 64)."""
    a, n = _cmat(mat)
    lib = _lib.load()
    o = _opts(gpu_num=gpu_num, device_id=device_id, threads=threads, walk_log2=walk_log2)
    out, st = (C.c_double * 4)(), SupStats()
    _lib.check(lib.sup_perman_complex_quad(a.ctypes.data, n, C.byref(o), int(bool(cpu)), out, C.byref(st)),
               "perman_complex_quad")
    v = ((out[0], out[1]), (out[2], out[3]))
    return (v, st.as_dict()) if return_stats else v


def perman_complex_quad_range(mat, c0: int, c1: int, cpu: bool = False, threads: int = 16, device_id: int = 0,
                              walk_log2: int = 0, return_stats: bool = False):
    """The part of perman_complex_quad's sum from wave-chunks [c0, c1) of its
    plan, folded pairwise over c - c0 (double-double adds per part) and not
    scaled by 4(n&1)-2, as ``((re_hi, re_lo), (im_hi, im_lo))``: aligned
    power-of-two ranges folded pairwise in order, then scaled, reproduce
    perman_complex_quad's bits.  One device, or (cpu=True) host threads."""
    a, n = _cmat(mat)
    lib = _lib.load()
    o = _opts(device_id=device_id, threads=threads, walk_log2=walk_log2)
    out, st = (C.c_double * 4)(), SupStats()
    _lib.check(lib.sup_perman_complex_quad_range(a.ctypes.data, n, int(c0), int(c1), C.byref(o), int(bool(cpu)), out,
                                                 C.byref(st)), "perman_complex_quad_range")
    v = ((out[0], out[1]), (out[2], out[3]))
    return (v, st.as_dict()) if return_stats else v


# Largest order the device walk of perman_complex_exact serves (SUP_CPLX_EXACT_MAX_DEVICE_N).
COMPLEX_EXACT_MAX_DEVICE_N = 61


def _cmat_exact(mat, what: str) -> tuple[np.ndarray, int]:
    """`mat` as a C-order complex128 matrix for the exact complex entries.  An
    integer that complex128 cannot hold exactly (|v| >= 2^53: an int64, or a
    Python int in an object array) is refused here, not rounded; what float
    and complex arrays hold goes to the library, which checks integrality and
    range itself."""
    raw = np.asarray(mat)
    if raw.dtype.kind in "iuO":
        for idx, v in np.ndenumerate(raw):
            if isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)) and abs(int(v)) >= 1 << 53:
                raise SupError(-1, what, f"entry {idx} = {int(v)} is not exactly representable in fp64 "
                                         "(parts must be integers with |part| < 2^31)")
    return _cmat(raw)


def perman_complex_exact(mat, gpu_num: int = 1, device_id: int = 0, cpu: bool = False, threads: int = 16,
                         return_stats: bool = False):
    """The exact permanent of a matrix of Gaussian integers as ``(re, im)``, two
    Python ints (sup_perman_complex_exact).  ``mat``: anything np.asarray turns
    into an n x n complex or integer array whose parts are integers with |part|
    < 2^31 and row sums of |Re| + |Im| below 2^31.  The Ryser / Gray sum of 2A
    in residue arithmetic over (Z/p)[i] (walk_cplxexact.hip) on gpu_num
    devices, or (cpu=True) its host twin on `threads` threads, joined by CRT:
    the same integers either way.  The device serves n <=
    COMPLEX_EXACT_MAX_DEVICE_N; above it SupError (SUP_EUNSUPPORTED) unless
    cpu=True (the host twin serves n <= 64)."""
    a, n = _cmat_exact(mat, "perman_complex_exact")
    lib = _lib.load()
    o = _opts(gpu_num=gpu_num, device_id=device_id, threads=threads)
    re, im, st = C.create_string_buffer(640), C.create_string_buffer(640), SupStats()
    _lib.check(lib.sup_perman_complex_exact(a.ctypes.data, n, C.byref(o), int(bool(cpu)), re, im, 640, C.byref(st)),
               "perman_complex_exact")
    v = (int(re.value.decode()), int(im.value.decode()))
    return (v, st.as_dict()) if return_stats else v


def perman_complex_exact_range(mat, c0: int, c1: int, group: int = 0, cpu: bool = False, threads: int = 16,
                               device_id: int = 0, walk_log2: int = 0, return_stats: bool = False, cap: int = 128):
    """Wave-chunks [c0, c1) of perman_complex_exact's walk of 2A
    (sup_perman_complex_exact_range): ``{"primes": [...], "re": [...], "im":
    [...]}``, per prime the residues in [0, p) of Re and Im of the range's part
    of T (not scaled; disjoint ranges add modulo p, the whole range is T).
    ``group``: 0 the cost model's G, or 1, 2; ``walk_log2``: walk bits (0 =
    default layout).  One device, or (cpu=True) host threads: the same
    residues."""
    a, n = _cmat_exact(mat, "perman_complex_exact_range")
    lib = _lib.load()
    o = _opts(device_id=device_id, threads=threads, walk_log2=walk_log2)
    size = max(int(cap), 1)
    primes, rre, rim = np.zeros(size, np.uint64), np.zeros(size, np.uint64), np.zeros(size, np.uint64)
    np_out, st = C.c_int(0), SupStats()
    _lib.check(lib.sup_perman_complex_exact_range(a.ctypes.data, n, int(c0), int(c1), C.byref(o), int(bool(cpu)),
                                                  int(group), primes.ctypes.data, rre.ctypes.data, rim.ctypes.data,
                                                  int(cap), C.byref(np_out), C.byref(st)),
               "perman_complex_exact_range")
    k = np_out.value
    v = {"primes": [int(x) for x in primes[:k]], "re": [int(x) for x in rre[:k]], "im": [int(x) for x in rim[:k]]}
    return (v, st.as_dict()) if return_stats else v


def _batch_result(out: np.ndarray, count: int) -> np.ndarray:
    return out[: 2 * count].view(np.complex128).copy()


def perman_complex_batch(mats, gpu_num: int = 1, device_id: int = 0, cpu: bool = False, threads: int = 16,
                         walk_log2: int = 0, return_stats: bool = False):
    """The permanents of ``count`` complex n x n matrices, ``mats`` of shape
    [count, n, n], in one call (sup_perman_complex_batch): np.ndarray
    complex128 of shape [count].  Result k is bit-identical to
    ``perman_complex(mats[k])`` with the same ``walk_log2`` — on the GPU (the
    batched walk walk_cplxb.hip for n <= 32), on any device count and
    (cpu=True) on host threads."""
    a = np.ascontiguousarray(np.asarray(mats, dtype=np.complex128))
    if a.ndim != 3 or a.shape[1] != a.shape[2]:
        raise ValueError(f"expected an array of shape [count, n, n], got shape {a.shape}")
    count, n = a.shape[0], a.shape[1]
    if not 1 <= n <= 64:
        raise ValueError(f"n = {n} outside [1, 64] (64-bit Gray index)")
    lib = _lib.load()
    o = _opts(gpu_num=gpu_num, device_id=device_id, threads=threads, walk_log2=walk_log2)
    out, st = np.zeros(2 * max(count, 1)), SupStats()
    src = a if count else np.zeros(2)  # a valid pointer for an empty batch
    _lib.check(lib.sup_perman_complex_batch(src.ctypes.data, n, count, C.byref(o), int(bool(cpu)), out.ctypes.data,
                                            C.byref(st)), "perman_complex_batch")
    v = _batch_result(out, count)
    return (v, st.as_dict()) if return_stats else v


def perman_complex_submatrices(U, rows, cols, gpu_num: int = 1, device_id: int = 0, cpu: bool = False,
                               threads: int = 16, walk_log2: int = 0, return_stats: bool = False):
    """The permanents of ``count`` n x n submatrices of one complex matrix U:
    ``rows`` and ``cols`` are integer arrays of shape [count, n], matrix k is
    ``U[np.ix_(rows[k], cols[k])]`` (indices may repeat), gathered where the
    walk's tables are written — on the device U is uploaded once
    (sup_perman_complex_submatrices).  np.ndarray complex128 of shape [count],
    bit-identical to ``perman_complex_batch`` of the gathered matrices."""
    u = np.ascontiguousarray(np.asarray(U, dtype=np.complex128))
    if u.ndim != 2 or u.shape[0] < 1 or u.shape[1] < 1:
        raise ValueError(f"expected a non-empty 2-d matrix U, got shape {u.shape}")
    r, c = np.asarray(rows), np.asarray(cols)
    if r.ndim != 2 or r.shape != c.shape:
        raise ValueError(f"rows and cols must both have shape [count, n], got {r.shape} and {c.shape}")
    for name, ix in (("rows", r), ("cols", c)):
        if ix.size and not np.issubdtype(ix.dtype, np.integer):
            raise ValueError(f"{name} must be an integer array, got dtype {ix.dtype}")
        if ix.size and (ix.min() < -2**31 or ix.max() >= 2**31):
            raise ValueError(f"{name} holds an index outside the 32-bit range")
    count, n = r.shape
    if not 1 <= n <= 64:
        raise ValueError(f"n = {n} outside [1, 64] (64-bit Gray index)")
    r32 = np.ascontiguousarray(r, dtype=np.int32) if count else np.zeros(1, np.int32)
    c32 = np.ascontiguousarray(c, dtype=np.int32) if count else np.zeros(1, np.int32)
    lib = _lib.load()
    o = _opts(gpu_num=gpu_num, device_id=device_id, threads=threads, walk_log2=walk_log2)
    out, st = np.zeros(2 * max(count, 1)), SupStats()
    _lib.check(lib.sup_perman_complex_submatrices(u.ctypes.data, u.shape[0], u.shape[1], r32.ctypes.data,
                                                  c32.ctypes.data, n, count, C.byref(o), int(bool(cpu)),
                                                  out.ctypes.data, C.byref(st)), "perman_complex_submatrices")
    v = _batch_result(out, count)
    return (v, st.as_dict()) if return_stats else v


def _index_array(name: str, ix, width: int) -> np.ndarray:
    ix = np.asarray(ix)
    if ix.ndim != 2 or ix.shape[1] != width:
        raise ValueError(f"{name} must have shape [count, {width}], got {ix.shape}")
    if ix.size and not np.issubdtype(ix.dtype, np.integer):
        raise ValueError(f"{name} must be an integer array, got dtype {ix.dtype}")
    if ix.size and (ix.min() < -2**31 or ix.max() >= 2**31):
        raise ValueError(f"{name} holds an index outside the 32-bit range")
    return np.ascontiguousarray(ix, dtype=np.int32) if ix.size else np.zeros(1, np.int32)


def perman_complex_minors_submatrices(U, rows, cols, gpu_num: int = 1, device_id: int = 0, cpu: bool = False,
                                      threads: int = 16, walk_log2: int = 0, return_stats: bool = False):
    """The permanents of all n minors of ``count`` n x (n-1) submatrices of one
    complex matrix U (sup_perman_complex_minors): ``rows`` has shape [count, n],
    ``cols`` shape [count, n-1], matrix k is ``B = U[np.ix_(rows[k], cols[k])]``
    (indices may repeat) and result [k, j] the permanent of B without row j —
    all n from one Gray walk per matrix (walk_cplxm.hip for n <= 32).
    np.ndarray complex128 of shape [count, n]; a function of (B, walk_log2)
    only: bit-identical on the GPU, on any device count and (cpu=True) on host
    threads.  n = 1 gives ones (the empty minor)."""
    u = np.ascontiguousarray(np.asarray(U, dtype=np.complex128))
    if u.ndim != 2 or u.shape[0] < 1 or u.shape[1] < 1:
        raise ValueError(f"expected a non-empty 2-d matrix U, got shape {u.shape}")
    r = np.asarray(rows)
    if r.ndim != 2:
        raise ValueError(f"rows must have shape [count, n], got {r.shape}")
    count, n = r.shape
    if not 1 <= n <= 64:
        raise ValueError(f"n = {n} outside [1, 64] (64-bit Gray index)")
    c = np.asarray(cols)
    if c.shape != (count, n - 1):
        raise ValueError(f"cols must have shape [count, n - 1] = {(count, n - 1)}, got {c.shape}")
    r32 = _index_array("rows", r, n)
    c32 = _index_array("cols", c.reshape(count, n - 1), n - 1)
    lib = _lib.load()
    o = _opts(gpu_num=gpu_num, device_id=device_id, threads=threads, walk_log2=walk_log2)
    out, st = np.zeros(2 * max(count * n, 1)), SupStats()
    _lib.check(lib.sup_perman_complex_minors(u.ctypes.data, u.shape[0], u.shape[1], r32.ctypes.data, c32.ctypes.data,
                                             n, count, C.byref(o), int(bool(cpu)), out.ctypes.data, C.byref(st)),
               "perman_complex_minors_submatrices")
    v = _batch_result(out, count * n).reshape(count, n)
    return (v, st.as_dict()) if return_stats else v


def _minors_mat(B) -> tuple[np.ndarray, int]:
    b = np.ascontiguousarray(np.asarray(B, dtype=np.complex128))
    if b.ndim != 2 or b.shape[0] < 1 or b.shape[1] != b.shape[0] - 1:
        raise ValueError(f"expected an n x (n-1) matrix, got shape {b.shape}")
    return b, b.shape[0]


def perman_complex_minors(B, gpu_num: int = 1, device_id: int = 0, cpu: bool = False, threads: int = 16,
                          walk_log2: int = 0, return_stats: bool = False):
    """The permanents of the n minors of one n x (n-1) complex matrix B: value
    j is the permanent of B without row j (the gradient of the permanent of
    [B | v] with respect to v).  np.ndarray complex128 of shape [n]; goes
    through ``perman_complex_minors_submatrices`` with identity lists."""
    b, n = _minors_mat(B)
    if not 1 <= n <= 64:
        raise ValueError(f"n = {n} outside [1, 64] (64-bit Gray index)")
    u = b if n > 1 else np.zeros((1, 1), np.complex128)
    rows = np.arange(n, dtype=np.int32)[None, :]
    cols = np.arange(n - 1, dtype=np.int32)[None, :]
    res = perman_complex_minors_submatrices(u, rows, cols, gpu_num=gpu_num, device_id=device_id, cpu=cpu,
                                            threads=threads, walk_log2=walk_log2, return_stats=return_stats)
    return (res[0][0], res[1]) if return_stats else res[0]


def perman_complex_minors_range(B, c0: int, c1: int, cpu: bool = False, threads: int = 16, device_id: int = 0,
                                walk_log2: int = 0, return_stats: bool = False):
    """Per minor of the n x (n-1) matrix B (n in [2, 32]) the part of its sum
    from wave-chunks [c0, c1) of the order-(n-1) plan, folded pairwise over
    c - c0 and not scaled by 4((n-1)&1)-2: aligned power-of-two ranges folded
    pairwise in order, then scaled, reproduce perman_complex_minors' bits.
    np.ndarray complex128 of shape [n].  One device, or (cpu=True) host threads."""
    b, n = _minors_mat(B)
    lib = _lib.load()
    o = _opts(device_id=device_id, threads=threads, walk_log2=walk_log2)
    out, st = np.zeros(2 * n), SupStats()
    src = b if b.size else np.zeros(2)
    _lib.check(lib.sup_perman_complex_minors_range(src.ctypes.data, n, int(c0), int(c1), C.byref(o), int(bool(cpu)),
                                                   out.ctypes.data, C.byref(st)), "perman_complex_minors_range")
    v = _batch_result(out, n)
    return (v, st.as_dict()) if return_stats else v


def boson_sample(U, inputs, nsamples: int, seed: int = 0, gpu_num: int = 1, device_id: int = 0, cpu: bool = False,
                 threads: int = 16, walk_log2: int = 0, return_stats: bool = False, collision_aware: bool = False):
    """``nsamples`` exact boson-sampling outcomes (Clifford & Clifford 2018,
    algorithm A; sup_boson_sample): n = len(inputs) photons enter the M x M
    unitary U in the distinct modes ``inputs``.  np.ndarray int32 of shape
    [nsamples, n]: each row the output modes, ascending (a mode repeats where
    photons collide).  Sample s depends on (U, inputs, seed, s) only — the
    GPU and (cpu=True) the host twin draw identical samples.
    ``collision_aware=True`` (sup_boson_sample_fock) takes every stage's
    minors from ``perman_complex_fock_minors_submatrices``, whose walk
    collapses the modes drawn more than once; its stats' ``visited_steps`` is
    the sum of the terms walked, ``gray_steps`` stays nominal."""
    u = np.ascontiguousarray(np.asarray(U, dtype=np.complex128))
    if u.ndim != 2 or u.shape[0] != u.shape[1] or u.shape[0] < 1:
        raise ValueError(f"expected a square matrix U, got shape {u.shape}")
    ins = np.asarray(inputs)
    if ins.ndim != 1 or ins.size < 1:
        raise ValueError(f"inputs must be a non-empty 1-d list of modes, got shape {ins.shape}")
    if not np.issubdtype(ins.dtype, np.integer):
        raise ValueError(f"inputs must be integers, got dtype {ins.dtype}")
    if ins.min() < -2**31 or ins.max() >= 2**31:
        raise ValueError("inputs holds a mode outside the 32-bit range")
    i32 = np.ascontiguousarray(ins, dtype=np.int32)
    nsamples, n = int(nsamples), int(i32.size)
    if nsamples < 0:
        raise ValueError("nsamples must be >= 0")
    lib = _lib.load()
    o = _opts(gpu_num=gpu_num, device_id=device_id, threads=threads, walk_log2=walk_log2)
    out, st = np.zeros((max(nsamples, 1), n), np.int32), SupStats()
    entry = lib.sup_boson_sample_fock if collision_aware else lib.sup_boson_sample
    _lib.check(entry(u.ctypes.data, u.shape[0], i32.ctypes.data, n, nsamples, int(seed) & 0xFFFFFFFFFFFFFFFF,
                     C.byref(o), int(bool(cpu)), out.ctypes.data, C.byref(st)), "boson_sample")
    v = out[:nsamples].copy()
    if not return_stats:
        return v
    d = st.as_dict()
    d["minors_ms"], d["pmf_ms"] = float(st.partials[0]), float(st.partials[1])
    return v, d


def _fock_lists(rows, cols):
    """rows / cols of shape [n] or [count, n] as contiguous int32 [count, n];
    single: the lists had shape [n]."""
    r, c = np.asarray(rows), np.asarray(cols)
    single = r.ndim == 1
    if single:
        r, c = r[None, :], c[None, :] if c.ndim == 1 else c
    if r.ndim != 2 or r.shape != c.shape:
        raise ValueError(f"rows and cols must both have shape [n] or [count, n], got {np.shape(rows)} and "
                         f"{np.shape(cols)}")
    for name, ix in (("rows", r), ("cols", c)):
        if ix.size and not np.issubdtype(ix.dtype, np.integer):
            raise ValueError(f"{name} must be an integer array, got dtype {ix.dtype}")
        if ix.size and (ix.min() < -2**31 or ix.max() >= 2**31):
            raise ValueError(f"{name} holds an index outside the 32-bit range")
    count, n = r.shape
    if not 1 <= n <= 64:
        raise ValueError(f"n = {n} outside [1, 64] (64-bit Gray index)")
    r32 = np.ascontiguousarray(r, dtype=np.int32) if count else np.zeros(1, np.int32)
    c32 = np.ascontiguousarray(c, dtype=np.int32) if count else np.zeros(1, np.int32)
    return r32, c32, count, n, single


def perman_complex_fock(U, rows, cols, gpu_num: int = 1, device_id: int = 0, cpu: bool = False, threads: int = 16,
                        return_stats: bool = False):
    """The permanents of n x n submatrices ``U[np.ix_(rows[k], cols[k])]`` of
    one complex matrix U, as ``perman_complex_submatrices`` but collision
    aware (sup_perman_complex_fock): equal indices on one side make equal
    columns (or rows), and the sum then runs over the multiplicity vectors of
    the side with fewer terms, T = prod (t'_k + 1) instead of 2^(n-1) (the
    collision-aware walk walk_cplxf.hip, or (cpu=True) its host twin,
    bit-identical).  Lists of shape [n] give one Python complex, of shape
    [count, n] a complex128 array of shape [count].  The values equal
    ``perman_complex_submatrices``' up to rounding, not bit for bit."""
    u = np.ascontiguousarray(np.asarray(U, dtype=np.complex128))
    if u.ndim != 2 or u.shape[0] < 1 or u.shape[1] < 1:
        raise ValueError(f"expected a non-empty 2-d matrix U, got shape {u.shape}")
    r32, c32, count, n, single = _fock_lists(rows, cols)
    lib = _lib.load()
    o = _opts(gpu_num=gpu_num, device_id=device_id, threads=threads)
    out, st = np.zeros(2 * max(count, 1)), SupStats()
    _lib.check(lib.sup_perman_complex_fock(u.ctypes.data, u.shape[0], u.shape[1], r32.ctypes.data, c32.ctypes.data,
                                           n, count, C.byref(o), int(bool(cpu)), out.ctypes.data, C.byref(st)),
               "perman_complex_fock")
    v = _batch_result(out, count)
    v = complex(v[0]) if single else v
    return (v, st.as_dict()) if return_stats else v


def perman_complex_fock_plan(rows, cols):
    """What ``perman_complex_fock`` does with these lists
    (sup_perman_complex_fock_plan, host only): (terms, side) — the terms T of
    the sum and the side collapsed (0 columns, 1 rows); two ints for lists of
    shape [n], two arrays of shape [count] for [count, n]."""
    r32, c32, count, n, single = _fock_lists(rows, cols)
    lib = _lib.load()
    terms, side = np.zeros(max(count, 1), np.uint64), np.zeros(max(count, 1), np.int32)
    _lib.check(lib.sup_perman_complex_fock_plan(r32.ctypes.data, c32.ctypes.data, n, count, terms.ctypes.data,
                                                side.ctypes.data), "perman_complex_fock_plan")
    if single:
        return int(terms[0]), int(side[0])
    return terms[:count].copy(), side[:count].copy()


def perman_complex_fock_minors_submatrices(U, rows, cols, gpu_num: int = 1, device_id: int = 0, cpu: bool = False,
                                           threads: int = 16, return_stats: bool = False):
    """``perman_complex_minors_submatrices`` with the repeated columns
    collapsed (sup_perman_complex_fock_minors): ``rows`` of shape [count, n],
    ``cols`` of shape [count, n-1], result [k, j] the permanent of
    ``U[np.ix_(rows[k], cols[k])]`` without row j, all n from one walk over the
    column multiplicities, T = prod (t'_k + 1) states instead of 2^(n-2)
    (walk_cplxfm.hip, or (cpu=True) its host twin, bit-identical).  n <= 32.
    The values equal ``perman_complex_minors_submatrices``' up to rounding,
    not bit for bit."""
    u = np.ascontiguousarray(np.asarray(U, dtype=np.complex128))
    if u.ndim != 2 or u.shape[0] < 1 or u.shape[1] < 1:
        raise ValueError(f"expected a non-empty 2-d matrix U, got shape {u.shape}")
    r = np.asarray(rows)
    if r.ndim != 2 or r.shape[1] < 1:
        raise ValueError(f"rows must have shape [count, n], got {r.shape}")
    count, n = r.shape
    c = np.asarray(cols)
    if c.shape != (count, n - 1):
        raise ValueError(f"cols must have shape [count, n - 1] = {(count, n - 1)}, got {c.shape}")
    r32 = _index_array("rows", r, n)
    c32 = _index_array("cols", c.reshape(count, n - 1), n - 1)
    lib = _lib.load()
    o = _opts(gpu_num=gpu_num, device_id=device_id, threads=threads)
    out, st = np.zeros(2 * max(count * n, 1)), SupStats()
    _lib.check(lib.sup_perman_complex_fock_minors(u.ctypes.data, u.shape[0], u.shape[1], r32.ctypes.data,
                                                  c32.ctypes.data, n, count, C.byref(o), int(bool(cpu)),
                                                  out.ctypes.data, C.byref(st)),
               "perman_complex_fock_minors_submatrices")
    v = _batch_result(out, count * n).reshape(count, n)
    return (v, st.as_dict()) if return_stats else v


def perman_complex_fock_minors(B, gpu_num: int = 1, device_id: int = 0, cpu: bool = False, threads: int = 16,
                               return_stats: bool = False):
    """The permanents of the n minors of one n x (n-1) complex matrix B through
    ``perman_complex_fock_minors_submatrices`` with identity lists (no column
    repeats, so T = 2^(n-2)).  np.ndarray complex128 of shape [n]."""
    b, n = _minors_mat(B)
    u = b if n > 1 else np.zeros((1, 1), np.complex128)
    rows = np.arange(n, dtype=np.int32)[None, :]
    cols = np.arange(n - 1, dtype=np.int32)[None, :]
    res = perman_complex_fock_minors_submatrices(u, rows, cols, gpu_num=gpu_num, device_id=device_id, cpu=cpu,
                                                 threads=threads, return_stats=return_stats)
    return (res[0][0], res[1]) if return_stats else res[0]


def perman_complex_fock_minors_plan(cols):
    """The terms T ``perman_complex_fock_minors_submatrices`` walks for these
    column lists (sup_perman_complex_fock_minors_plan, host only): an int for a
    list of shape [n-1], a uint64 array of shape [count] for [count, n-1]."""
    c = np.asarray(cols)
    single = c.ndim == 1
    if single:
        c = c[None, :]
    if c.ndim != 2:
        raise ValueError(f"cols must have shape [n - 1] or [count, n - 1], got {np.shape(cols)}")
    count, q = c.shape
    c32 = _index_array("cols", c, q)
    terms = np.zeros(max(count, 1), np.uint64)
    _lib.check(_lib.load().sup_perman_complex_fock_minors_plan(c32.ctypes.data, q + 1, count, terms.ctypes.data),
               "perman_complex_fock_minors_plan")
    return int(terms[0]) if single else terms[:count].copy()


def _haf_lists(idx):
    """idx of shape [n] or [count, n] as contiguous int32 [count, n]; single:
    the list had shape [n]."""
    ix = np.asarray(idx)
    single = ix.ndim == 1
    if single:
        ix = ix[None, :]
    if ix.ndim != 2:
        raise ValueError(f"idx must have shape [n] or [count, n], got {np.shape(idx)}")
    if ix.size and not np.issubdtype(ix.dtype, np.integer):
        raise ValueError(f"idx must be an integer array, got dtype {ix.dtype}")
    if ix.size and (ix.min() < -2**31 or ix.max() >= 2**31):
        raise ValueError("idx holds an index outside the 32-bit range")
    count, n = ix.shape
    if not 1 <= n <= 64:
        raise ValueError(f"n = {n} outside [1, 64] (64-bit Gray index)")
    i32 = np.ascontiguousarray(ix, dtype=np.int32) if count else np.zeros(1, np.int32)
    return i32, count, n, single


def hafnian_batch(A, idx, mu=None, loop: bool = False, gpu_num: int = 1, device_id: int = 0, cpu: bool = False,
                  threads: int = 16, return_stats: bool = False):
    """The hafnians (``loop=True``: the loop hafnians) of the gathers
    ``A[np.ix_(idx[k], idx[k])]`` of one complex symmetric matrix A
    (sup_hafnian_complex, sup_loop_hafnian_complex): the lists may repeat, one
    index per detected photon, and the sum runs over the multiplicity vectors,
    T = prod (s'_k + 1) terms instead of 2^(n-1) (the hafnian walk
    walk_haf.hip, or (cpu=True) its host twin, bit-identical).  ``mu``
    (length M, default the diagonal of A) replaces the diagonal on self-loops
    of the loop form.  A list of shape [n] gives one Python complex, of shape
    [count, n] a complex128 array of shape [count].  Without repeats the cost
    is 2^(n-1) states: this entry is for patterns with collisions and small
    orders."""
    a = np.ascontiguousarray(np.asarray(A, dtype=np.complex128))
    if a.ndim != 2 or a.shape[0] != a.shape[1] or a.shape[0] < 1:
        raise ValueError(f"expected a non-empty square matrix A, got shape {a.shape}")
    i32, count, n, single = _haf_lists(idx)
    lib = _lib.load()
    o = _opts(gpu_num=gpu_num, device_id=device_id, threads=threads)
    out, st = np.zeros(2 * max(count, 1)), SupStats()
    if loop:
        m = np.ascontiguousarray(np.diag(a) if mu is None else np.asarray(mu, dtype=np.complex128))
        if m.shape != (a.shape[0],):
            raise ValueError(f"mu must have shape [{a.shape[0]}], got {m.shape}")
        rc = lib.sup_loop_hafnian_complex(a.ctypes.data, a.shape[0], m.ctypes.data, i32.ctypes.data, n, count,
                                          C.byref(o), int(bool(cpu)), out.ctypes.data, C.byref(st))
    else:
        rc = lib.sup_hafnian_complex(a.ctypes.data, a.shape[0], i32.ctypes.data, n, count, C.byref(o),
                                     int(bool(cpu)), out.ctypes.data, C.byref(st))
    _lib.check(rc, "loop_hafnian" if loop else "hafnian")
    v = _batch_result(out, count)
    v = complex(v[0]) if single else v
    return (v, st.as_dict()) if return_stats else v


def hafnian(A, **kw):
    """The hafnian of the whole complex symmetric matrix A (``hafnian_batch``
    with idx = 0..n-1; n <= 64, 2^(n-1) states)."""
    return hafnian_batch(A, np.arange(np.shape(A)[0]), **kw)


def loop_hafnian(A, mu=None, **kw):
    """The loop hafnian of the whole matrix A; ``mu`` defaults to its diagonal."""
    return hafnian_batch(A, np.arange(np.shape(A)[0]), mu=mu, loop=True, **kw)


def hafnian_repeated(A, rpt, mu=None, loop: bool = False, **kw):
    """The (loop) hafnian of A with mode k taken ``rpt[k]`` times (zeros
    allowed): ``hafnian_batch`` on the list that repeats k rpt[k] times."""
    r = np.asarray(rpt)
    if (r.ndim != 1 or r.shape[0] != np.shape(A)[0] or (r.size and not np.issubdtype(r.dtype, np.integer))
            or (r < 0).any()):
        raise ValueError(f"rpt must hold one non-negative integer per mode of A, got {rpt!r}")
    return hafnian_batch(A, np.repeat(np.arange(r.shape[0]), r), mu=mu, loop=loop, **kw)


def hafnian_plan(idx):
    """The terms T ``hafnian_batch`` walks for these lists
    (sup_hafnian_complex_plan, host only): an int for a list of shape [n], a
    uint64 array of shape [count] for [count, n]."""
    i32, count, n, single = _haf_lists(idx)
    terms = np.zeros(max(count, 1), np.uint64)
    _lib.check(_lib.load().sup_hafnian_complex_plan(i32.ctypes.data, n, count, terms.ctypes.data), "hafnian_plan")
    return int(terms[0]) if single else terms[:count].copy()


# include/superman.h SUP_HAFNIAN_QUAD_MAX_DEVICE_N: the largest order the device
# kernel of hafnian_quad_batch serves (host threads serve n <= 64).
HAFNIAN_QUAD_MAX_DEVICE_N = 64


def hafnian_quad_batch(A, idx, mu=None, loop: bool = False, gpu_num: int = 1, device_id: int = 0, cpu: bool = False,
                       threads: int = 16, return_stats: bool = False):
    """``hafnian_batch`` in complex double-double (sup_hafnian_complex_quad,
    sup_loop_hafnian_complex_quad): the same gathers, sum and layout, every
    running value carried to ~106 bits per part (walk_hafdd.hip, or (cpu=True)
    its host twin, bit-identical).  It is the truth ``hafnian``,
    ``loop_hafnian`` and ``hafnian_powertrace`` are judged against on matrices
    that are not Gaussian integers.  A list of shape [n] gives
    ``((re_hi, re_lo), (im_hi, im_lo))``, of shape [count, n] a float64 array of
    shape [count, 4] with those columns; each part is ``hi + lo`` exactly."""
    a = np.ascontiguousarray(np.asarray(A, dtype=np.complex128))
    if a.ndim != 2 or a.shape[0] != a.shape[1] or a.shape[0] < 1:
        raise ValueError(f"expected a non-empty square matrix A, got shape {a.shape}")
    i32, count, n, single = _haf_lists(idx)
    lib = _lib.load()
    o = _opts(gpu_num=gpu_num, device_id=device_id, threads=threads)
    out, st = np.zeros(4 * max(count, 1)), SupStats()
    if loop:
        m = np.ascontiguousarray(np.diag(a) if mu is None else np.asarray(mu, dtype=np.complex128))
        if m.shape != (a.shape[0],):
            raise ValueError(f"mu must have shape [{a.shape[0]}], got {m.shape}")
        rc = lib.sup_loop_hafnian_complex_quad(a.ctypes.data, a.shape[0], m.ctypes.data, i32.ctypes.data, n, count,
                                               C.byref(o), int(bool(cpu)), out.ctypes.data, C.byref(st))
    else:
        rc = lib.sup_hafnian_complex_quad(a.ctypes.data, a.shape[0], i32.ctypes.data, n, count, C.byref(o),
                                          int(bool(cpu)), out.ctypes.data, C.byref(st))
    _lib.check(rc, "loop_hafnian_quad" if loop else "hafnian_quad")
    v = out[:4 * count].reshape(count, 4).copy()
    if single:
        v = ((float(v[0, 0]), float(v[0, 1])), (float(v[0, 2]), float(v[0, 3])))
    return (v, st.as_dict()) if return_stats else v


def hafnian_quad(A, **kw):
    """The hafnian of the whole complex symmetric matrix A in double-double
    (``hafnian_quad_batch`` with idx = 0..n-1)."""
    return hafnian_quad_batch(A, np.arange(np.shape(A)[0]), **kw)


def loop_hafnian_quad(A, mu=None, **kw):
    """The loop hafnian of the whole matrix A in double-double; ``mu``
    defaults to its diagonal."""
    return hafnian_quad_batch(A, np.arange(np.shape(A)[0]), mu=mu, loop=True, **kw)


def hafnian_quad_repeated(A, rpt, mu=None, loop: bool = False, **kw):
    """The double-double (loop) hafnian of A with mode k taken ``rpt[k]``
    times (zeros allowed): ``hafnian_quad_batch`` on the list that repeats k
    rpt[k] times."""
    r = np.asarray(rpt)
    if (r.ndim != 1 or r.shape[0] != np.shape(A)[0] or (r.size and not np.issubdtype(r.dtype, np.integer))
            or (r < 0).any()):
        raise ValueError(f"rpt must hold one non-negative integer per mode of A, got {rpt!r}")
    return hafnian_quad_batch(A, np.repeat(np.arange(r.shape[0]), r), mu=mu, loop=loop, **kw)


def _haf_exact_parts(x, what: str, name: str) -> np.ndarray:
    """`x` as a C-order complex128 array for the exact hafnian entry
    (``_cmat_exact``'s rule): an integer complex128 cannot hold exactly is
    refused here with its place, not rounded; integrality and range of what
    float and complex arrays hold are the library's checks."""
    raw = np.asarray(x)
    if raw.dtype.kind in "iuO":
        for idx, v in np.ndenumerate(raw):
            if isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)) and abs(int(v)) >= 1 << 53:
                raise SupError(-1, what, f"{name} entry {idx} = {int(v)} is not exactly representable in fp64 "
                                         "(parts must be integers with |part| < 2^31)")
    return np.ascontiguousarray(np.asarray(raw, dtype=np.complex128))


def hafnian_exact_batch(A, idx, mu=None, loop: bool = False, gpu_num: int = 1, device_id: int = 0, cpu: bool = False,
                        threads: int = 16, return_stats: bool = False):
    """The exact hafnians (``loop=True``: loop hafnians) of the gathers
    ``A[np.ix_(idx[k], idx[k])]`` of a symmetric matrix of Gaussian integers
    (sup_hafnian_complex_exact): ``hafnian_batch``'s sum over the multiplicity
    vectors on integers, in residue arithmetic over (Z/p)[i] for primes below
    2^25 (walk_hafexact.hip, or (cpu=True) its host twin: the same integers),
    joined by CRT.  Parts of A and mu must be integers with |part| < 2^31;
    ``mu`` defaults to the diagonal of A in the loop form.  A list of shape [n]
    gives ``(re, im)``, two Python ints; of shape [count, n] a list of such
    pairs.  It is the truth ``hafnian``, ``loop_hafnian`` and
    ``hafnian_powertrace`` are judged against, and counts perfect matchings."""
    what = "loop_hafnian_exact" if loop else "hafnian_exact"
    a = _haf_exact_parts(A, what, "A")
    if a.ndim != 2 or a.shape[0] != a.shape[1] or a.shape[0] < 1:
        raise ValueError(f"expected a non-empty square matrix A, got shape {a.shape}")
    m = None
    if loop:
        m = np.ascontiguousarray(np.diag(a)) if mu is None else _haf_exact_parts(mu, what, "mu")
        if m.shape != (a.shape[0],):
            raise ValueError(f"mu must have shape [{a.shape[0]}], got {m.shape}")
    i32, count, n, single = _haf_lists(idx)
    lib = _lib.load()
    o = _opts(gpu_num=gpu_num, device_id=device_id, threads=threads)
    ln = 768
    re, im, st = C.create_string_buffer(ln * max(count, 1)), C.create_string_buffer(ln * max(count, 1)), SupStats()
    rc = lib.sup_hafnian_complex_exact(a.ctypes.data, a.shape[0], m.ctypes.data if loop else None, i32.ctypes.data, n,
                                       count, C.byref(o), int(bool(cpu)), re, im, ln, C.byref(st))
    _lib.check(rc, what)
    rb, ib = re.raw, im.raw
    v = [(int(rb[k * ln:rb.index(b"\0", k * ln)]), int(ib[k * ln:ib.index(b"\0", k * ln)])) for k in range(count)]
    v = v[0] if single else v
    return (v, st.as_dict()) if return_stats else v


def hafnian_exact(A, **kw):
    """The exact hafnian of the whole symmetric Gaussian-integer matrix A as
    ``(re, im)`` (``hafnian_exact_batch`` with idx = 0..n-1)."""
    return hafnian_exact_batch(A, np.arange(np.shape(A)[0]), **kw)


def loop_hafnian_exact(A, mu=None, **kw):
    """The exact loop hafnian of the whole matrix A; ``mu`` defaults to its diagonal."""
    return hafnian_exact_batch(A, np.arange(np.shape(A)[0]), mu=mu, loop=True, **kw)


def hafnian_exact_repeated(A, rpt, mu=None, loop: bool = False, **kw):
    """The exact (loop) hafnian of A with mode k taken ``rpt[k]`` times (zeros
    allowed): ``hafnian_exact_batch`` on the list that repeats k rpt[k] times."""
    r = np.asarray(rpt)
    if (r.ndim != 1 or r.shape[0] != np.shape(A)[0] or (r.size and not np.issubdtype(r.dtype, np.integer))
            or (r < 0).any()):
        raise ValueError(f"rpt must hold one non-negative integer per mode of A, got {rpt!r}")
    return hafnian_exact_batch(A, np.repeat(np.arange(r.shape[0]), r), mu=mu, loop=loop, **kw)


# include/superman.h SUP_HAFNIAN_PT_MAX_DEVICE_N: the largest order the
# power-trace kernel serves on the device (host threads serve n <= 64)
HAFNIAN_PT_MAX_DEVICE_N = 62


def _haf_matrix(A, mu, loop):
    a = np.ascontiguousarray(np.asarray(A, dtype=np.complex128))
    if a.ndim != 2 or a.shape[0] != a.shape[1] or a.shape[0] < 1:
        raise ValueError(f"expected a non-empty square matrix A, got shape {a.shape}")
    m = None
    if loop:
        m = np.ascontiguousarray(np.diag(a) if mu is None else np.asarray(mu, dtype=np.complex128))
        if m.shape != (a.shape[0],):
            raise ValueError(f"mu must have shape [{a.shape[0]}], got {m.shape}")
    return a, m


def hafnian_powertrace_batch(A, idx, mu=None, loop: bool = False, gpu_num: int = 1, device_id: int = 0,
                             cpu: bool = False, threads: int = 16, return_stats: bool = False):
    """The hafnians (``loop=True``: the loop hafnians) of the gathers
    ``A[np.ix_(idx[k], idx[k])]`` by the power-trace algorithm
    (sup_hafnian_complex_pt, sup_loop_hafnian_complex_pt): 2^(n/2) subsets of
    n^3-sized work each instead of ``hafnian_batch``'s 2^(n-1) states, whatever
    the repeats (the kernel walk_hafpt.hip, or (cpu=True) its host twin,
    bit-identical).  Arguments and shapes as ``hafnian_batch``; the values agree
    with it to rounding, not bit for bit.  On the device n <=
    ``HAFNIAN_PT_MAX_DEVICE_N``; host threads serve n <= 64."""
    a, m = _haf_matrix(A, mu, loop)
    i32, count, n, single = _haf_lists(idx)
    lib = _lib.load()
    o = _opts(gpu_num=gpu_num, device_id=device_id, threads=threads)
    out, st = np.zeros(2 * max(count, 1)), SupStats()
    if loop:
        rc = lib.sup_loop_hafnian_complex_pt(a.ctypes.data, a.shape[0], m.ctypes.data, i32.ctypes.data, n, count,
                                             C.byref(o), int(bool(cpu)), out.ctypes.data, C.byref(st))
    else:
        rc = lib.sup_hafnian_complex_pt(a.ctypes.data, a.shape[0], i32.ctypes.data, n, count, C.byref(o),
                                        int(bool(cpu)), out.ctypes.data, C.byref(st))
    _lib.check(rc, "loop_hafnian_powertrace" if loop else "hafnian_powertrace")
    v = _batch_result(out, count)
    v = complex(v[0]) if single else v
    return (v, st.as_dict()) if return_stats else v


def hafnian_powertrace(A, **kw):
    """The hafnian of the whole complex symmetric matrix A by the power-trace
    algorithm (``hafnian_powertrace_batch`` with idx = 0..n-1)."""
    return hafnian_powertrace_batch(A, np.arange(np.shape(A)[0]), **kw)


def loop_hafnian_powertrace(A, mu=None, **kw):
    """The loop hafnian of the whole matrix A by the power-trace algorithm;
    ``mu`` defaults to its diagonal."""
    return hafnian_powertrace_batch(A, np.arange(np.shape(A)[0]), mu=mu, loop=True, **kw)


def hafnian_powertrace_range(A, idx, z_begin: int, z_end: int, mu=None, loop: bool = False, device_id: int = 0,
                             cpu: bool = False, threads: int = 16, return_stats: bool = False):
    """The part of one list's power-trace sum from the subsets z in
    [max(1, z_begin), z_end) (sup_hafnian_complex_pt_range): the chunk
    partials of the range folded pairwise.  The whole range [0, 2^m) has
    ``hafnian_powertrace_batch``'s bits."""
    a, m = _haf_matrix(A, mu, loop)
    i32, count, n, single = _haf_lists(idx)
    if not single:
        raise ValueError("hafnian_powertrace_range takes one index list of shape [n]")
    if not (0 <= int(z_begin) < 2**64 and 0 <= int(z_end) < 2**64):
        raise ValueError("z_begin and z_end must be unsigned 64-bit integers")
    lib = _lib.load()
    o = _opts(gpu_num=1, device_id=device_id, threads=threads)
    out, st = np.zeros(2), SupStats()
    rc = lib.sup_hafnian_complex_pt_range(a.ctypes.data, a.shape[0], m.ctypes.data if loop else None, i32.ctypes.data,
                                          n, int(z_begin), int(z_end), C.byref(o), int(bool(cpu)), out.ctypes.data,
                                          C.byref(st))
    _lib.check(rc, "hafnian_powertrace_range")
    v = complex(out[0], out[1])
    return (v, st.as_dict()) if return_stats else v


def hafnian_powertrace_plan(n: int, loop: bool = False):
    """(subsets, fp64 operations per subset) of one matrix of order n
    (sup_hafnian_complex_pt_plan, host only)."""
    subsets, ops = C.c_uint64(0), C.c_double(0.0)
    _lib.check(_lib.load().sup_hafnian_complex_pt_plan(int(n), int(bool(loop)), C.byref(subsets), C.byref(ops)),
               "hafnian_powertrace_plan")
    return int(subsets.value), float(ops.value)


# include/superman.h SUP_TORONTONIAN_MAX_DEVICE_N: the largest number of modes
# the torontonian kernel serves on the device (every n the entry takes)
TORONTONIAN_MAX_DEVICE_N = 32


def _tor_matrix(O):
    o = np.ascontiguousarray(np.asarray(O, dtype=np.complex128))
    if o.ndim != 2 or o.shape[0] != o.shape[1] or o.shape[0] < 2 or o.shape[0] % 2:
        raise ValueError(f"expected a 2M x 2M matrix O with M >= 1, got shape {o.shape}")
    return o


def _tor_lists(modes):
    i32 = np.ascontiguousarray(np.asarray(modes, dtype=np.int32))
    single = i32.ndim == 1
    if single:
        i32 = i32[None, :]
    if i32.ndim != 2 or i32.shape[1] < 1:
        raise ValueError(f"modes must have shape [n] or [count, n] with n >= 1, got {np.shape(modes)}")
    return np.ascontiguousarray(i32), int(i32.shape[0]), int(i32.shape[1]), single


def torontonian_batch(O, modes, gpu_num: int = 1, device_id: int = 0, cpu: bool = False, threads: int = 16,
                      return_stats: bool = False):
    """The torontonians of the 2M x 2M Hermitian matrix ``O`` (thewalrus'
    ordering: row i is mode i, row i + M its conjugate partner) on lists of
    distinct modes (sup_torontonian): ``tor(O_s)`` with O_s the rows and columns
    {s_b, s_b + M}.  ``modes`` has shape [n] (one result, a float) or [count, n]
    (an array).  The kernel walk_tor.hip or (cpu=True) its host twin,
    bit-identical.  Only the lower triangle of O and the real parts of its
    diagonal are read; a list whose I - O_z is not positive definite for some
    subset gives NaN."""
    o = _tor_matrix(O)
    i32, count, n, single = _tor_lists(modes)
    lib = _lib.load()
    op = _opts(gpu_num=gpu_num, device_id=device_id, threads=threads)
    out, st = np.zeros(max(count, 1)), SupStats()
    rc = lib.sup_torontonian(o.ctypes.data, o.shape[0] // 2, i32.ctypes.data, n, count, C.byref(op), int(bool(cpu)),
                             out.ctypes.data, C.byref(st))
    _lib.check(rc, "torontonian")
    v = float(out[0]) if single else out[:count].copy()
    return (v, st.as_dict()) if return_stats else v


def torontonian(O, **kw):
    """The torontonian of the whole 2M x 2M matrix O (``torontonian_batch``
    with modes = 0..M-1), as thewalrus' ``tor``."""
    return torontonian_batch(O, np.arange(np.shape(O)[0] // 2), **kw)


def torontonian_range(O, modes, z_begin: int, z_end: int, device_id: int = 0, cpu: bool = False, threads: int = 16,
                      return_stats: bool = False):
    """The part of one list's torontonian sum from the subsets z in [z_begin,
    z_end) (sup_torontonian_range): the chunk partials of the range folded
    pairwise.  The whole range [0, 2^n) has ``torontonian_batch``'s bits."""
    o = _tor_matrix(O)
    i32, count, n, single = _tor_lists(modes)
    if not single:
        raise ValueError("torontonian_range takes one list of modes of shape [n]")
    if not (0 <= int(z_begin) < 2**64 and 0 <= int(z_end) < 2**64):
        raise ValueError("z_begin and z_end must be unsigned 64-bit integers")
    lib = _lib.load()
    op = _opts(gpu_num=1, device_id=device_id, threads=threads)
    out, st = np.zeros(1), SupStats()
    rc = lib.sup_torontonian_range(o.ctypes.data, o.shape[0] // 2, i32.ctypes.data, n, int(z_begin), int(z_end),
                                   C.byref(op), int(bool(cpu)), out.ctypes.data, C.byref(st))
    _lib.check(rc, "torontonian_range")
    v = float(out[0])
    return (v, st.as_dict()) if return_stats else v


def torontonian_plan(n: int):
    """(subsets, fp64 operations per subset) of one list of n modes
    (sup_torontonian_plan, host only)."""
    subsets, ops = C.c_uint64(0), C.c_double(0.0)
    _lib.check(_lib.load().sup_torontonian_plan(int(n), C.byref(subsets), C.byref(ops)), "torontonian_plan")
    return int(subsets.value), float(ops.value)


# include/superman.h SUP_LOOP_TORONTONIAN_MAX_DEVICE_N: the largest number of
# modes the loop torontonian kernel serves on the device (every n the entry takes)
LOOP_TORONTONIAN_MAX_DEVICE_N = 32


def _ltor_gamma(gamma, o):
    g = np.asarray(gamma, dtype=np.complex128)
    if g.ndim == 0:
        g = np.full(o.shape[0], complex(g), dtype=np.complex128)
    g = np.ascontiguousarray(g)
    if g.shape != (o.shape[0],):
        raise ValueError(f"gamma must have the 2M = {o.shape[0]} entries of O's rows, got shape {g.shape}")
    return g


def loop_torontonian_batch(O, gamma, modes, gpu_num: int = 1, device_id: int = 0, cpu: bool = False, threads: int = 16,
                           return_stats: bool = False):
    """The loop torontonians (thewalrus' ``ltor``) of the 2M x 2M Hermitian
    matrix ``O`` and the complex vector ``gamma`` of length 2M (a scalar fills
    it) on lists of distinct modes (sup_loop_torontonian): O and gamma in
    thewalrus' ordering, ``modes`` of shape [n] (a float) or [count, n] (an
    array).  The kernel walk_ltor.hip or (cpu=True) its host twin,
    bit-identical; gamma = 0 has ``torontonian_batch``'s bits."""
    o = _tor_matrix(O)
    g = _ltor_gamma(gamma, o)
    i32, count, n, single = _tor_lists(modes)
    lib = _lib.load()
    op = _opts(gpu_num=gpu_num, device_id=device_id, threads=threads)
    out, st = np.zeros(max(count, 1)), SupStats()
    rc = lib.sup_loop_torontonian(o.ctypes.data, o.shape[0] // 2, g.ctypes.data, i32.ctypes.data, n, count, C.byref(op),
                                  int(bool(cpu)), out.ctypes.data, C.byref(st))
    _lib.check(rc, "loop_torontonian")
    v = float(out[0]) if single else out[:count].copy()
    return (v, st.as_dict()) if return_stats else v


def loop_torontonian(O, gamma, **kw):
    """The loop torontonian of the whole matrix O and vector gamma
    (``loop_torontonian_batch`` with modes = 0..M-1), as thewalrus' ``ltor``."""
    return loop_torontonian_batch(O, gamma, np.arange(np.shape(O)[0] // 2), **kw)


def loop_torontonian_range(O, gamma, modes, z_begin: int, z_end: int, device_id: int = 0, cpu: bool = False,
                           threads: int = 16, return_stats: bool = False):
    """The part of one list's loop torontonian sum from the subsets z in
    [z_begin, z_end) (sup_loop_torontonian_range), cut and folded as
    ``torontonian_range``."""
    o = _tor_matrix(O)
    g = _ltor_gamma(gamma, o)
    i32, count, n, single = _tor_lists(modes)
    if not single:
        raise ValueError("loop_torontonian_range takes one list of modes of shape [n]")
    if not (0 <= int(z_begin) < 2**64 and 0 <= int(z_end) < 2**64):
        raise ValueError("z_begin and z_end must be unsigned 64-bit integers")
    lib = _lib.load()
    op = _opts(gpu_num=1, device_id=device_id, threads=threads)
    out, st = np.zeros(1), SupStats()
    rc = lib.sup_loop_torontonian_range(o.ctypes.data, o.shape[0] // 2, g.ctypes.data, i32.ctypes.data, n, int(z_begin),
                                        int(z_end), C.byref(op), int(bool(cpu)), out.ctypes.data, C.byref(st))
    _lib.check(rc, "loop_torontonian_range")
    v = float(out[0])
    return (v, st.as_dict()) if return_stats else v


def loop_torontonian_plan(n: int):
    """(subsets, fp64 operations per subset) of one list of n modes
    (sup_loop_torontonian_plan, host only)."""
    subsets, ops = C.c_uint64(0), C.c_double(0.0)
    _lib.check(_lib.load().sup_loop_torontonian_plan(int(n), C.byref(subsets), C.byref(ops)), "loop_torontonian_plan")
    return int(subsets.value), float(ops.value)


def ltor_exp(x, device: bool = False, device_id: int = 0):
    """The exponential of the loop torontonian's terms (ltor.hpp ltor_exp:
    fma, multiply, rint and exponent-field arithmetic only), on the host or
    elementwise on the device; the two agree bit for bit.  A scalar gives a
    float, an array an array."""
    a = np.asarray(x, dtype=np.float64)
    lib = _lib.load()
    flat = np.ascontiguousarray(a.reshape(-1))
    out = np.zeros(flat.shape[0])
    if device:
        _lib.check(lib.sup_ltor_exp_device(flat.ctypes.data, flat.shape[0], out.ctypes.data, int(device_id)), "ltor_exp")
    else:
        for i in range(flat.shape[0]):
            out[i] = lib.sup_ltor_exp(float(flat[i]))
    return float(out[0]) if a.ndim == 0 else out.reshape(a.shape)


# include/superman.h SUP_TORONTONIAN_TABLE_MAX_N: the most modes a table takes
# (2^28 doubles = 2 GiB of results), on the device and on host threads
TORONTONIAN_TABLE_MAX_N = 28
# superman_amd/csrc/tortab.hpp: the transform's compiled shape (2^L doubles per
# work-group tile, K bits per further pass); SUP_MOBIUS_BITS=L,K forces smaller
MOBIUS_TILE_BITS = 12
MOBIUS_PASS_BITS = 6


def _tor_table(O, gamma, modes, transform, device_id, cpu, threads, return_stats):
    o = _tor_matrix(O)
    g = None if gamma is None else _ltor_gamma(gamma, o)
    i32, count, n, single = _tor_lists(np.arange(o.shape[0] // 2) if modes is None else modes)
    if not single:
        raise ValueError("a torontonian table takes one list of modes of shape [n]")
    lib = _lib.load()
    op = _opts(gpu_num=1, device_id=device_id, threads=threads)
    # above the cap the entry refuses before it writes: no 2^n buffer for it
    out, st = np.zeros(1 << n if n <= TORONTONIAN_TABLE_MAX_N else 1), SupStats()
    if g is None:
        rc = lib.sup_torontonian_table(o.ctypes.data, o.shape[0] // 2, i32.ctypes.data, n, int(bool(transform)),
                                       C.byref(op), int(bool(cpu)), out.ctypes.data, C.byref(st))
    else:
        rc = lib.sup_loop_torontonian_table(o.ctypes.data, o.shape[0] // 2, g.ctypes.data, i32.ctypes.data, n,
                                            int(bool(transform)), C.byref(op), int(bool(cpu)), out.ctypes.data,
                                            C.byref(st))
    _lib.check(rc, "torontonian_table" if g is None else "loop_torontonian_table")
    return (out, st.as_dict()) if return_stats else out


def torontonian_table(O, modes=None, transform: bool = True, device_id: int = 0, cpu: bool = False, threads: int = 16,
                      return_stats: bool = False):
    """The torontonians of EVERY sub-list of one list of distinct modes
    (default: all M) from one walk (sup_torontonian_table): an array of 2^n
    doubles, entry ``mask`` = ``tor`` on the list positions whose bits ``mask``
    has, entry 0 = 1.  ``transform=False`` gives the raw table f(z) =
    1 / sqrt det(I - O_z) the walk stores; the subset Moebius transform
    (``subset_mobius``) of it is the result.  One device or (cpu=True) the host
    twin, bit-identical; n <= ``TORONTONIAN_TABLE_MAX_N``.  A subset that is not
    positive definite makes exactly the masks that contain it NaN."""
    return _tor_table(O, None, modes, transform, device_id, cpu, threads, return_stats)


def loop_torontonian_table(O, gamma, modes=None, transform: bool = True, device_id: int = 0, cpu: bool = False,
                           threads: int = 16, return_stats: bool = False):
    """``torontonian_table`` for loop torontonians (sup_loop_torontonian_table):
    entry ``mask`` = ``ltor`` of O and gamma on the list positions in ``mask``."""
    return _tor_table(O, gamma, modes, transform, device_id, cpu, threads, return_stats)


def subset_mobius(t, cpu: bool = False, device_id: int = 0, threads: int = 16):
    """The subset Moebius transform of a table of 2^n doubles
    (sup_mobius_subsets): out[S] = sum over Z in S of (-1)^(|S| - |Z|) t[Z], by
    the stages b = 0 .. n-1 ascending, ``t[z] -= t[z ^ (1 << b)]`` where z has
    bit b: one subtraction each, the same bits on the device (mobius.hip) and on
    host threads.  Returns a new array."""
    a = np.ascontiguousarray(np.asarray(t, dtype=np.float64)).reshape(-1).copy()
    n = int(a.shape[0]).bit_length() - 1
    if a.shape[0] < 1 or a.shape[0] != 1 << n:
        raise ValueError(f"expected 2^n values, got {a.shape[0]}")
    op = _opts(gpu_num=1, device_id=device_id, threads=threads)
    _lib.check(_lib.load().sup_mobius_subsets(a.ctypes.data, n, C.byref(op), int(bool(cpu))), "subset_mobius")
    return a


def _threshold_reduce(mu, cov, modes):
    """mu and cov (xxpp) of the listed modes alone: the others traced out."""
    cov = np.asarray(cov, dtype=np.float64)
    if cov.ndim != 2 or cov.shape[0] != cov.shape[1] or cov.shape[0] < 2 or cov.shape[0] % 2:
        raise ValueError(f"expected a 2M x 2M covariance matrix with M >= 1, got shape {cov.shape}")
    M = cov.shape[0] // 2
    if modes is None:
        return mu, cov
    m = np.asarray(modes, dtype=np.int64).reshape(-1)
    if m.size < 1 or np.any(m < 0) or np.any(m >= M) or np.unique(m).size != m.size:
        raise ValueError(f"modes must be distinct integers in [0, {M}), got {modes}")
    ix = np.concatenate([m, m + M])
    return (None if mu is None else np.asarray(mu, dtype=np.float64)[ix]), cov[np.ix_(ix, ix)]


def threshold_detection_distribution(mu, cov, modes=None, hbar: float = 2.0, **kw):
    """The probabilities of ALL 2^n click patterns of the listed modes (default:
    all M; the others are traced out) of the Gaussian state ``mu``, ``cov``
    (xxpp ordering) on threshold detectors, from one (loop) torontonian table:
    bit b of the index is the click on ``modes[b]``.  ``mu=None``: no
    displacement, through ``torontonian_table``.  ``kw`` goes to the table call
    (cpu, threads, device_id)."""
    mu_r, cov_r = _threshold_reduce(mu, cov, modes)
    O, gamma, pre = _threshold_setup(mu_r, cov_r, hbar)
    tab = torontonian_table(O, **kw) if gamma is None else loop_torontonian_table(O, gamma, **kw)
    return pre * tab


def threshold_detection_sample(mu, cov, nsamples: int, seed: int, modes=None, hbar: float = 2.0, **kw):
    """``nsamples`` exact click patterns (uint8 [nsamples, n], column b = the
    click on ``modes[b]``) of the state on threshold detectors, by the inverse
    CDF over ``threshold_detection_distribution``: negative roundings count as
    0, and the uniform numbers are ``numpy.random.default_rng(seed)``'s.  The
    samples are a function of the table's bits: the same on the device and
    with ``cpu=True``."""
    p = threshold_detection_distribution(mu, cov, modes=modes, hbar=hbar, **kw)
    n = int(p.shape[0]).bit_length() - 1
    cdf = np.cumsum(np.clip(p, 0.0, None))
    u = np.random.default_rng(seed).random(int(nsamples)) * cdf[-1]
    idx = np.minimum(np.searchsorted(cdf, u, side="right"), p.shape[0] - 1)
    return ((idx[:, None] >> np.arange(n)[None, :]) & 1).astype(np.uint8)


def _threshold_setup(mu, cov, hbar):
    """(O, gamma or None, prefactor) of a Gaussian state in xxpp ordering:
    W = [[I, iI], [I, -iI]] / sqrt 2, sigma = W cov W^H / hbar, Q = sigma + I / 2,
    alpha = W mu / sqrt hbar, O = I - Q^-1, gamma = Q^-1 alpha, prefactor =
    exp(-1/2 alpha^H Q^-1 alpha) / sqrt det Q."""
    cov = np.asarray(cov, dtype=np.float64)
    if cov.ndim != 2 or cov.shape[0] != cov.shape[1] or cov.shape[0] < 2 or cov.shape[0] % 2:
        raise ValueError(f"expected a 2M x 2M covariance matrix with M >= 1, got shape {cov.shape}")
    M = cov.shape[0] // 2
    I = np.eye(M)
    W = np.block([[I, 1j * I], [I, -1j * I]]) / np.sqrt(2.0)
    Q = W @ cov @ W.conj().T / float(hbar) + np.eye(2 * M) / 2.0
    Qi = np.linalg.inv(Q)
    Qi = (Qi + Qi.conj().T) / 2.0
    O = np.eye(2 * M) - Qi
    pre = 1.0 / np.sqrt(np.linalg.det(Q).real)
    if mu is None:
        return O, None, float(pre)
    mu = np.asarray(mu, dtype=np.float64)
    if mu.shape != (2 * M,):
        raise ValueError(f"mu must have the 2M = {2 * M} entries of cov's rows, got shape {mu.shape}")
    alpha = W @ mu / np.sqrt(float(hbar))
    gamma = Qi @ alpha
    return O, gamma, float(pre * np.exp(-0.5 * (alpha.conj() @ gamma).real))


def threshold_detection_probs(mu, cov, patterns, hbar: float = 2.0, **kw):
    """The probabilities of click patterns (shape [count, M] of 0 / 1, or one
    pattern of shape [M]) of the Gaussian state with mean ``mu`` and covariance
    ``cov`` (xxpp ordering, vacuum = hbar / 2) on threshold detectors: the
    prefactor times the loop torontonian on the clicked modes, one batched
    ``loop_torontonian_batch`` call per click count (numpy does the setup on
    the host).  ``mu=None``: no displacement, through ``torontonian_batch``
    and with its bits.  ``kw`` goes to the batch call (cpu, threads, gpu_num,
    device_id)."""
    O, gamma, pre = _threshold_setup(mu, cov, hbar)
    M = O.shape[0] // 2
    pat = np.asarray(patterns)
    single = pat.ndim == 1
    if single:
        pat = pat[None, :]
    if pat.ndim != 2 or pat.shape[1] != M or not np.all((pat == 0) | (pat == 1)):
        raise ValueError(f"patterns must be 0 / 1 with shape [M] or [count, M], M = {M}; got shape {np.shape(patterns)}")
    pat = pat.astype(bool)
    clicks = pat.sum(1)
    out = np.zeros(pat.shape[0])
    for k in np.unique(clicks):
        which = np.nonzero(clicks == k)[0]
        if k == 0:
            out[which] = pre  # the empty pattern: the prefactor alone
            continue
        modes = np.stack([np.nonzero(pat[i])[0] for i in which]).astype(np.int32)
        v = torontonian_batch(O, modes, **kw) if gamma is None else loop_torontonian_batch(O, gamma, modes, **kw)
        out[which] = pre * np.asarray(v)
    return float(out[0]) if single else out


def threshold_detection_prob(mu, cov, clicks, hbar: float = 2.0, **kw):
    """The probability of one click pattern (``threshold_detection_probs``)."""
    return threshold_detection_probs(mu, cov, np.asarray(clicks).reshape(-1), hbar=hbar, **kw)


def loop_hafnian_each(A, mus, lists, mu_of=None, gpu_num: int = 1, device_id: int = 0, cpu: bool = False,
                      threads: int = 16, return_stats: bool = False):
    """The loop hafnians of ragged gathers of one complex symmetric matrix A,
    each with its own displacement (sup_loop_hafnian_complex_each): item k is
    the loop hafnian of ``A[np.ix_(lists[k], lists[k])]`` with
    ``mus[mu_of[k]][lists[k]]`` on the diagonal (``mu_of=None``: row k).  The
    lists may differ in length (0..64) and may repeat; an empty list gives
    exactly 1.  One call is one queue on the device (walk_lhafe.hip) whatever
    the orders, and item k has the bits of ``hafnian_batch(A, lists[k],
    mu=mus[mu_of[k]], loop=True)``.  complex128 array of shape [count]."""
    a = np.ascontiguousarray(np.asarray(A, dtype=np.complex128))
    if a.ndim != 2 or a.shape[0] != a.shape[1] or a.shape[0] < 1:
        raise ValueError(f"expected a non-empty square matrix A, got shape {a.shape}")
    M = a.shape[0]
    m = np.ascontiguousarray(np.asarray(mus, dtype=np.complex128))
    if m.ndim == 1:
        m = m[None, :]
    if m.ndim != 2 or m.shape[1] != M or m.shape[0] < 1:
        raise ValueError(f"mus must have shape [nmu, {M}] with nmu >= 1, got {m.shape}")
    rows = [np.asarray(l).reshape(-1) for l in lists]
    count = len(rows)
    n32 = np.array([r.size for r in rows] + [0], dtype=np.int64)
    if n32.max() > 64:
        raise ValueError(f"a list has {int(n32.max())} entries, more than 64 (64-bit Gray index)")
    flat = np.concatenate([r for r in rows if r.size]) if n32.sum() else np.zeros(0, np.int64)
    if flat.size and not np.issubdtype(flat.dtype, np.integer):
        raise ValueError(f"lists must hold integers, got dtype {flat.dtype}")
    if flat.size and (flat.min() < -2**31 or flat.max() >= 2**31):
        raise ValueError("lists hold an index outside the 32-bit range")
    stride = max(int(n32.max()), 1)
    idx = np.zeros((max(count, 1), stride), np.int32)
    if flat.size:  # row k's entries at idx[k, :n[k]]
        first = np.cumsum(n32[:count]) - n32[:count]
        idx[np.repeat(np.arange(count), n32[:count]), np.arange(flat.size) - np.repeat(first, n32[:count])] = flat
    n32 = np.ascontiguousarray(n32[:max(count, 1)], dtype=np.int32)
    of = None
    if mu_of is not None:
        ofa = np.asarray(mu_of)
        if ofa.shape != (count,) or (count and not np.issubdtype(ofa.dtype, np.integer)):
            raise ValueError(f"mu_of must hold one integer per list, got shape {ofa.shape}")
        if count and (ofa.min() < -2**31 or ofa.max() >= 2**31):
            raise ValueError("mu_of holds a row outside the 32-bit range")
        of = np.ascontiguousarray(ofa, dtype=np.int32) if count else np.zeros(1, np.int32)
    lib = _lib.load()
    o = _opts(gpu_num=gpu_num, device_id=device_id, threads=threads)
    out, st = np.zeros(2 * max(count, 1)), SupStats()
    rc = lib.sup_loop_hafnian_complex_each(a.ctypes.data, M, m.ctypes.data, m.shape[0],
                                           None if of is None else of.ctypes.data, idx.ctypes.data, stride,
                                           n32.ctypes.data, count, C.byref(o), int(bool(cpu)), out.ctypes.data,
                                           C.byref(st))
    _lib.check(rc, "loop_hafnian_each")
    v = _batch_result(out, count)
    return (v, st.as_dict()) if return_stats else v


def gbs_pure_state(mu, cov, hbar: float = 2.0):
    """``(B, zeta, p0)`` of a pure Gaussian state with mean ``mu`` (or None) and
    covariance ``cov`` (xxpp ordering, vacuum = hbar / 2), from
    ``_threshold_setup``'s O, gamma and prefactor: with Abar = X O (X swaps the
    two M-blocks), B = Abar[M:, M:] (symmetrised), zeta = gamma[:M] and
    <n|psi> = sqrt(p0) lhaf(B gathered with n_i copies of i, zeta) /
    sqrt(prod n_i!) up to one global phase.  The state is pure exactly when the
    off-diagonal M x M blocks of Abar vanish: ValueError when they exceed 1e-8
    of max |Abar| (and 1e-14, the rounding of O = I - Q^-1 whose parts are of
    order one: the vacuum's Abar is nothing but that rounding)."""
    O, gamma, pre = _threshold_setup(mu, cov, hbar)
    M = O.shape[0] // 2
    # Abar = X O: the rows of O with the two blocks swapped
    off = max(np.abs(O[M:, M:]).max(), np.abs(O[:M, :M]).max())
    if off > max(1e-8 * np.abs(O).max(), 1e-14):
        raise ValueError(f"the state is not pure: the off-diagonal blocks of Abar reach {off:.3e}")
    B = O[:M, M:]
    B = np.ascontiguousarray((B + B.T) / 2.0)
    zeta = np.zeros(M, np.complex128) if gamma is None else np.ascontiguousarray(gamma[:M])
    return B, zeta, pre


def _pnr_patterns(patterns, M):
    pat = np.asarray(patterns)
    single = pat.ndim == 1
    if single:
        pat = pat[None, :]
    if pat.ndim != 2 or pat.shape[1] != M or (pat.size and not np.issubdtype(pat.dtype, np.integer)) or (pat < 0).any():
        raise ValueError(f"patterns must hold non-negative integers with shape [M] or [count, M], M = {M}; "
                         f"got shape {np.shape(patterns)}")
    return pat.astype(np.int64), single


def pnr_detection_probs(mu, cov, patterns, hbar: float = 2.0, **kw):
    """The probabilities of photon-number patterns (shape [count, M], or one
    pattern of shape [M]) of the Gaussian state with mean ``mu`` (or None) and
    covariance ``cov`` (xxpp ordering, vacuum = hbar / 2) on
    photon-number-resolving detectors.  A pure state (``gbs_pure_state``
    accepts it) takes one ragged ``loop_hafnian_each`` call at order N = the
    pattern's photon total: p = p0 |lhaf(B, zeta)|^2 / prod n_i!.  Any other
    state takes p = p0 lhaf(Abar, conj(gamma)) / prod n_i! on the list with i
    and i + M n_i times each, order 2N: one ``hafnian_batch`` call per photon
    total (``mu=None``: the plain hafnian).  The all-zero pattern is p0 alone.
    ``kw`` goes to those calls (cpu, threads, gpu_num, device_id)."""
    O, gamma, pre = _threshold_setup(mu, cov, hbar)
    M = O.shape[0] // 2
    pat, single = _pnr_patterns(patterns, M)
    tot = pat.sum(1)
    fac = np.array([float(np.prod([math.factorial(int(v)) for v in p])) for p in pat])
    out = np.zeros(pat.shape[0])
    try:
        B, zeta, _ = gbs_pure_state(mu, cov, hbar)
    except ValueError:
        B = None
    if B is not None:
        if tot.size and tot.max() > 64:
            raise ValueError(f"a pattern holds {int(tot.max())} photons, more than 64")
        lists = [np.repeat(np.arange(M), p) for p in pat]
        v = loop_hafnian_each(B, zeta[None, :], lists, mu_of=np.zeros(len(lists), np.int32), **kw)
        out = pre * (v.real * v.real + v.imag * v.imag) / fac
    else:
        if tot.size and tot.max() > 32:
            raise ValueError(f"a pattern holds {int(tot.max())} photons, more than 32 (order 2N <= 64)")
        Abar = np.concatenate([O[M:], O[:M]])
        Abar = np.ascontiguousarray((Abar + Abar.T) / 2.0)
        for N in np.unique(tot):
            which = np.nonzero(tot == N)[0]
            if N == 0:
                continue
            idx = np.stack([np.repeat(np.concatenate([np.arange(M), np.arange(M) + M]), np.concatenate([pat[i], pat[i]]))
                            for i in which]).astype(np.int32)
            if gamma is None:
                v = hafnian_batch(Abar, idx, **kw)
            else:
                v = hafnian_batch(Abar, idx, mu=np.conj(gamma), loop=True, **kw)
            out[which] = pre * np.asarray(v).real / fac[which]
    out[tot == 0] = pre  # the empty pattern: the prefactor alone
    return float(out[0]) if single else out


def pnr_detection_prob(mu, cov, pattern, hbar: float = 2.0, **kw):
    """The probability of one photon-number pattern (``pnr_detection_probs``)."""
    return pnr_detection_probs(mu, cov, np.asarray(pattern).reshape(-1), hbar=hbar, **kw)


# include/superman.h SUP_LHAF_TABLE_MAX_ENTRIES: the most entries a loop-hafnian
# table takes (2^27 complex values = 2 GiB), on the device and on host threads
LHAF_TABLE_MAX_ENTRIES = 1 << 27


def _lhaf_dims(dims, M=None):
    d = np.asarray(dims)
    if d.ndim == 0 and M is not None:  # a cutoff: photon numbers 0 .. cutoff on every mode
        d = np.full(M, int(d) + 1)
    d = d.reshape(-1)
    if d.size < 1 or not np.issubdtype(d.dtype, np.integer) or d.min() < -2**31 or d.max() >= 2**31:
        raise ValueError(f"dims must hold at least one 32-bit integer, got {dims}")
    if M is not None and d.size != M:
        raise ValueError(f"dims must hold one size per mode, M = {M}; got {d.size}")
    return np.ascontiguousarray(d, dtype=np.int32)


def loop_hafnian_table(A, mu, dims, cpu: bool = False, threads: int = 16, device_id: int = 0,
                       return_stats: bool = False):
    """Every normalised loop hafnian of A up to per-mode cutoffs from ONE
    recurrence (sup_loop_hafnian_table): a complex array of shape
    ``tuple(dims)`` with ``t[n_0, .., n_{M-1}] = lhaf(A gathered with n_i copies
    of i, mu) / sqrt(prod n_i!)`` for n_i < dims[i], the diagonal of A counting
    pairs of copies of one mode and ``mu`` on self-loops only.  ``mu=None``
    gives the hafnian table (odd photon totals are 0).  ``t[0, .., 0]`` is
    exactly 1.  The array is the Fortran-order view of the C buffer (mode 0
    fastest), no copy.  One device or (cpu=True) the host twin, bit-identical;
    prod dims <= ``LHAF_TABLE_MAX_ENTRIES``."""
    a = np.ascontiguousarray(np.asarray(A, dtype=np.complex128))
    if a.ndim != 2 or a.shape[0] != a.shape[1] or a.shape[0] < 1:
        raise ValueError(f"expected a non-empty square matrix A, got shape {a.shape}")
    M = a.shape[0]
    d = _lhaf_dims(dims, M)
    m = None
    if mu is not None:
        m = np.ascontiguousarray(np.asarray(mu, dtype=np.complex128))
        if m.shape != (M,):
            raise ValueError(f"mu must have shape [{M}], got {m.shape}")
    total = 1
    for v in d.tolist():
        total *= max(v, 0)
    # a refused call writes nothing: no buffer of the full size for it
    ok = M <= 64 and d.min() >= 1 and d.max() <= 65 and total <= LHAF_TABLE_MAX_ENTRIES
    out, st = np.zeros(total if ok else 1, np.complex128), SupStats()
    op = _opts(gpu_num=1, device_id=device_id, threads=threads)
    rc = _lib.load().sup_loop_hafnian_table(a.ctypes.data, M, None if m is None else m.ctypes.data, d.ctypes.data,
                                            C.byref(op), int(bool(cpu)), out.ctypes.data, C.byref(st))
    _lib.check(rc, "loop_hafnian_table")
    t = out.reshape(tuple(d.tolist()), order="F")
    if not return_stats:
        return t
    s = st.as_dict()
    s["launches"] = int(st.partials[0])
    return t, s


def loop_hafnian_table_plan(dims):
    """``(entries, launches, ops_per_entry)`` of ``loop_hafnian_table`` at
    ``dims`` (sup_loop_hafnian_table_plan, host only): prod dims, the kernel
    launches of the device path and the fp64 operations per entry."""
    d = _lhaf_dims(dims)
    e, l, ops = C.c_uint64(0), C.c_uint64(0), C.c_double(0.0)
    _lib.check(_lib.load().sup_loop_hafnian_table_plan(d.ctypes.data, d.size, C.byref(e), C.byref(l), C.byref(ops)),
               "loop_hafnian_table_plan")
    return int(e.value), int(l.value), float(ops.value)


def gbs_state_vector(mu, cov, dims_or_cutoff, hbar: float = 2.0, **kw):
    """The Fock amplitudes ``psi[n_0, .., n_{M-1}]``, n_i < dims[i] (or <= an
    integer cutoff), of the pure Gaussian state ``mu`` (or None), ``cov`` (xxpp
    ordering): sqrt(p0) times ``loop_hafnian_table`` of ``gbs_pure_state``'s B
    and zeta, up to one global phase.  Mixed states raise ValueError as
    ``gbs_pure_state`` does.  ``kw`` goes to the table call (cpu, threads,
    device_id)."""
    B, zeta, p0 = gbs_pure_state(mu, cov, hbar)
    d = _lhaf_dims(dims_or_cutoff, B.shape[0])
    return np.sqrt(p0) * loop_hafnian_table(B, None if mu is None else zeta, d, **kw)


def gbs_density_matrix(mu, cov, dims_or_cutoff, hbar: float = 2.0, **kw):
    """The density matrix of ANY Gaussian state in the Fock basis up to the
    cutoffs: an array of 2M axes of shape dims + dims, ``rho[n_0, .., n_{M-1},
    m_0, .., m_{M-1}] = <n| rho |m>``, from one ``loop_hafnian_table`` of the
    2M x 2M Abar and conj(gamma) of ``pnr_detection_probs`` at dims + dims, times
    p0.  A pure state gives psi psi^dagger of ``gbs_state_vector``.  ValueError
    when prod dims^2 exceeds ``LHAF_TABLE_MAX_ENTRIES``."""
    O, gamma, pre = _threshold_setup(mu, cov, hbar)
    M = O.shape[0] // 2
    d = _lhaf_dims(dims_or_cutoff, M)
    if d.min() >= 1:
        D = 1
        for v in d.tolist():
            D *= v
        if D * D > LHAF_TABLE_MAX_ENTRIES:
            raise ValueError(f"a density matrix at dims {tuple(d.tolist())} has {D}^2 = {D * D} entries, more than "
                             f"LHAF_TABLE_MAX_ENTRIES = {LHAF_TABLE_MAX_ENTRIES}")
    Abar = np.concatenate([O[M:], O[:M]])
    Abar = np.ascontiguousarray((Abar + Abar.T) / 2.0)
    t = loop_hafnian_table(Abar, None if gamma is None else np.conj(gamma), np.concatenate([d, d]), **kw)
    # Abar's second block is gbs_pure_state's B: its axes are the ket's
    return pre * np.transpose(t, list(range(M, 2 * M)) + list(range(M)))


def pnr_detection_distribution(mu, cov, dims_or_cutoff, modes=None, hbar: float = 2.0, **kw):
    """The joint photon-number distribution ``p[n_0, .., n_{k-1}]``, n_i <
    dims[i] (or <= an integer cutoff), of the listed modes (default: all M; the
    others are traced out first, as ``threshold_detection_distribution`` does)
    on photon-number-resolving detectors.  A pure state takes |psi|^2 of
    ``gbs_state_vector``; any other state the diagonal of
    ``gbs_density_matrix``.  1 - p.sum() is the mass above the cutoffs."""
    mu_r, cov_r = _threshold_reduce(mu, cov, modes)
    try:
        psi = gbs_state_vector(mu_r, cov_r, dims_or_cutoff, hbar=hbar, **kw)
    except ValueError as e:
        if "not pure" not in str(e):
            raise
        psi = None
    if psi is not None:
        return psi.real * psi.real + psi.imag * psi.imag
    rho = gbs_density_matrix(mu_r, cov_r, dims_or_cutoff, hbar=hbar, **kw)
    k = rho.ndim // 2
    D = int(np.prod(rho.shape[:k]))
    return np.ascontiguousarray(rho.reshape(D, D, order="F").diagonal().real).reshape(rho.shape[:k], order="F")


def pnr_detection_sample(mu, cov, nsamples: int, seed: int, dims_or_cutoff, return_missing: bool = False, modes=None,
                         hbar: float = 2.0, **kw):
    """``nsamples`` exact photon-number patterns (int32 [nsamples, k]) from
    ``pnr_detection_distribution`` renormalised over the table, by the inverse
    CDF in the C buffer's order (mode 0 fastest): negative roundings count as 0,
    and the uniform numbers are ``numpy.random.default_rng(seed)``'s.  The
    samples are a function of the table's bits: the same on the device and with
    ``cpu=True``.  ``return_missing=True`` also gives 1 - sum p, the mass above
    the cutoffs that the renormalisation spreads."""
    p = pnr_detection_distribution(mu, cov, dims_or_cutoff, modes=modes, hbar=hbar, **kw)
    flat = np.clip(p.reshape(-1, order="F"), 0.0, None)
    cdf = np.cumsum(flat)
    u = np.random.default_rng(seed).random(int(nsamples)) * cdf[-1]
    idx = np.minimum(np.searchsorted(cdf, u, side="right"), flat.shape[0] - 1)
    pat = np.stack(np.unravel_index(idx, p.shape, order="F"), axis=1).astype(np.int32)
    return (pat, float(1.0 - flat.sum())) if return_missing else pat


def gbs_sample_chain(B, zeta, het, seed: int, cutoff: int = 8, sample0: int = 0, gpu_num: int = 1, device_id: int = 0,
                     cpu: bool = False, threads: int = 16, return_stats: bool = False):
    """The deterministic part of the PNR sampler (sup_gbs_sample): the chain
    rule over the modes for the pure state ``B`` (M x M symmetric), ``zeta``
    ([nsamples, M], or [M] for every sample) and the heterodyne outcomes ``het``
    ([nsamples, M] complex).  Every mode step is one ragged loop-hafnian call
    per batch of samples.  Row s depends on (B, zeta[s], het[s], cutoff, seed,
    sample0 + s) only.  int32 [nsamples, M]; -1 from the mode on at which a
    sample's weights summed to zero or to a non-finite value."""
    b = np.ascontiguousarray(np.asarray(B, dtype=np.complex128))
    if b.ndim != 2 or b.shape[0] != b.shape[1] or b.shape[0] < 1:
        raise ValueError(f"expected a non-empty square matrix B, got shape {b.shape}")
    M = b.shape[0]
    h = np.ascontiguousarray(np.asarray(het, dtype=np.complex128))
    if h.ndim != 2 or h.shape[1] != M:
        raise ValueError(f"het must have shape [nsamples, {M}], got {h.shape}")
    ns = h.shape[0]
    z = np.asarray(zeta, dtype=np.complex128)
    if z.shape == (M,):
        z = np.broadcast_to(z, (ns, M))
    if z.shape != (ns, M):
        raise ValueError(f"zeta must have shape [{M}] or [{ns}, {M}], got {z.shape}")
    z = np.ascontiguousarray(z)
    if sample0 < 0:
        raise ValueError("sample0 must be >= 0")
    lib = _lib.load()
    o = _opts(gpu_num=gpu_num, device_id=device_id, threads=threads)
    out, st = np.zeros((max(ns, 1), M), np.int32), SupStats()
    hp = h.ctypes.data if ns else out.ctypes.data
    zp = z.ctypes.data if ns else out.ctypes.data
    _lib.check(lib.sup_gbs_sample(b.ctypes.data, M, zp, hp, int(cutoff), ns, int(sample0),
                                  int(seed) & 0xFFFFFFFFFFFFFFFF, C.byref(o), int(bool(cpu)), out.ctypes.data,
                                  C.byref(st)), "gbs_sample")
    v = out[:ns].copy()
    if not return_stats:
        return v
    d = st.as_dict()
    d["each_ms"], d["host_ms"], d["failed"] = float(st.partials[0]), float(st.partials[1]), int(st.partials[2])
    return v, d


def gbs_sample(mu, cov, nsamples: int, seed: int, cutoff: int = 8, hbar: float = 2.0, sample0: int = 0, **kw):
    """``nsamples`` photon-number patterns (int32 [nsamples, M]) of the pure
    Gaussian state ``mu`` (or None), ``cov`` (xxpp ordering) on
    photon-number-resolving detectors, by the chain rule of Bulmer et al. 2022:
    the heterodyne outcomes are ``numpy.random.default_rng(seed)
    .standard_normal((sample0 + nsamples, 2M))`` times the Cholesky factor of
    cov + (hbar / 2) I plus the mean, rows [sample0, sample0 + nsamples), and
    the rest is ``gbs_sample_chain``.  Mode k is drawn from its conditional law
    renormalised over 0..cutoff: the only approximation, exact as the cutoff
    grows.  Mixed states raise ValueError (``gbs_pure_state``).  The same
    samples on the device and with ``cpu=True``; rows drawn in pieces with
    ``sample0`` equal the whole run's.  ``kw`` goes to ``gbs_sample_chain``."""
    B, zeta, _ = gbs_pure_state(mu, cov, hbar)
    het = _gbs_heterodyne(mu, cov, B.shape[0], nsamples, seed, hbar, sample0)
    return gbs_sample_chain(B, zeta, het, seed, cutoff=cutoff, sample0=int(sample0), **kw)


def _gbs_heterodyne(mu, cov, M, nsamples, seed, hbar, sample0):
    """Rows [sample0, sample0 + nsamples) of the heterodyne outcomes the chain
    rule samplers condition on: ``numpy.random.default_rng(seed)
    .standard_normal((sample0 + nsamples, 2M))`` times the Cholesky factor of
    cov + (hbar / 2) I plus the mean, as complex amplitudes [nsamples, M]."""
    nsamples, sample0 = int(nsamples), int(sample0)
    if nsamples < 0 or sample0 < 0:
        raise ValueError("nsamples and sample0 must be >= 0")
    V = np.asarray(cov, dtype=np.float64)
    L = np.linalg.cholesky(V + (float(hbar) / 2.0) * np.eye(2 * M))
    g = np.random.default_rng(seed).standard_normal((sample0 + nsamples, 2 * M))[sample0:]
    xp = g @ L.T
    if mu is not None:
        xp = xp + np.asarray(mu, dtype=np.float64)[None, :]
    return (xp[:, :M] + 1j * xp[:, M:]) / np.sqrt(2.0 * float(hbar))


def loop_torontonian_each(O, gammas, lists, gamma_of=None, gpu_num: int = 1, device_id: int = 0, cpu: bool = False,
                          threads: int = 16, return_stats: bool = False):
    """The loop torontonians of ragged lists of distinct modes of one 2M x 2M
    Hermitian matrix O, each with its own displacement
    (sup_loop_torontonian_each): item k is ``loop_torontonian_batch(O,
    gammas[gamma_of[k]], lists[k])`` (``gamma_of=None``: row k), bit for bit.
    ``gammas`` has shape [ngamma, 2M] (or [2M]: one row).  The lists may differ
    in length (0..32); an empty list gives exactly 1.  One call is one queue on
    the device (walk_ltore in walk_ltor.hip) whatever the orders.  float64 array
    of shape [count]."""
    o = _tor_matrix(O)
    g = np.ascontiguousarray(np.asarray(gammas, dtype=np.complex128))
    if g.ndim == 1:
        g = g[None, :]
    if g.ndim != 2 or g.shape[1] != o.shape[0] or g.shape[0] < 1:
        raise ValueError(f"gammas must have shape [ngamma, {o.shape[0]}] with ngamma >= 1, got {g.shape}")
    rows = [np.asarray(l).reshape(-1) for l in lists]
    count = len(rows)
    n32 = np.array([r.size for r in rows] + [0], dtype=np.int64)
    flat = np.concatenate([r for r in rows if r.size]) if n32.sum() else np.zeros(0, np.int64)
    if flat.size and not np.issubdtype(flat.dtype, np.integer):
        raise ValueError(f"lists must hold integers, got dtype {flat.dtype}")
    if flat.size and (flat.min() < -2**31 or flat.max() >= 2**31):
        raise ValueError("lists hold a mode outside the 32-bit range")
    stride = max(int(n32.max()), 1)
    idx = np.zeros((max(count, 1), stride), np.int32)
    if flat.size:  # row k's entries at idx[k, :n[k]]
        first = np.cumsum(n32[:count]) - n32[:count]
        idx[np.repeat(np.arange(count), n32[:count]), np.arange(flat.size) - np.repeat(first, n32[:count])] = flat
    n32 = np.ascontiguousarray(n32[:max(count, 1)], dtype=np.int32)
    of = None
    if gamma_of is not None:
        ofa = np.asarray(gamma_of)
        if ofa.shape != (count,) or (count and not np.issubdtype(ofa.dtype, np.integer)):
            raise ValueError(f"gamma_of must hold one integer per list, got shape {ofa.shape}")
        if count and (ofa.min() < -2**31 or ofa.max() >= 2**31):
            raise ValueError("gamma_of holds a row outside the 32-bit range")
        of = np.ascontiguousarray(ofa, dtype=np.int32) if count else np.zeros(1, np.int32)
    lib = _lib.load()
    op = _opts(gpu_num=gpu_num, device_id=device_id, threads=threads)
    out, st = np.zeros(max(count, 1)), SupStats()
    rc = lib.sup_loop_torontonian_each(o.ctypes.data, o.shape[0] // 2, g.ctypes.data, g.shape[0],
                                       None if of is None else of.ctypes.data, idx.ctypes.data, stride, n32.ctypes.data,
                                       count, C.byref(op), int(bool(cpu)), out.ctypes.data, C.byref(st))
    _lib.check(rc, "loop_torontonian_each")
    v = out[:count].copy()
    return (v, st.as_dict()) if return_stats else v


def threshold_sample_chain(B, zeta, het, seed: int, sample0: int = 0, return_weights: bool = False, gpu_num: int = 1,
                           device_id: int = 0, cpu: bool = False, threads: int = 16, return_stats: bool = False):
    """The deterministic part of the threshold-detector sampler
    (sup_threshold_sample): the chain rule over the modes for the pure state
    ``B`` (M x M symmetric), ``zeta`` ([nsamples, M], or [M] for every sample)
    and the heterodyne outcomes ``het`` ([nsamples, M] complex).  Every mode step
    is one ragged loop torontonian call of two items per sample of a batch: the
    clicks so far without and with the mode.  Row s depends on (B, zeta[s],
    het[s], seed, sample0 + s) only.  int32 [nsamples, M] of 0 / 1; -1 from the
    mode on at which a sample's two weights summed to zero or to a non-finite
    value or its list would pass 32 modes.  ``return_weights=True`` adds the
    float64 array [nsamples, M, 2] of (w_0, w_1) as used; ``return_stats=True``
    the statistics, last."""
    b = np.ascontiguousarray(np.asarray(B, dtype=np.complex128))
    if b.ndim != 2 or b.shape[0] != b.shape[1] or b.shape[0] < 1:
        raise ValueError(f"expected a non-empty square matrix B, got shape {b.shape}")
    M = b.shape[0]
    h = np.ascontiguousarray(np.asarray(het, dtype=np.complex128))
    if h.ndim != 2 or h.shape[1] != M:
        raise ValueError(f"het must have shape [nsamples, {M}], got {h.shape}")
    ns = h.shape[0]
    z = np.asarray(zeta, dtype=np.complex128)
    if z.shape == (M,):
        z = np.broadcast_to(z, (ns, M))
    if z.shape != (ns, M):
        raise ValueError(f"zeta must have shape [{M}] or [{ns}, {M}], got {z.shape}")
    z = np.ascontiguousarray(z)
    if sample0 < 0:
        raise ValueError("sample0 must be >= 0")
    lib = _lib.load()
    o = _opts(gpu_num=gpu_num, device_id=device_id, threads=threads)
    out, st = np.zeros((max(ns, 1), M), np.int32), SupStats()
    w = np.zeros((max(ns, 1), M, 2)) if return_weights else None
    hp = h.ctypes.data if ns else out.ctypes.data
    zp = z.ctypes.data if ns else out.ctypes.data
    _lib.check(lib.sup_threshold_sample(b.ctypes.data, M, zp, hp, ns, int(sample0), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                        C.byref(o), int(bool(cpu)), out.ctypes.data,
                                        None if w is None else w.ctypes.data, C.byref(st)), "threshold_sample")
    res = [out[:ns].copy()]
    if return_weights:
        res.append(w[:ns].copy())
    if return_stats:
        d = st.as_dict()
        d["each_ms"], d["host_ms"], d["failed"] = float(st.partials[0]), float(st.partials[1]), int(st.partials[2])
        res.append(d)
    return res[0] if len(res) == 1 else tuple(res)


def threshold_sample(mu, cov, nsamples: int, seed: int, hbar: float = 2.0, sample0: int = 0, **kw):
    """``nsamples`` click patterns (int32 [nsamples, M] of 0 / 1) of the pure
    Gaussian state ``mu`` (or None), ``cov`` (xxpp ordering) on threshold
    detectors, by the chain rule of Bulmer et al. 2022 with loop torontonians
    for the two outcomes of a mode: exact, and not bounded by a table's 28
    modes (a sample may click on 32 modes at most).  The heterodyne outcomes
    are ``gbs_sample``'s for the same seed; the rest is
    ``threshold_sample_chain``.  Mixed states raise ValueError
    (``gbs_pure_state``).  The same samples on the device and with
    ``cpu=True``; rows drawn in pieces with ``sample0`` equal the whole run's.
    ``kw`` goes to ``threshold_sample_chain``."""
    B, zeta, _ = gbs_pure_state(mu, cov, hbar)
    het = _gbs_heterodyne(mu, cov, B.shape[0], nsamples, seed, hbar, sample0)
    return threshold_sample_chain(B, zeta, het, seed, sample0=int(sample0), **kw)


def partial(mat, start: int, end: int, kernel: str = "dense", gpu_num: int = 1, device_id: int = 0,
            walk_log2: int = 0, return_stats: bool = False):
    """GPU partial Ryser sum over reference Gray indices [start, end) (index 0 = p0 term)."""
    a, dt, n = _mat(mat)
    lib = _lib.load()
    o = _opts(gpu_num=gpu_num, device_id=device_id, walk_log2=walk_log2)
    out, st = C.c_double(0.0), SupStats()
    _lib.check(lib.sup_partial(a.ctypes.data, dt, n, _KERNELS[kernel], int(start), int(end), C.byref(o),
                               C.byref(out), C.byref(st)), "partial")
    return (out.value, st.as_dict()) if return_stats else out.value


def perman_shard(mat, shard: int, nshards: int, kernel: str = "dense", device_id: int = 0,
                 return_stats: bool = False, jit: int = 0, walk_log2: int = 0):
    """Partial sum of shard `shard` of `nshards` of the engine's enumeration
    (one process per GPU): the shards add up to perm / (4(n&1)-2)."""
    a, dt, n = _mat(mat)
    lib = _lib.load()
    o = _opts(device_id=device_id, jit=jit, walk_log2=walk_log2)
    out, st = C.c_double(0.0), SupStats()
    _lib.check(lib.sup_perman_shard(a.ctypes.data, dt, n, _KERNELS[kernel], int(shard), int(nshards), C.byref(o),
                                    C.byref(out), C.byref(st)), "perman_shard")
    return (out.value, st.as_dict()) if return_stats else out.value


class ShardCall:
    """perman_shard prepared once — the matrix conversion, options and result
    structs built ahead, so a repeated call (the bench's timed step, one rank's
    shard per step) costs the C-ABI call itself: call() -> (partial, walk
    kernel ms); stats() -> the last call's sup_stats."""

    def __init__(self, mat, shard: int, nshards: int, kernel: str = "dense", device_id: int = 0, jit: int = 0,
                 walk_log2: int = 0, timing: bool = True):
        self._a, dt, n = _mat(mat)
        self._lib = _lib.load()
        self._o = _opts(device_id=device_id, jit=jit, walk_log2=walk_log2)
        # timing=False: the walk's HIP events are read later by kernel_time()
        # (the call returns as soon as its result is there; kernel ms 0)
        self._o.timing = int(bool(timing))
        self._out, self._st = C.c_double(0.0), SupStats()
        self._fn = self._lib.sup_perman_shard
        self._args = (self._a.ctypes.data, dt, n, _KERNELS[kernel], int(shard), int(nshards), C.byref(self._o),
                      C.byref(self._out), C.byref(self._st))

    def __call__(self):
        rc = self._fn(*self._args)
        if rc:
            _lib.check(rc, "perman_shard")
        return self._out.value, self._st.kernel_ms

    def stats(self) -> dict:
        return self._st.as_dict()


def kernel_time(device_id: int = 0):
    """(total ms, launches) of this thread's walk kernels on `device_id` since
    the last call, from ShardCall(..., timing=False) calls (sup_kernel_time:
    their HIP events, read now)."""
    lib = _lib.load()
    ms, cnt = C.c_double(0.0), C.c_uint64(0)
    _lib.check(lib.sup_kernel_time(int(device_id), C.byref(ms), C.byref(cnt)), "kernel_time")
    return ms.value, cnt.value


def plan_info(mat, kernel: str = "dense", jit: int = 0, gpu_num: int = 1, device_id: int = 0,
              walk_log2: int = 0) -> dict:
    """The plan the engine runs for `kernel` (and options jit / gpu_num): walk
    kind, column map, layout, cost model (fp64 ops per Gray step), cached walk
    bits and specialised pair bits of the segmented walk.  A SkipPer
    plan may sample its visited fraction on device `device_id`."""
    a, dt, n = _mat(mat)
    lib = _lib.load()
    kind, L, m, cc, pb = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_int()
    ops = C.c_double(0.0)
    cm = np.zeros(max(n - 1, 1), np.int32)
    o = _opts(gpu_num=gpu_num, device_id=device_id, jit=jit, walk_log2=walk_log2)
    _lib.check(lib.sup_plan_info(a.ctypes.data, dt, n, _KERNELS[kernel], C.byref(o), C.byref(kind), cm.ctypes.data,
                                 C.byref(L), C.byref(m), C.byref(cc), C.byref(pb), C.byref(ops)), "plan_info")
    return {"kind": WALK_NAMES[kind.value], "colmap": cm[: n - 1].copy(), "L": L.value, "m": m.value,
            "cached": cc.value, "pair_bits": pb.value, "est_ops_per_step": ops.value}


CENSUS_CLASSES = ("x_adds", "copy_adds", "outer_forms", "inner_forms", "d_fmas", "accumulates", "lane_sum",
                  "shared_adds", "shared_copies", "shared_forms", "hi_adds", "hi_copies", "hi_forms")


def plan_census(mat, kernel: str = "dense", jit: int = 0, gpu_num: int = 1, device_id: int = 0,
                walk_log2: int = 0) -> dict:
    """Op census of the plan plan_info describes (sup_plan_census): fp64 ops per
    Gray step of the segmented walk's generated kernel by class ("classes": an
    ordered dict over CENSUS_CLASSES, the walk loop, whose values added in
    order give plan_info's est_ops_per_step exactly), "chunk_start" (the chunk
    start and end amortised per Gray step, beside that sum) and "hi_bits", the
    walk bits above the specialised pair bits that have straight-line steps of
    their own."""
    a, dt, n = _mat(mat)
    lib = _lib.load()
    hi = C.c_int()
    cen = np.zeros(len(CENSUS_CLASSES) + 1, np.float64)
    o = _opts(gpu_num=gpu_num, device_id=device_id, jit=jit, walk_log2=walk_log2)
    _lib.check(lib.sup_plan_census(a.ctypes.data, dt, n, _KERNELS[kernel], C.byref(o), C.byref(hi), cen.ctypes.data),
               "plan_census")
    return {"hi_bits": hi.value, "classes": dict(zip(CENSUS_CLASSES, (float(v) for v in cen))),
            "chunk_start": float(cen[-1])}


def plan_key(mat, kernel: str = "dense", jit: int = 0, gpu_num: int = 1, device_id: int = 0,
             walk_log2: int = 0) -> int:
    """64-bit fingerprint of the plan perman / perman_shard would run
    (sup_plan_key): ranks that plan on their own must agree on it before their
    shards are summed."""
    a, dt, n = _mat(mat)
    lib = _lib.load()
    key = C.c_uint64(0)
    o = _opts(gpu_num=gpu_num, device_id=device_id, jit=jit, walk_log2=walk_log2)
    _lib.check(lib.sup_plan_key(a.ctypes.data, dt, n, _KERNELS[kernel], C.byref(o), C.byref(key)), "plan_key")
    return key.value


def prepare(mat, kernel: str = "dense", jit: int = 0, gpu_num: int = 1, device_id: int = 0,
            walk_log2: int = 0) -> dict:
    """Plan `mat` as perman / perman_shard would and compile the segmented
    walk's specialised kernel now if the plan uses it (hiprtc, no device
    needed): {"kind": walk name, "compile_ms": hiprtc time (0 when cached)}.
    Planning work that needs a device (SkipPer's sample) runs on `device_id`."""
    a, dt, n = _mat(mat)
    lib = _lib.load()
    kind, ms = C.c_int(), C.c_double(0.0)
    o = _opts(gpu_num=gpu_num, device_id=device_id, jit=jit, walk_log2=walk_log2)
    _lib.check(lib.sup_prepare(a.ctypes.data, dt, n, _KERNELS[kernel], C.byref(o), C.byref(kind), C.byref(ms)),
               "prepare")
    return {"kind": WALK_NAMES[kind.value], "compile_ms": ms.value}


def nw_start(mat) -> tuple[np.ndarray, float]:
    a, dt, n = _mat(mat)
    lib = _lib.load()
    x0 = np.zeros(n, np.float64)
    p0 = C.c_double(0.0)
    _lib.check(lib.sup_nw_start(a.ctypes.data, dt, n, x0.ctypes.data_as(C.POINTER(C.c_double)), C.byref(p0)),
               "nw_start")
    return x0, p0.value


def read_matrix(path: str, binary: bool = False) -> tuple[np.ndarray, str, int]:
    """v1 matrix file -> (matrix, type name, nnz from the header) (util.h:343-358).
    MatrixMarket files (detected by their banner) are read as by read_mtx."""
    lib = _lib.load()
    p, t, n, nnz = C.c_void_p(), C.c_int(), C.c_int(), C.c_int()
    _lib.check(lib.sup_read_matrix(path.encode(), int(bool(binary)), C.byref(p), C.byref(t), C.byref(n),
                                   C.byref(nnz)), "read_matrix")
    try:
        dtype = _NP[t.value]
        buf = (C.c_char * (n.value * n.value * np.dtype(dtype).itemsize)).from_address(p.value)
        m = np.frombuffer(buf, dtype=dtype).reshape(n.value, n.value).copy()
    finally:
        lib.sup_free(p)
    return m, _TYPE_NAME[t.value], nnz.value


def sort_order(mat) -> tuple[np.ndarray, np.ndarray]:
    """SortOrder (util.h:553-619): returns (permuted matrix, colperm)."""
    a, dt, n = _mat(mat)
    a = a.copy()
    cp = np.zeros(n, np.int32)
    _lib.check(_lib.load().sup_sort_order(a.ctypes.data, dt, n, cp.ctypes.data), "sort_order")
    return a, cp


def skip_order(mat) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """SkipOrder (util.h:621-684): returns (permuted matrix, rowperm, colperm)."""
    a, dt, n = _mat(mat)
    a = a.copy()
    rp, cp = np.zeros(n, np.int32), np.zeros(n, np.int32)
    _lib.check(_lib.load().sup_skip_order(a.ctypes.data, dt, n, rp.ctypes.data, cp.ctypes.data), "skip_order")
    return a, rp, cp


def compress(mat) -> dict:
    """CSR + CSC with the != 0 nonzero test (util.h:522-551)."""
    a, dt, n = _mat(mat)
    lib = _lib.load()
    nnz = C.c_int(0)
    _lib.check(lib.sup_count_nnz(a.ctypes.data, dt, n, C.byref(nnz)), "count_nnz")
    k = max(nnz.value, 1)
    out = {"cptrs": np.zeros(n + 1, np.int32), "rows": np.zeros(k, np.int32), "cvals": np.zeros(k, a.dtype),
           "rptrs": np.zeros(n + 1, np.int32), "cols": np.zeros(k, np.int32), "rvals": np.zeros(k, a.dtype)}
    _lib.check(lib.sup_compress(a.ctypes.data, dt, n, *(out[f].ctypes.data for f in
                                                        ("cptrs", "rows", "cvals", "rptrs", "cols", "rvals"))),
               "compress")
    for f in ("rows", "cvals", "cols", "rvals"):
        out[f] = out[f][: nnz.value]
    return out


# ---- reference-named wrappers (gpu_exact_dense.cu / gpu_exact_sparse.cu) -----------
def gpu_perman64_xshared_coalescing_mshared(mat, grid_dim=2048, block_dim=256):
    return perman(mat, 4)


def gpu_perman64_xshared_coalescing_mshared_multigpu(mat, gpu_num, grid_dim=2048, block_dim=256):
    return perman(mat, 5, gpu_num=gpu_num)


def gpu_perman64_xshared_coalescing_mshared_multigpucpu_chunks(mat, gpu_num, cpu=False, threads=16,
                                                               grid_dim=2048, block_dim=256):
    return perman(mat, 6, gpu_num=gpu_num, cpu=cpu, threads=threads)


def gpu_perman64_xshared_coalescing_mshared_sparse(mat, grid_dim=2048, block_dim=256):
    return perman(mat, 4, sparse=True)


def gpu_perman64_xshared_coalescing_mshared_multigpu_sparse(mat, gpu_num, grid_dim=2048, block_dim=256):
    return perman(mat, 5, sparse=True, gpu_num=gpu_num)


def gpu_perman64_xshared_coalescing_mshared_multigpucpu_chunks_sparse(mat, gpu_num, cpu=False, threads=16,
                                                                      grid_dim=2048, block_dim=256):
    return perman(mat, 6, sparse=True, gpu_num=gpu_num, cpu=cpu, threads=threads)


def gpu_perman64_xshared_coalescing_mshared_skipper(mat, grid_dim=2048, block_dim=256):
    return perman(mat, 7, sparse=True)


def gpu_perman64_xshared_coalescing_mshared_multigpucpu_chunks_skipper(mat, gpu_num, cpu=False, threads=16,
                                                                       grid_dim=2048, block_dim=256):
    return perman(mat, 8, sparse=True, gpu_num=gpu_num, cpu=cpu, threads=threads)


def _reduce_opts(compress=True, scale=None, min_n=30, max_deg=5, preprocessing=0) -> SupReduceOpts:
    lib = _lib.load()
    r = SupReduceOpts()
    lib.sup_reduce_opts_init(C.byref(r))
    r.compress = int(bool(compress))
    r.scale_threshold = float(scale) if scale else 0.0
    r.min_n, r.max_deg, r.preprocessing = int(min_n), int(max_deg), int(preprocessing)
    return r


def decompose(mat, leaf, compress: bool = True, scale=None, min_n: int = 30, max_deg: int = 5):
    """Reductions of the reference's -o / -u (revised_perman/main.cpp:993-1264)
    with a Python leaf function: returns (perm, leaves) where perm combines
    leaf(A_leaf) over the d1/d2/d34 expansion tree and divides scale factors
    out, and leaves lists every leaf matrix handed to `leaf`."""
    a, dt, n = _mat(mat, 4096)
    lib = _lib.load()
    seen, err = [], []

    def cb(ptr, k, _user, out):
        try:
            m = np.ctypeslib.as_array(ptr, shape=(k * k,)).reshape(k, k).copy()
            seen.append(m)
            out[0] = float(leaf(m))
            return 0
        except Exception as e:  # surfaced after the C call returns
            err.append(e)
            return -1

    fn = LEAF_FN(cb)
    r = _reduce_opts(compress, scale, min_n, max_deg)
    out, nl = C.c_double(0.0), C.c_int(0)
    rc = lib.sup_decompose(a.ctypes.data, dt, n, C.byref(r), fn, None, C.byref(out), C.byref(nl))
    if err:
        raise err[0]
    _lib.check(rc, "decompose")
    return out.value, seen


def perman_reduced(mat, algo: int = 4, sparse: bool = False, compress: bool = True, scale=None,
                   preprocessing: int = 0, gpu_num: int = 1, cpu: bool = False, threads: int = 16,
                   device_id: int = 0, min_n: int = 30, max_deg: int = 5, return_stats: bool = False):
    """-o / -u front end: reduce the matrix, then run the algorithm `algo` on
    every leaf (after -r `preprocessing`) on the GPU, or on host threads with
    cpu=True (the CLI's -c)."""
    table = ALGOS_SPARSE if sparse else ALGOS_DENSE
    if algo not in table:
        raise SupError(-7, "perman_reduced", f"unknown algorithm id {algo}")
    _, kernel, sched = table[algo]
    if sched == SCHED_SINGLE:
        gpu_num = 1
    a, dt, n = _mat(mat, 4096)
    lib = _lib.load()
    o = _opts(gpu_num, device_id, threads)
    r = _reduce_opts(compress, scale, min_n, max_deg, preprocessing)
    out, st = C.c_double(0.0), SupStats()
    _lib.check(lib.sup_perman_reduced(a.ctypes.data, dt, n, kernel, sched, C.byref(o), int(bool(cpu)), C.byref(r),
                                      C.byref(out), C.byref(st)), "perman_reduced")
    return (out.value, st.as_dict()) if return_stats else out.value


def perman_reduced_exact(mat, cpu: bool = False, threads: int = 16, device_id: int = 0, gpu_num: int = 1,
                         min_n: int = 30, max_deg: int = 5, return_stats: bool = False):
    """-o with exact leaves (sup_perman_reduced_exact): the d1/d2/d34 tree folds
    every coefficient into its integer leaves, so the permanent is the exact
    sum of their exact permanents (Python int)."""
    a, dt, n = _mat(mat, 4096)
    lib = _lib.load()
    o = _opts(gpu_num, device_id, threads)
    r = _reduce_opts(True, None, min_n, max_deg)
    buf = C.create_string_buffer(1 << 16)
    st = SupStats()
    _lib.check(lib.sup_perman_reduced_exact(a.ctypes.data, dt, n, C.byref(o), int(bool(cpu)), C.byref(r), buf,
                                            len(buf), C.byref(st)), "perman_reduced_exact")
    v = int(buf.value.decode())
    return (v, st.as_dict()) if return_stats else v


def perman_reduced_quad(mat, compress: bool = True, scale=None, cpu: bool = False, threads: int = 16,
                        device_id: int = 0, gpu_num: int = 1, min_n: int = 30, max_deg: int = 5,
                        return_stats: bool = False):
    """-o / -u with double-double leaves and combine (sup_perman_reduced_quad):
    (hi, lo), perm = hi + lo."""
    a, dt, n = _mat(mat, 4096)
    lib = _lib.load()
    o = _opts(gpu_num, device_id, threads)
    r = _reduce_opts(compress, scale, min_n, max_deg)
    hi, lo, st = C.c_double(0.0), C.c_double(0.0), SupStats()
    _lib.check(lib.sup_perman_reduced_quad(a.ctypes.data, dt, n, C.byref(o), int(bool(cpu)), C.byref(r),
                                           C.byref(hi), C.byref(lo), C.byref(st)), "perman_reduced_quad")
    return ((hi.value, lo.value), st.as_dict()) if return_stats else (hi.value, lo.value)


def read_mtx(path: str, binary: bool = False) -> tuple[np.ndarray, str, int]:
    """MatrixMarket coordinate file -> (matrix, type name, nz lines) (read_matrix.hpp:11-157)."""
    lib = _lib.load()
    p, t, n, nnz = C.c_void_p(), C.c_int(), C.c_int(), C.c_int()
    _lib.check(lib.sup_read_mtx(path.encode(), int(bool(binary)), C.byref(p), C.byref(t), C.byref(n),
                                C.byref(nnz)), f"read_mtx({path})")
    try:
        dtype = _NP[t.value]
        buf = (C.c_char * (n.value * n.value * np.dtype(dtype).itemsize)).from_address(p.value)
        m = np.frombuffer(buf, dtype=dtype).reshape(n.value, n.value).copy()
    finally:
        lib.sup_free(p)
    return m, _TYPE_NAME[t.value], nnz.value


def read_mtx_complex(path: str) -> tuple[np.ndarray, int]:
    """MatrixMarket coordinate file whose field is `complex` -> (complex128
    matrix, nz lines): general, symmetric (same value mirrored) or hermitian
    (conjugate mirrored, real diagonal); n <= 64."""
    lib = _lib.load()
    p, n, nnz = C.c_void_p(), C.c_int(), C.c_int()
    _lib.check(lib.sup_read_mtx_complex(os.fsencode(path), C.byref(p), C.byref(n), C.byref(nnz)),
               f"read_mtx_complex({path})")
    try:
        buf = (C.c_char * (n.value * n.value * 16)).from_address(p.value)
        m = np.frombuffer(buf, dtype=np.complex128).reshape(n.value, n.value).copy()
    finally:
        lib.sup_free(p)
    return m, nnz.value


# main.cu:77-103 / 156-183 (GPU) and 193-243 (CPU) approximation dispatch:
# algo id -> (method, multi-device form)
ALGOS_APPROX = {1: ("rasmussen", False), 2: ("approximation", False), 3: ("rasmussen", True),
                4: ("approximation", True)}


def approx(mat, algo: int = 1, samples: int = 100000, scale_intervals: int = 4, scale_times: int = 5,
           seed: int = 1, gpu_num: int = 1, cpu: bool = False, cpu_worker: bool = False, threads: int = 16,
           device_id: int = 0, return_stats: bool = False):
    """Randomized estimate of the permanent of the 0/1 pattern of `mat` (the
    reference's -a mode): algo 1/3 Rasmussen, 2/4 scaling-guided sampling;
    3/4 are the multi-device forms (gpu_num devices, + a CPU worker with
    cpu_worker).  cpu=True runs on host threads (the CLI's -c -a).  The
    estimate depends only on (mat, algo's method, samples, seed)."""
    if algo not in ALGOS_APPROX:
        raise SupError(-7, "approx", f"unknown approximation id {algo}")
    method, multi = ALGOS_APPROX[algo]
    a, dt, n = _mat(mat, 1024)
    lib = _lib.load()
    o = _opts(gpu_num if multi else 1, device_id, threads)
    o.cpu_worker = int(bool(cpu_worker and multi))
    r = SupApproxResult()
    _lib.check(lib.sup_approx(a.ctypes.data, dt, n, 0 if method == "rasmussen" else 1, int(samples),
                              int(scale_intervals), int(scale_times), int(seed), C.byref(o), int(bool(cpu)),
                              C.byref(r)), "approx")
    return (r.mean, r.as_dict()) if return_stats else r.mean


def grid_graph(m: int, n: int) -> np.ndarray:
    """Bipartite adjacency of the m x n grid graph (util.h:403-520); its
    permanent is the number of domino tilings of the board."""
    lib = _lib.load()
    p, nov = C.POINTER(C.c_int)(), C.c_int()
    _lib.check(lib.sup_grid_graph(int(m), int(n), C.byref(p), C.byref(nov)), "grid_graph")
    try:
        a = np.ctypeslib.as_array(p, shape=(nov.value * nov.value,)).reshape(nov.value, nov.value).copy()
    finally:
        lib.sup_free(C.cast(p, C.c_void_p))
    return a.astype(np.int32)
