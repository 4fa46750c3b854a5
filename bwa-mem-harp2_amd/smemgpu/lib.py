"""ctypes binding of libsmemgpu.so (include/smem_gpu.h).

The library is built in-tree by `make -C bwa-mem-harp2_amd` (or
__graft_entry__.build()).  Loading fails loudly if it is missing: there is no
Python or CPU fallback for the seeding path.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("SMEMGPU_LIB") or os.path.join(PKG_DIR, "lib", "libsmemgpu.so")  # override: A/B builds

SMEM_OK = 0
ERRORS = {-1: "SMEM_E_ARG", -2: "SMEM_E_NOMEM", -3: "SMEM_E_IO", -4: "SMEM_E_DEVICE",
          -5: "SMEM_E_INTERNAL", -6: "SMEM_E_CAPACITY"}

# every symbol include/smem_gpu.h declares
EXPORTED = [
    "smem_opt_default", "smem_bwt_build", "smem_bwt_build_gpu", "smem_bwt_read", "smem_bwt_write", "smem_index_free",
    "smem_gpu_device_count", "smem_gpu_init", "smem_gpu_shutdown", "smem_gpu_collect",
    "smem_batch_create", "smem_batch_destroy", "smem_batch_set_reads", "smem_batch_set_reads_packed",
    "smem_batch_run", "smem_batch_fetch", "smem_batch_read", "smem_batch_results", "smem_batch_stats",
    "smem_gpu_set_lanes_per_cu", "smem_gpu_set_intv_cap", "smem_gpu_set_kernel_variant", "smem_gpu_get_kernel_variant", "smem_gpu_grid_reads", "smem_gpu_set_kmer_table", "smem_batch_debug", "smem_strerror",
    "smem_gpu_kmer_facts", "smem_gpu_seed_kernel", "smem_kmer_depth", "smem_kmer_call_depth",
    "smem_kmer_probe_depth", "smem_gpu_kmer_probe_depth",
    "smem_gpu_set_kmer_table_leaf", "smem_kmer_leaf_probe_depth", "smem_gpu_kmer_leaf_facts",
    "smem_gpu_build_id",
    "smem_bwt_build_sa", "smem_bwt_build_gpu_sa", "smem_sa_read", "smem_sa_write", "smem_sa_free", "smem_gpu_load_sa",
    "smem_batch_sa", "smem_batch_sa_results",
    "smem_chain_opt_default", "smem_batch_chain", "smem_batch_chain_results", "smem_bwt_build_gpu_large",
    "smem_ksw_opt_default", "smem_ksw_extend", "smem_aln_opt_default", "smem_chain2aln",
    "smem_gpu_seed_stream", "smem_batch_results_packed",
    "smem_gpu_load_pac", "smem_batch_chain2aln", "smem_batch_aln_results", "smem_ksw_align2",
    "smem_gpu_init_devices", "smem_gpu_parse_devices", "smem_gpu_collect_ex", "smem_batch_fetch_mask",
    "smem_gpu_reserve_slots", "smem_gpu_set_max_active", "smem_gpu_get_max_active", "smem_gpu_kernel_id", "smem_gpu_fault",
    "smem_batch_memory", "smem_gpu_memory", "smem_gpu_init_devices_async", "smem_gpu_wait_ready",
    "smem_gpu_open_async", "smem_gpu_load_sa_async", "smem_gpu_load_pac_async",
    "smem_reg2aln",
    "smem_fin_opt_default", "smem_reg_finalize", "smem_batch_reg_finalize", "smem_batch_fin_results",
    "smem_gpu_load_contigs", "smem_batch_reg2aln", "smem_batch_aln2_results",
    "smem_gpu_load_contig_names", "smem_batch_set_read_text", "smem_batch_sam", "smem_batch_sam_results",
    "smem_sam_text", "smem_batch_sam_stats", "smem_sam_text_pe",
    "smem_ksw_align2_long", "smem_matesw_opt_default", "smem_matesw", "smem_gpu_cu_count",
    "smem_pestat_opt_default", "smem_pestat", "smem_pair_opt_default", "smem_pair",
    "smem_occ_narrow_ok", "smem_occ64_host", "smem_extend_host",
]

# smem_batch_fetch_mask bits (include/smem_gpu.h)
FETCH_INTV, FETCH_SA, FETCH_CHAINS, FETCH_REGS, FETCH_ALL = 1, 2, 4, 8, 15
FETCH_FIN = 16   # Batch.reg_finalize's results; not part of FETCH_ALL
FETCH_ALN = 32   # Batch.reg2aln's results; not part of FETCH_ALL
FETCH_SAM = 64   # Batch.sam's text; not part of FETCH_ALL
KSWA_MAX_TLEN = 2048   # SMEM_KSWA_MAX_TLEN: the longest target of Gpu.ksw_align2_long
COLLECT_NO_FETCH = 1


def source_hash() -> str:
    """The content hash bwa-mem-harp2_amd/Makefile compiles into the library
    (SRC_HASH): sha256 of csrc/*.{hip,cpp,c,h}, include/*.h and the Makefile
    (its compiler flags), concatenated in path order, first 16 hex digits."""
    import glob
    import hashlib
    inc = os.path.join(os.path.dirname(PKG_DIR), "include")
    files = sorted(glob.glob(os.path.join(PKG_DIR, "csrc", "*.hip")) + glob.glob(os.path.join(PKG_DIR, "csrc", "*.cpp"))
                   + glob.glob(os.path.join(PKG_DIR, "csrc", "*.c")) + glob.glob(os.path.join(PKG_DIR, "csrc", "*.h"))
                   + glob.glob(os.path.join(inc, "*.h")) + [os.path.join(PKG_DIR, "Makefile")])
    h = hashlib.sha256()
    for f in files:
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def build_id() -> str:
    """The source hash the loaded libsmemgpu.so was built from."""
    return load().smem_gpu_build_id().decode()


def kernel_id() -> str:
    """Hash of the loaded library's seeding-kernel sources and compile flags only
    (bwa-mem-harp2_amd/Makefile KERNEL_HASH): seed_kernel counters recorded on
    another build of the runtime still describe it when this id matches."""
    return load().smem_gpu_kernel_id().decode()


class SmemError(RuntimeError):
    pass


class Intv(C.Structure):
    _fields_ = [("x", C.c_uint64 * 3), ("info", C.c_uint64)]


class IndexT(C.Structure):
    _fields_ = [("primary", C.c_uint64), ("L2", C.c_uint64 * 5), ("seq_len", C.c_uint64),
                ("bwt_size", C.c_uint64), ("bwt", C.POINTER(C.c_uint32)), ("owns", C.c_int)]


class SaT(C.Structure):
    _fields_ = [("primary", C.c_uint64), ("L2", C.c_uint64 * 5), ("seq_len", C.c_uint64), ("sa_intv", C.c_uint64),
                ("n_sa", C.c_uint64), ("sa", C.POINTER(C.c_uint64)), ("owns", C.c_int)]


class OptT(C.Structure):
    _fields_ = [("min_seed_len", C.c_int), ("split_factor", C.c_float), ("split_width", C.c_int),
                ("start_width", C.c_int)]


class BatchStats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("compact_ms", C.c_double), ("n_intv", C.c_uint64),
                ("n_calls", C.c_uint64), ("n_overflow", C.c_uint32), ("grid", C.c_int), ("block", C.c_int),
                ("sa_ms", C.c_double), ("n_occ", C.c_uint64), ("chain_ms", C.c_double), ("n_chains", C.c_uint64),
                ("aln_ms", C.c_double), ("n_regs", C.c_uint64), ("t_start", C.c_uint64), ("t_end", C.c_uint64),
                ("fin_ms", C.c_double), ("fin_lane_ms", C.c_double), ("fin_wave_ms", C.c_double),
                ("n_fin", C.c_uint64), ("n_fin_sel", C.c_uint64),
                ("g2a_ms", C.c_double), ("g2a_prep_ms", C.c_double), ("n_g2a", C.c_uint64),
                ("n_g2a_deferred", C.c_uint64), ("n_g2a_xref", C.c_uint64), ("n_g2a_passes", C.c_uint64)]


class SamStats(C.Structure):
    """smem_sam_stats_t"""
    _fields_ = [("sam_ms", C.c_double), ("n_sam_bytes", C.c_uint64), ("n_sam_host", C.c_uint64),
                ("sam_write_ms", C.c_double)]


class StreamStats(C.Structure):
    """smem_stream_stats_t"""
    _fields_ = [("wall_s", C.c_double), ("n_reads", C.c_uint64), ("n_chunks", C.c_uint64), ("n_intv", C.c_uint64),
                ("h2d_bytes", C.c_uint64), ("d2h_bytes", C.c_uint64), ("workers", C.c_int), ("stage_s", C.c_double),
                ("run_s", C.c_double), ("fetch_s", C.c_double)]


# int (*smem_chunk_fn)(void *ctx, int64_t chunk, int64_t first_read, int n_reads, const smem_batch_t *b)
CHUNK_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_void_p)


class KswOptT(C.Structure):
    """smem_ksw_opt_t"""
    _fields_ = [("mat", C.c_int8 * 25), ("pad", C.c_int8 * 3), ("o_del", C.c_int32), ("e_del", C.c_int32),
                ("o_ins", C.c_int32), ("e_ins", C.c_int32)]


class ChainOptT(C.Structure):
    _fields_ = [("w", C.c_int), ("max_chain_gap", C.c_int), ("mask_level", C.c_float),
                ("chain_drop_ratio", C.c_float), ("filter", C.c_int)]


class AlnOptT(C.Structure):
    """smem_aln_opt_t: the mem_opt_t fields mem_chain2aln reads"""
    _fields_ = [("mat", C.c_int8 * 25), ("pad", C.c_int8 * 3), ("o_del", C.c_int32), ("e_del", C.c_int32),
                ("o_ins", C.c_int32), ("e_ins", C.c_int32), ("a", C.c_int32), ("w", C.c_int32), ("zdrop", C.c_int32),
                ("pen_clip5", C.c_int32), ("pen_clip3", C.c_int32), ("min_seed_len", C.c_int32)]


def aln_opt(**kw) -> AlnOptT:
    """smem_aln_opt_default (mem_opt_init's scoring, software/bwamem.c:47-70)
    with the named fields overridden (e.g. min_seed_len=19, w=100)."""
    o = AlnOptT()
    load().smem_aln_opt_default(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


class FinOptT(C.Structure):
    """smem_fin_opt_t: the mem_opt_t fields raw regions -> final regions reads"""
    _fields_ = [("a", C.c_int), ("b", C.c_int), ("o_del", C.c_int), ("e_del", C.c_int), ("o_ins", C.c_int),
                ("e_ins", C.c_int), ("min_seed_len", C.c_int), ("T", C.c_int), ("mask_level", C.c_float),
                ("mask_level_redun", C.c_float), ("mapQ_coef_len", C.c_float), ("mapQ_coef_fac", C.c_int),
                ("flag", C.c_int)]


FIN_F_NO_EXACT, FIN_F_ALL, FIN_F_NO_MULTI = 1, 2, 4
FIN_MAX_REGS, FIN_TAB_LEN, FIN_REJECT = 1024, 4096, 1


def fin_opt(**kw) -> FinOptT:
    """smem_fin_opt_default (mem_opt_init, software/bwamem.c:48-75) with the
    named fields overridden; no_exact / all / no_multi set the flag bits."""
    o = FinOptT()
    load().smem_fin_opt_default(C.byref(o))
    for k, v in kw.items():
        if k in ("no_exact", "all", "no_multi"):
            bit = {"no_exact": FIN_F_NO_EXACT, "all": FIN_F_ALL, "no_multi": FIN_F_NO_MULTI}[k]
            o.flag = (o.flag | bit) if v else (o.flag & ~bit)
        else:
            setattr(o, k, v)
    return o


class PestatT(C.Structure):
    """smem_pestat_t = mem_pestat_t"""
    _fields_ = [("low", C.c_int32), ("high", C.c_int32), ("failed", C.c_int32), ("pad", C.c_int32),
                ("avg", C.c_double), ("std", C.c_double)]


class MateswOptT(C.Structure):
    """smem_matesw_opt_t: the mem_opt_t fields mate rescue reads"""
    _fields_ = [("mat", C.c_int8 * 25), ("pad", C.c_int8 * 3), ("o_del", C.c_int32), ("e_del", C.c_int32),
                ("o_ins", C.c_int32), ("e_ins", C.c_int32), ("a", C.c_int32), ("min_seed_len", C.c_int32),
                ("pen_unpaired", C.c_int32), ("max_matesw", C.c_int32), ("mask_level_redun", C.c_float),
                ("pad2", C.c_int32)]


MSW_HOST = 1   # SMEM_MSW_HOST: the pair is the caller's


def matesw_opt(**kw) -> MateswOptT:
    """smem_matesw_opt_default (mem_opt_init, software/bwamem.c:48-75) with the named fields
    overridden; mat takes the 25 entries of a scoring matrix (synth.bwa_scmat)."""
    o = MateswOptT()
    load().smem_matesw_opt_default(C.byref(o))
    for k, v in kw.items():
        if k == "mat":
            for i, x in enumerate(np.asarray(v, dtype=np.int8).reshape(-1)[:25]):
                o.mat[i] = int(x)
        else:
            setattr(o, k, v)
    return o


class PestatOptT(C.Structure):
    """smem_pestat_opt_t: the mem_opt_t fields mem_pestat reads"""
    _fields_ = [("a", C.c_int32), ("min_seed_len", C.c_int32), ("max_ins", C.c_int32), ("mask_level", C.c_float),
                ("pad", C.c_int32 * 2)]


class PairOptT(C.Structure):
    """smem_pair_opt_t: the mem_opt_t fields mem_pair and the decision block of mem_sam_pe read"""
    _fields_ = [("a", C.c_int32), ("b", C.c_int32), ("o_del", C.c_int32), ("e_del", C.c_int32), ("o_ins", C.c_int32),
                ("e_ins", C.c_int32), ("pen_unpaired", C.c_int32), ("T", C.c_int32), ("min_seed_len", C.c_int32),
                ("mapQ_coef_len", C.c_float), ("mapQ_coef_fac", C.c_int32), ("flags", C.c_int32)]


PESTAT_MAX_INS = 65535   # SMEM_PESTAT_MAX_INS
PESTAT_WAVES_PER_CU = 8  # the statistics kernel's grid: this many waves of 64 pairs a CU (csrc/pair_kernels.h)
PAIR_TAB_LEN = 65536     # SMEM_PAIR_TAB_LEN
PAIR_LANE_MAX = 16       # pairs of up to this many regions in both lists are done a pair per lane
PAIR_WAVES_PER_CU = 4    # the long pairs' grid (csrc/pair_kernels.h)
PAIR_F_NOPAIRING = 1     # SMEM_PAIR_F_NOPAIRING
PAIR_HOST = 1            # SMEM_PAIR_HOST: the pair is the caller's
# smem_pestat_t and smem_pair_sel_t
PESTAT_DT = np.dtype([("low", "<i4"), ("high", "<i4"), ("failed", "<i4"), ("pad", "<i4"), ("avg", "<f8"), ("std", "<f8")])
PAIR_SEL_DT = np.dtype([("status", "<i4"), ("branch", "<i4"), ("z", "<i4", (2,)), ("mapq", "<i4", (2,)),
                        ("proper", "<i4"), ("o", "<i4"), ("subo", "<i4"), ("n_sub", "<i4"), ("sub", "<i4", (2,)),
                        ("promoted", "<i4", (2,))])


def pestat_opt(**kw) -> PestatOptT:
    """smem_pestat_opt_default (mem_opt_init, software/bwamem.c:48-75) with the named fields overridden"""
    o = PestatOptT()
    load().smem_pestat_opt_default(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def pair_opt(**kw) -> PairOptT:
    """smem_pair_opt_default with the named fields overridden; nopairing sets the flag bit"""
    o = PairOptT()
    load().smem_pair_opt_default(C.byref(o))
    for k, v in kw.items():
        if k == "nopairing":
            o.flags = (o.flags | PAIR_F_NOPAIRING) if v else (o.flags & ~PAIR_F_NOPAIRING)
        else:
            setattr(o, k, v)
    return o


SEED_DT = np.dtype([("rbeg", "<i8"), ("qbeg", "<i4"), ("len", "<i4")])          # smem_seed_t = mem_seed_t
CHAIN_DT = np.dtype([("pos", "<i8"), ("seed_off", "<u8"), ("n", "<i4"), ("pad", "<i4")])  # smem_chain_t
# smem_alnreg_t = mem_alnreg_t (the 64-byte records chain2aln returns)
ALNREG_DT = np.dtype([("rb", "<i8"), ("re", "<i8"), ("qb", "<i4"), ("qe", "<i4"), ("score", "<i4"), ("truesc", "<i4"),
                      ("sub", "<i4"), ("csub", "<i4"), ("sub_n", "<i4"), ("w", "<i4"), ("seedcov", "<i4"),
                      ("secondary", "<i4"), ("hash", "<u8")])
# smem_aln_t
ALN_DT = np.dtype([("pos", "<i8"), ("is_rev", "<i4"), ("n_cigar", "<i4"), ("NM", "<i4"), ("score", "<i4"),
                   ("tries", "<i4"), ("status", "<i4"), ("cigar_off", "<u8"), ("md_off", "<u8"), ("md_len", "<i4"),
                   ("pad", "<i4")])
ALN_UNMAPPED, ALN_NOCIGAR, ALN_REJECT, ALN_XREF = 1, 2, 3, 4
FIN_SEL_DT = np.dtype([("mapq", "<i4"), ("flag", "<i4"), ("xs", "<i4")])   # smem_fin_sel_t
SAM_REC_DT = np.dtype([("mapq", "<i4"), ("flag", "<i4"), ("score", "<i4"), ("xs", "<i4")])   # smem_sam_rec_t
SAM_HOST = 1     # SMEM_SAM_HOST: the read's lines are the caller's


class SamOptT(C.Structure):
    """smem_sam_opt_t"""
    _fields_ = [("rg_id", C.c_char_p)]


def pack_strings(strs) -> tuple:
    """[str or bytes] -> (uint8 bytes, uint64 offsets[n + 1]): the layout names and comments travel in"""
    b = [x if isinstance(x, (bytes, bytearray)) else str(x).encode("latin-1") for x in strs]
    off = np.zeros(len(b) + 1, dtype=np.uint64)
    if b:
        off[1:] = np.cumsum([len(x) for x in b])
    return np.frombuffer(b"".join(b), dtype=np.uint8).copy(), off
SMEM_E_CAPACITY = -6


_lib = None


def load() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SmemError(f"{LIB_PATH} is missing: build it with `make -C {PKG_DIR}` (no fallback exists)")
    lib = C.CDLL(LIB_PATH)
    P = C.POINTER
    lib.smem_opt_default.argtypes = [P(OptT)]
    lib.smem_opt_default.restype = None
    lib.smem_bwt_build.argtypes = [C.c_void_p, C.c_uint64, P(IndexT)]
    lib.smem_bwt_build_gpu.argtypes = [C.c_int, C.c_void_p, C.c_uint64, P(IndexT)]
    lib.smem_bwt_read.argtypes = [C.c_char_p, P(IndexT)]
    lib.smem_bwt_write.argtypes = [C.c_char_p, P(IndexT)]
    lib.smem_index_free.argtypes = [P(IndexT)]
    lib.smem_index_free.restype = None
    lib.smem_bwt_build_sa.argtypes = [C.c_void_p, C.c_uint64, C.c_int, P(IndexT), P(SaT)]
    lib.smem_bwt_build_gpu_sa.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_int, P(IndexT), P(SaT)]
    lib.smem_bwt_build_gpu_large.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_int, P(IndexT), P(SaT)]
    lib.smem_sa_read.argtypes = [C.c_char_p, P(SaT)]
    lib.smem_sa_write.argtypes = [C.c_char_p, P(SaT)]
    lib.smem_sa_free.argtypes = [P(SaT)]
    lib.smem_sa_free.restype = None
    lib.smem_gpu_load_sa.argtypes = [C.c_void_p, P(SaT)]
    lib.smem_batch_sa.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.smem_batch_sa_results.argtypes = [C.c_void_p, P(P(C.c_uint64)), P(P(C.c_uint64)), P(C.c_uint64)]
    lib.smem_ksw_opt_default.argtypes = [P(KswOptT)]
    lib.smem_ksw_opt_default.restype = None
    lib.smem_ksw_extend.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                    P(KswOptT), C.c_void_p, P(C.c_double)]
    lib.smem_aln_opt_default.argtypes = [C.c_void_p]
    lib.smem_aln_opt_default.restype = None
    lib.smem_chain2aln.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_uint64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                   P(C.c_double)]
    lib.smem_reg2aln.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, P(C.c_uint64),
                                 C.c_void_p, C.c_uint64, P(C.c_uint64), P(C.c_double)]
    lib.smem_fin_opt_default.argtypes = [P(FinOptT)]
    lib.smem_fin_opt_default.restype = None
    lib.smem_reg_finalize.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                      P(FinOptT), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, P(C.c_double)]
    lib.smem_batch_reg_finalize.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, P(FinOptT)]
    lib.smem_batch_fin_results.argtypes = [C.c_void_p, P(C.c_void_p), P(P(C.c_uint64)), P(C.c_void_p),
                                           P(P(C.c_uint64)), P(P(C.c_uint64)), P(P(C.c_int32)), P(C.c_uint64),
                                           P(C.c_uint64)]
    lib.smem_gpu_load_contigs.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64]
    lib.smem_batch_reg2aln.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.smem_batch_aln2_results.argtypes = [C.c_void_p, P(C.c_void_p), P(P(C.c_int32)), P(P(C.c_uint64)),
                                            P(P(C.c_uint32)), P(C.c_uint64), P(C.c_void_p), P(C.c_uint64),
                                            P(C.c_uint64)]
    if hasattr(lib, "smem_sam_text"):  # absent from A/B libraries built before the SAM text stage
        lib.smem_gpu_load_contig_names.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        lib.smem_batch_set_read_text.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.smem_batch_sam.argtypes = [C.c_void_p, P(SamOptT)]
        lib.smem_batch_sam_stats.argtypes = [C.c_void_p, P(SamStats)]
        lib.smem_batch_sam_results.argtypes = [C.c_void_p, P(C.c_void_p), P(P(C.c_uint64)), P(P(C.c_int32)),
                                               P(C.c_uint64)]
        lib.smem_sam_text.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 13 + [C.c_uint64, C.c_void_p, C.c_uint64,
                                                                                 C.c_int, C.c_void_p, C.c_void_p,
                                                                                 C.c_void_p, P(SamOptT), C.c_void_p,
                                                                                 C.c_uint64, C.c_void_p, C.c_void_p,
                                                                                 P(C.c_uint64), P(C.c_double)]
    if hasattr(lib, "smem_sam_text_pe"):
        lib.smem_sam_text_pe.argtypes = [C.c_void_p, C.c_int, C.c_void_p] + lib.smem_sam_text.argtypes[1:]
    lib.smem_chain_opt_default.argtypes = [P(ChainOptT)]
    lib.smem_chain_opt_default.restype = None
    lib.smem_batch_chain.argtypes = [C.c_void_p, C.c_int64, P(ChainOptT)]
    lib.smem_batch_chain_results.argtypes = [C.c_void_p, P(C.c_void_p), P(P(C.c_uint64)), P(C.c_void_p),
                                             P(C.c_uint64), P(C.c_uint64)]
    lib.smem_gpu_device_count.argtypes = []
    lib.smem_gpu_init.argtypes = [P(C.c_void_p), C.c_int, C.c_void_p, C.c_uint64, C.c_uint64, P(C.c_uint64)]
    lib.smem_gpu_shutdown.argtypes = [C.c_void_p]
    lib.smem_gpu_shutdown.restype = None
    lib.smem_gpu_collect.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, P(OptT), P(C.c_void_p)]
    lib.smem_gpu_collect_ex.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, P(OptT), C.c_int,
                                        P(C.c_void_p)]
    lib.smem_gpu_init_devices.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64,
                                          P(C.c_uint64), C.c_void_p, C.c_void_p, C.c_int64]
    lib.smem_gpu_parse_devices.argtypes = [C.c_char_p, C.c_void_p, C.c_int]
    lib.smem_batch_fetch_mask.argtypes = [C.c_void_p, C.c_int]
    lib.smem_gpu_seed_stream.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, P(OptT), C.c_int, C.c_int,
                                         C.c_int, C.c_void_p, C.c_void_p, P(StreamStats)]
    lib.smem_ksw_align2.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                    P(KswOptT), C.c_void_p, P(C.c_double)]
    lib.smem_ksw_align2_long.argtypes = lib.smem_ksw_align2.argtypes
    lib.smem_matesw_opt_default.argtypes = [P(MateswOptT)]
    lib.smem_matesw_opt_default.restype = None
    lib.smem_matesw.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_int64, P(MateswOptT), C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                C.c_void_p, P(C.c_uint64), P(C.c_double)]
    lib.smem_pestat_opt_default.argtypes = [P(PestatOptT)]
    lib.smem_pestat_opt_default.restype = None
    lib.smem_pestat.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, P(PestatOptT), C.c_void_p,
                                C.c_void_p, P(C.c_double)]
    lib.smem_pair_opt_default.argtypes = [P(PairOptT)]
    lib.smem_pair_opt_default.restype = None
    lib.smem_pair.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p,
                              P(PairOptT), C.c_void_p, P(C.c_double)]
    lib.smem_gpu_load_pac.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    lib.smem_batch_chain2aln.argtypes = [C.c_void_p, C.c_void_p]
    lib.smem_batch_aln_results.argtypes = [C.c_void_p, P(C.c_void_p), P(P(C.c_uint64)), P(C.c_uint64)]
    lib.smem_batch_results_packed.argtypes = [C.c_void_p, P(C.c_void_p), P(P(C.c_uint64)), P(P(C.c_uint32)),
                                              P(P(C.c_uint64))]
    lib.smem_batch_create.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.c_int, P(C.c_void_p)]
    lib.smem_batch_destroy.argtypes = [C.c_void_p]
    lib.smem_batch_destroy.restype = None
    lib.smem_batch_set_reads.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.smem_batch_set_reads_packed.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.smem_batch_run.argtypes = [C.c_void_p, P(OptT)]
    lib.smem_batch_fetch.argtypes = [C.c_void_p]
    lib.smem_batch_read.argtypes = [C.c_void_p, C.c_int, P(P(Intv)), P(C.c_int), P(P(C.c_uint32)), P(C.c_int)]
    lib.smem_batch_results.argtypes = [C.c_void_p, P(P(Intv)), P(P(C.c_uint64)), P(P(C.c_uint32)), P(P(C.c_uint64))]
    lib.smem_batch_stats.argtypes = [C.c_void_p, P(BatchStats)]
    lib.smem_gpu_set_lanes_per_cu.argtypes = [C.c_void_p, C.c_int]
    lib.smem_gpu_set_intv_cap.argtypes = [C.c_void_p, C.c_int]
    lib.smem_gpu_set_kernel_variant.argtypes = [C.c_void_p, C.c_int]
    lib.smem_gpu_get_kernel_variant.argtypes = [C.c_void_p]
    lib.smem_gpu_get_kernel_variant.restype = C.c_int
    lib.smem_gpu_grid_reads.argtypes = [C.c_void_p]
    lib.smem_gpu_grid_reads.restype = C.c_int
    if hasattr(lib, "smem_gpu_cu_count"):  # absent from A/B libraries built before it
        lib.smem_gpu_cu_count.argtypes = [C.c_void_p]
        lib.smem_gpu_cu_count.restype = C.c_int
    lib.smem_gpu_set_kmer_table.argtypes = [C.c_void_p, C.c_int]
    if hasattr(lib, "smem_gpu_kmer_facts"):  # absent from A/B libraries built before the virtual entries
        lib.smem_gpu_kmer_facts.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_int]
        lib.smem_gpu_kmer_facts.restype = C.c_int
        lib.smem_gpu_seed_kernel.argtypes = [C.c_void_p]
        lib.smem_gpu_seed_kernel.restype = C.c_int
        lib.smem_kmer_depth.argtypes = [C.c_void_p, C.c_int]
        lib.smem_kmer_depth.restype = C.c_int
        lib.smem_kmer_call_depth.argtypes = [C.c_void_p, C.c_int, C.c_int64]
        lib.smem_kmer_call_depth.restype = C.c_int
    if hasattr(lib, "smem_kmer_probe_depth"):  # absent from A/B libraries built before the unstored level's minimum
        lib.smem_kmer_probe_depth.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.c_int64]
        lib.smem_kmer_probe_depth.restype = C.c_int
        lib.smem_gpu_kmer_probe_depth.argtypes = [C.c_void_p, C.c_int64, C.POINTER(C.c_uint64)]
        lib.smem_gpu_kmer_probe_depth.restype = C.c_int
    if hasattr(lib, "smem_kmer_leaf_probe_depth"):  # absent from A/B libraries built before the leaf level
        lib.smem_gpu_set_kmer_table_leaf.argtypes = [C.c_void_p, C.c_int]
        lib.smem_gpu_set_kmer_table_leaf.restype = C.c_int
        lib.smem_kmer_leaf_probe_depth.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.c_int, C.c_int, C.c_uint64, C.c_int64]
        lib.smem_kmer_leaf_probe_depth.restype = C.c_int
        lib.smem_gpu_kmer_leaf_facts.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_uint64), C.POINTER(C.c_int),
                                                 C.POINTER(C.c_uint64)]
        lib.smem_gpu_kmer_leaf_facts.restype = C.c_int
    if hasattr(lib, "smem_occ_narrow_ok"):  # absent from A/B libraries built before the bit-plane layout
        lib.smem_occ_narrow_ok.argtypes = [C.c_void_p]
        lib.smem_occ_narrow_ok.restype = C.c_int
        lib.smem_occ64_host.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
        lib.smem_occ64_host.restype = C.c_int
        lib.smem_extend_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64,
                                         C.c_int, C.c_uint64, C.c_void_p, C.c_int, C.c_void_p]
        lib.smem_extend_host.restype = C.c_int
    if hasattr(lib, "smem_batch_debug"):  # absent from older A/B builds
        lib.smem_batch_debug.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    lib.smem_strerror.argtypes = [C.c_int]
    lib.smem_strerror.restype = C.c_char_p
    lib.smem_gpu_build_id.argtypes = []
    lib.smem_gpu_build_id.restype = C.c_char_p
    lib.smem_gpu_kernel_id.argtypes = []
    lib.smem_gpu_kernel_id.restype = C.c_char_p
    lib.smem_gpu_reserve_slots.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    lib.smem_gpu_set_max_active.argtypes = [C.c_void_p, C.c_int]
    lib.smem_gpu_get_max_active.argtypes = [C.c_void_p]
    lib.smem_gpu_fault.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    lib.smem_gpu_init_devices_async.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64,
                                                P(C.c_uint64), C.c_void_p, C.c_void_p, C.c_int64]
    lib.smem_gpu_wait_ready.argtypes = [C.c_void_p]
    lib.smem_batch_memory.argtypes = [C.c_void_p, P(C.c_uint64), P(C.c_uint64)]
    lib.smem_gpu_memory.argtypes = [C.c_void_p, P(C.c_uint64), P(C.c_uint64), P(C.c_uint64), P(C.c_int)]
    _lib = lib
    return lib


def _check(rc: int, what: str) -> None:
    if rc != SMEM_OK:
        msg = load().smem_strerror(rc).decode(errors="replace")
        raise SmemError(f"{what} failed: {ERRORS.get(rc, rc)}: {msg}")


@dataclass
class Options:
    """mem_opt_t fields of the seeding loop (defaults: software/bwamem.c:58-65)."""
    min_seed_len: int = 19
    split_factor: float = 1.5
    split_width: int = 10
    start_width: int = 1

    def c(self) -> OptT:
        return OptT(self.min_seed_len, self.split_factor, self.split_width, self.start_width)


class Index:
    """BWA .bwt FM-index in host memory (owned by the library)."""

    def __init__(self, raw: IndexT):
        self._raw = raw

    @classmethod
    def build(cls, fwd_codes: np.ndarray) -> "Index":
        fwd = np.ascontiguousarray(fwd_codes, dtype=np.uint8)
        raw = IndexT()
        _check(load().smem_bwt_build(fwd.ctypes.data, fwd.size, C.byref(raw)), "smem_bwt_build")
        return cls(raw)

    @classmethod
    def build_gpu(cls, fwd_codes: np.ndarray, device: int = 0, large: bool = False) -> "Index":
        """Same bytes as build(), constructed on a HIP device (prefix doubling;
        large=True forces the bucketed 64-bit builder used past 2^32 symbols)."""
        fwd = np.ascontiguousarray(fwd_codes, dtype=np.uint8)
        raw = IndexT()
        if large:
            _check(load().smem_bwt_build_gpu_large(device, fwd.ctypes.data, fwd.size, 0, C.byref(raw), None),
                   "smem_bwt_build_gpu_large")
        else:
            _check(load().smem_bwt_build_gpu(device, fwd.ctypes.data, fwd.size, C.byref(raw)), "smem_bwt_build_gpu")
        return cls(raw)

    @classmethod
    def build_sa(cls, fwd_codes: np.ndarray, sa_intv: int = 32, gpu: bool = False, device: int = 0,
                 large: bool = False):
        """(Index, SA): the .bwt and the sampled SA bwa index writes beside it."""
        fwd = np.ascontiguousarray(fwd_codes, dtype=np.uint8)
        raw, sraw = IndexT(), SaT()
        if gpu and large:
            _check(load().smem_bwt_build_gpu_large(device, fwd.ctypes.data, fwd.size, sa_intv, C.byref(raw),
                                                   C.byref(sraw)), "smem_bwt_build_gpu_large")
        elif gpu:
            _check(load().smem_bwt_build_gpu_sa(device, fwd.ctypes.data, fwd.size, sa_intv, C.byref(raw), C.byref(sraw)),
                   "smem_bwt_build_gpu_sa")
        else:
            _check(load().smem_bwt_build_sa(fwd.ctypes.data, fwd.size, sa_intv, C.byref(raw), C.byref(sraw)),
                   "smem_bwt_build_sa")
        return cls(raw), SA(sraw)

    @classmethod
    def read(cls, path: str) -> "Index":
        raw = IndexT()
        _check(load().smem_bwt_read(path.encode(), C.byref(raw)), f"smem_bwt_read({path})")
        return cls(raw)

    def write(self, path: str) -> None:
        _check(load().smem_bwt_write(path.encode(), C.byref(self._raw)), f"smem_bwt_write({path})")

    @property
    def primary(self) -> int:
        return int(self._raw.primary)

    @property
    def L2(self) -> np.ndarray:
        return np.array(list(self._raw.L2), dtype=np.uint64)

    @property
    def seq_len(self) -> int:
        return int(self._raw.seq_len)

    @property
    def words(self) -> np.ndarray:
        """uint32 view (no copy) of the interleaved BWT + Occ words."""
        n = int(self._raw.bwt_size)
        return np.ctypeslib.as_array(self._raw.bwt, shape=(n,))

    def close(self) -> None:
        if self._raw.bwt:
            load().smem_index_free(C.byref(self._raw))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SA:
    """Sampled suffix array (.sa) in host memory (owned by the library)."""

    def __init__(self, raw: SaT):
        self._raw = raw

    @classmethod
    def read(cls, path: str) -> "SA":
        raw = SaT()
        _check(load().smem_sa_read(path.encode(), C.byref(raw)), f"smem_sa_read({path})")
        return cls(raw)

    def write(self, path: str) -> None:
        _check(load().smem_sa_write(path.encode(), C.byref(self._raw)), f"smem_sa_write({path})")

    @property
    def sa_intv(self) -> int:
        return int(self._raw.sa_intv)

    @property
    def seq_len(self) -> int:
        return int(self._raw.seq_len)

    @property
    def samples(self) -> np.ndarray:
        """uint64 view (no copy) of sa[0 .. n_sa-1]; sa[0] = 2^64-1."""
        return np.ctypeslib.as_array(self._raw.sa, shape=(int(self._raw.n_sa),))

    def close(self) -> None:
        if self._raw.sa:
            load().smem_sa_free(C.byref(self._raw))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def device_count() -> int:
    return int(load().smem_gpu_device_count())


@dataclass
class FinResults:
    """raw regions -> final regions (smem_reg_finalize / smem_batch_reg_finalize)"""
    regs: np.ndarray      # ALNREG_DT: every read's final list, in mem_mark_primary_se's order
    out_off: np.ndarray   # (n_reads + 1,) uint64 into regs / sel
    sel: np.ndarray       # FIN_SEL_DT, one per final region; flag -1: no record
    sel_idx: np.ndarray   # uint64: the regions with a record, per read in print order, as indices into regs
    sel_off: np.ndarray   # (n_reads + 1,) uint64 into sel_idx
    status: np.ndarray    # (n_reads,) int32: 0 or FIN_REJECT
    kernel_ms: float = 0.0


@dataclass
class AlnResults:
    """final regions -> alignments (smem_batch_reg2aln)"""
    alns: np.ndarray      # ALN_DT, one per record; status ALN_XREF: bwa_fix_xref2 is needed, the caller's
    rid: np.ndarray       # int32, one per record: the contig of pos (-1: no alignment, or no contig table)
    aln_off: np.ndarray   # (n_reads + 1,) uint64 into alns / rid: sel_off, or the caller's idx_off
    cigar: np.ndarray     # uint32 words; record k's are cigar[cigar_off : cigar_off + n_cigar]
    md: np.ndarray        # uint8; record k's MD is md[md_off : md_off + md_len]


@dataclass
class SamResults:
    """alignments -> SAM text (smem_batch_sam / smem_sam_text)"""
    text: np.ndarray      # uint8: read r's lines are text[text_off[r] : text_off[r + 1]], reads in batch order
    text_off: np.ndarray  # (n_reads + 1,) uint64
    status: np.ndarray    # (n_reads,) int32: 0, or SAM_HOST (no bytes: the caller prints the read)
    kernel_ms: float = 0.0

    def read(self, r: int) -> bytes:
        return self.text[int(self.text_off[r]):int(self.text_off[r + 1])].tobytes()


@dataclass
class Results:
    intv: np.ndarray      # (N, 4) uint64: x0, x1, x2, info
    intv_off: np.ndarray  # (n_reads + 1,) uint64
    call_n: np.ndarray    # (n_lists,) uint32
    call_off: np.ndarray  # (n_reads + 1,) uint64
    occ_off: np.ndarray | None = None  # (N + 1,) uint64, when Batch.sa() ran
    sa_pos: np.ndarray | None = None   # (n_occ,) uint64 bwt_sa positions
    chains: np.ndarray | None = None   # CHAIN_DT, when Batch.chain() ran
    chain_off: np.ndarray | None = None  # (n_reads + 1,) uint64
    seeds: np.ndarray | None = None    # SEED_DT, each chain's seeds contiguous
    regs: np.ndarray | None = None     # raw 64-byte smem_alnreg_t records, when Batch.chain2aln() ran
    reg_off: np.ndarray | None = None  # (n_reads + 1,) uint64
    fin: "FinResults | None" = None    # when Batch.reg_finalize() ran and FETCH_FIN was asked for
    aln: "AlnResults | None" = None    # when Batch.reg2aln() ran and FETCH_ALN was asked for
    sam: "SamResults | None" = None    # when Batch.sam() ran and FETCH_SAM was asked for

    def read_chains(self, i: int) -> list:
        """read i's chains as [(pos, seeds)], in mem_chain(+flt) order."""
        out = []
        for c in self.chains[int(self.chain_off[i]):int(self.chain_off[i + 1])]:
            o = int(c["seed_off"])
            out.append((int(c["pos"]), self.seeds[o:o + int(c["n"])]))
        return out

    def to_smch(self) -> bytes:
        from . import synth
        return synth.write_smch([self.read_chains(i) for i in range(self.chain_off.size - 1)])

    def read_sa(self, i: int) -> np.ndarray:
        """bwt_sa positions of read i's seed occurrences, in interval order."""
        a, b = int(self.intv_off[i]), int(self.intv_off[i + 1])
        return self.sa_pos[int(self.occ_off[a]):int(self.occ_off[b])]

    def to_smsa(self) -> bytes:
        from . import synth
        return synth.write_smsa([self.read_sa(i) for i in range(self.intv_off.size - 1)])

    def read_calls(self, i: int) -> list:
        """The lists smem_next2 returned for read i, in order."""
        iv = self.intv[self.intv_off[i]:self.intv_off[i + 1]]
        ns = self.call_n[self.call_off[i]:self.call_off[i + 1]]
        out, p = [], 0
        for n in ns:
            out.append(iv[p:p + int(n)])
            p += int(n)
        return out

    def to_smgo(self) -> bytes:
        import struct
        n = self.intv_off.size - 1
        parts = [b"SMGO0001", struct.pack("<Q", n)]
        for i in range(n):
            calls = self.read_calls(i)
            parts.append(struct.pack("<I", len(calls)))
            for arr in calls:
                parts.append(struct.pack("<I", arr.shape[0]))
                parts.append(np.ascontiguousarray(arr, dtype="<u8").tobytes())
        return b"".join(parts)


class Gpu:
    """One HIP device with the index resident in HBM (smem_gpu_init)."""

    def __init__(self, index: Index, device: int = 0, lanes_per_cu: int = 0, intv_cap: int = 0, variant: int = 0,
                 kmer_k: int = 0):
        lib = load()
        self._h = C.c_void_p()
        words = index.words
        L2 = (C.c_uint64 * 5)(*[int(v) for v in index.L2])
        _check(lib.smem_gpu_init(C.byref(self._h), device, words.ctypes.data, words.size, index.primary, L2),
               "smem_gpu_init")
        if lanes_per_cu:
            _check(lib.smem_gpu_set_lanes_per_cu(self._h, lanes_per_cu), "smem_gpu_set_lanes_per_cu")
        if intv_cap:
            _check(lib.smem_gpu_set_intv_cap(self._h, intv_cap), "smem_gpu_set_intv_cap")
        if kmer_k:
            self.set_kmer_table(kmer_k)
        if variant:
            _check(lib.smem_gpu_set_kernel_variant(self._h, variant), "smem_gpu_set_kernel_variant")
        self.device = device

    @classmethod
    def open_async(cls, index: Index, devices, sa: "SA" = None, pac=None, l_pac: int = 0) -> list:
        """smem_gpu_init_devices_async: one Gpu per entry of `devices`, whose
        uploads run in the background (index, sa and pac must outlive them:
        keep the objects alive until wait_ready() or close())."""
        lib = load()
        n = len(devices)
        hs = (C.c_void_p * n)()
        devs = (C.c_int * n)(*devices)
        words = index.words
        L2 = (C.c_uint64 * 5)(*[int(v) for v in index.L2])
        pac_p = np.ascontiguousarray(pac, dtype=np.uint8).ctypes.data if pac is not None else None
        _check(lib.smem_gpu_init_devices_async(hs, n, devs, words.ctypes.data, words.size, index.primary, L2,
                                               C.byref(sa._raw) if sa is not None else None, pac_p, int(l_pac)),
               "smem_gpu_init_devices_async")
        out = []
        for i in range(n):
            g = cls.__new__(cls)
            g._h = C.c_void_p(hs[i])
            g.device = devices[i]
            out.append(g)
        return out

    def wait_ready(self) -> None:
        _check(load().smem_gpu_wait_ready(self._h), "smem_gpu_wait_ready")

    def set_variant(self, variant: int) -> None:
        """Seeding-kernel variant (0 = default; see smem_gpu_set_kernel_variant)."""
        _check(load().smem_gpu_set_kernel_variant(self._h, variant), "smem_gpu_set_kernel_variant")

    @property
    def grid_reads(self) -> int:
        """Reads one seeding launch holds in flight (smem_gpu_grid_reads)."""
        return int(load().smem_gpu_grid_reads(self._h))

    def cu_count(self) -> int:
        """The device's compute units (smem_gpu_cu_count)."""
        lib = load()
        if not hasattr(lib, "smem_gpu_cu_count"):
            raise SmemError("smem_gpu_cu_count: this library was built before it")
        n = int(lib.smem_gpu_cu_count(self._h))
        if n < 1:
            raise SmemError(f"smem_gpu_cu_count failed: {n}")
        return n

    @property
    def variant(self) -> int:
        """The seeding-kernel variant this handle runs (smem_gpu_get_kernel_variant)."""
        return int(load().smem_gpu_get_kernel_variant(self._h))

    def set_kmer_table(self, k: int) -> None:
        """Build (k = 1..15) or free (0) the device k-mer bi-interval table."""
        _check(load().smem_gpu_set_kmer_table(self._h, k), "smem_gpu_set_kmer_table")

    def set_kmer_table_leaf(self, k: int) -> None:
        """Build the table of k levels (1..13) with level k + 1 stored behind them as its leaf
        (smem_gpu_set_kmer_table_leaf; SMEM_GPU_KMER_LEAF=0 in the environment: without the leaf)."""
        _check(load().smem_gpu_set_kmer_table_leaf(self._h, k), "smem_gpu_set_kmer_table_leaf")

    def kmer_leaf_facts(self) -> dict:
        """The table's leaf (smem_gpu_kmer_leaf_facts): its level k + 1 (0: none), its smallest size, whether
        it is strict (no present string of it has a one-base extension of its own size), and the smallest
        size of level k + 2, which the build reduced from it."""
        lv, st = C.c_int(0), C.c_int(0)
        mn, nx = C.c_uint64(0), C.c_uint64(0)
        _check(load().smem_gpu_kmer_leaf_facts(self._h, C.byref(lv), C.byref(mn), C.byref(st), C.byref(nx)),
               "smem_gpu_kmer_leaf_facts")
        return {"level": lv.value, "min": int(mn.value), "strict": bool(st.value), "next_min": int(nx.value)}

    def kmer_facts(self) -> dict:
        """The k-mer table's facts (smem_gpu_kmer_facts): k its depth (0: none), D the largest level
        below k such that every string of D + 1 bases occurs, minsz[L] the smallest interval size of
        level L (the stored levels only: see kmer_probe_depth for the depth a launch runs at)."""
        k, d = C.c_int(0), C.c_int(0)
        mn = np.zeros(16, dtype=np.uint64)
        _check(load().smem_gpu_kmer_facts(self._h, C.byref(k), C.byref(d), mn.ctypes.data, 16), "smem_gpu_kmer_facts")
        return {"k": k.value, "D": d.value, "minsz": [int(v) for v in mn[:k.value + 1]]}

    def kmer_probe_depth(self, min_intv: int = 1) -> dict:
        """The depth a launch probes the table at for calls with this min_intv, and the smallest size of
        the unstored level k + 1 (smem_gpu_kmer_probe_depth).  kmer_facts()["D"] counts the stored levels
        only (D <= k - 1); the kernel may also rely on level k + 1, which the build reduced without
        storing it, so the depth here is k where kmer_facts would say k - 1, and k + 1 where the table has
        a leaf that vouches for itself (kmer_leaf_facts; min_next is then the leaf's minimum).  A run takes it for
        min_intv = start_width (a read's first calls) and split_width + 1 (its re-seeding calls)."""
        nx = C.c_uint64(0)
        dp = load().smem_gpu_kmer_probe_depth(self._h, int(min_intv), C.byref(nx))
        if dp < 0:
            _check(dp, "smem_gpu_kmer_probe_depth")
        return {"depth": dp, "min_next": int(nx.value)}

    @property
    def seed_kernel(self) -> int:
        """The seeding-kernel instantiation the next launch runs (smem_gpu_seed_kernel)."""
        return int(load().smem_gpu_seed_kernel(self._h))

    def load_sa(self, sa: "SA") -> None:
        _check(load().smem_gpu_load_sa(self._h, C.byref(sa._raw)), "smem_gpu_load_sa")

    def set_max_active(self, n: int) -> None:
        """Admission: at most n calls on the device at once (smem_gpu_set_max_active; 0 = default)."""
        _check(load().smem_gpu_set_max_active(self._h, n), "smem_gpu_set_max_active")

    def max_active(self) -> int:
        """The admission limit in force (smem_gpu_get_max_active)."""
        rc = load().smem_gpu_get_max_active(self._h)
        if rc < 0:
            _check(rc, "smem_gpu_get_max_active")
        return rc

    def memory(self) -> dict:
        """smem_gpu_memory: bytes of the resident index, of the kept batches (device / pinned)."""
        ix, d, h, nb = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_int()
        _check(load().smem_gpu_memory(self._h, C.byref(ix), C.byref(d), C.byref(h), C.byref(nb)), "smem_gpu_memory")
        return {"index_bytes": ix.value, "batch_device_bytes": d.value, "batch_pinned_bytes": h.value,
                "batches": nb.value}

    def fault(self) -> tuple:
        """(0 | 1 runtime fault | 2 injected sticky fault, message) -- smem_gpu_fault"""
        buf = C.create_string_buffer(512)
        f = load().smem_gpu_fault(self._h, buf, 512)
        return f, buf.value.decode(errors="replace")

    def reserve_slots(self, n_slots: int, reads_per_slot: int, max_len: int) -> None:
        """Pre-size collect_ex worker slots in the background (smem_gpu_reserve_slots)."""
        _check(load().smem_gpu_reserve_slots(self._h, n_slots, reads_per_slot, max_len), "smem_gpu_reserve_slots")

    def batch(self, max_reads: int, max_bases: int, max_len: int) -> "Batch":
        return Batch(self, max_reads, max_bases, max_len)

    def seed_stream(self, codes: np.ndarray, offs: np.ndarray, opt: "Options" = None, chunk_reads: int = 1 << 20,
                    workers: int = 3, pairs: bool = False, collect: bool = False, packed: bool = False,
                    release: bool = False) -> tuple:
        """Stream a read set through smem_gpu_seed_stream (chunks of
        chunk_reads, `workers` host workers each with its own batch and HIP
        stream; packed: 16-B wire entries; release: free the workers'
        batches instead of keeping them for the next call).  Returns (stats
        dict, per-chunk Results in chunk order when collect else None)."""
        lib = load()
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        o = (opt or Options()).c()
        st = StreamStats()
        got = {}
        err = []

        def on_chunk(ctx, chunk, first, n, bh):
            try:
                got[int(chunk)] = _results_of(lib, bh, n, packed)
                return 0
            except Exception as e:  # surfaced after the stream returns
                err.append(e)
                return -5

        cb = CHUNK_FN(on_chunk) if collect else None
        rc = lib.smem_gpu_seed_stream(self._h, offs.size - 1, codes.ctypes.data, offs.ctypes.data, C.byref(o),
                                      int(chunk_reads), int(workers), (1 if pairs else 0) | (2 if packed else 0) | (4 if release else 0),
                                      C.cast(cb, C.c_void_p) if cb else None, None, C.byref(st))
        if err:
            raise err[0]
        _check(rc, "smem_gpu_seed_stream")
        stats = {k: getattr(st, k) for k, _ in StreamStats._fields_}
        return stats, ([got[k] for k in sorted(got)] if collect else None)

    def ksw_extend(self, kb) -> tuple:
        """ksw_extend2 (software/ksw.c:379) of every task of a synth.KswBatch on
        this device: (results as synth.KSW_RESULT, kernel ms)."""
        from . import synth
        lib = load()
        tasks = np.ascontiguousarray(kb.tasks, dtype=synth.KSW_TASK)
        q = np.ascontiguousarray(kb.q, dtype=np.uint8)
        t = np.ascontiguousarray(kb.t, dtype=np.uint8)
        o = KswOptT()
        for i, v in enumerate(np.asarray(kb.mat, dtype=np.int8)):
            o.mat[i] = int(v)
        o.o_del, o.e_del, o.o_ins, o.e_ins = kb.o_del, kb.e_del, kb.o_ins, kb.e_ins
        out = np.zeros(max(tasks.size, 1), dtype=synth.KSW_RESULT)
        ms = C.c_double()
        _check(lib.smem_ksw_extend(self._h, tasks.size, tasks.ctypes.data, q.ctypes.data, q.size, t.ctypes.data,
                                   t.size, C.byref(o), out.ctypes.data, C.byref(ms)), "smem_ksw_extend")
        return out[:tasks.size], ms.value

    def ksw_align2(self, kb) -> tuple:
        """ksw_align2 (software/ksw.c:342) of every KSWA_TASK of a synth.KswBatch
        on this device: (results as synth.KSWA_RESULT, kernel ms)."""
        return self._ksw_align2(kb, "smem_ksw_align2")

    def ksw_align2_long(self, kb) -> tuple:
        """ksw_align2 with targets of up to KSWA_MAX_TLEN bases, mem_matesw's windows
        (smem_ksw_align2_long): (results as synth.KSWA_RESULT, kernel ms)."""
        return self._ksw_align2(kb, "smem_ksw_align2_long")

    def _ksw_align2(self, kb, entry: str) -> tuple:
        from . import synth
        lib = load()
        tasks = np.ascontiguousarray(kb.tasks, dtype=synth.KSWA_TASK)
        q = np.ascontiguousarray(kb.q, dtype=np.uint8)
        t = np.ascontiguousarray(kb.t, dtype=np.uint8)
        o = KswOptT()
        for i, v in enumerate(np.asarray(kb.mat, dtype=np.int8)):
            o.mat[i] = int(v)
        o.o_del, o.e_del, o.o_ins, o.e_ins = kb.o_del, kb.e_del, kb.o_ins, kb.e_ins
        out = np.zeros(max(tasks.size, 1), dtype=synth.KSWA_RESULT)
        ms = C.c_double()
        _check(getattr(lib, entry)(self._h, tasks.size, tasks.ctypes.data, q.ctypes.data, q.size, t.ctypes.data,
                                   t.size, C.byref(o), out.ctypes.data, C.byref(ms)), entry)
        return out[:tasks.size], ms.value

    def matesw(self, pac, l_pac: int, codes, offs, regs, reg_off, pes, opt: "MateswOptT" = None,
               regs_cap: int | None = None, grow: bool = True) -> tuple:
        """The rescue loop of mem_sam_pe (software/bwamem_pair.c:252-263) of every pair on this
        device (smem_matesw): reads 2p and 2p + 1 are pair p, regs (ALNREG_DT) / reg_off each
        read's regions, pes four (low, high, failed) tuples or PestatT, pac None: the resident
        one.  Returns (regions as ALNREG_DT, reg_off_out, n_sw, status, kernel ms).  The output
        starts at regs_cap regions (default: a guess) and the call is repeated with the size the
        library reports when that is too small (grow=False: SmemError with .n_regs instead)."""
        lib = load()
        if pac is not None:
            pac = np.ascontiguousarray(pac, dtype=np.uint8)
            if pac.size < (int(l_pac) + 3) // 4:
                raise SmemError("matesw: pac holds fewer than (l_pac + 3) / 4 bytes")
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        reg_off = np.ascontiguousarray(reg_off, dtype=np.uint64)
        regs = np.ascontiguousarray(regs)
        if regs.dtype != ALNREG_DT:
            regs = np.frombuffer(regs.astype(np.uint8, copy=False).tobytes(), dtype=ALNREG_DT)
        if offs.size < 1 or offs.size % 2 != 1 or reg_off.size != offs.size:
            raise SmemError("matesw: offs and reg_off need 2 n_pairs + 1 entries")
        if int(reg_off[-1]) > regs.size or int(offs[-1]) > codes.size:
            raise SmemError("matesw: offsets end past their arrays")
        n_pairs = (offs.size - 1) // 2
        pe = (PestatT * 4)()
        for r in range(4):
            if isinstance(pes[r], PestatT):
                pe[r] = pes[r]
            else:
                pe[r].low, pe[r].high, pe[r].failed = (int(x) for x in pes[r][:3])
        if opt is None:
            opt = matesw_opt()
        cap = int(regs_cap) if regs_cap is not None else int(reg_off[-1]) + 2 * n_pairs + 16
        reg_off_out = np.zeros(2 * n_pairs + 1, dtype=np.uint64)
        n_sw = np.zeros(max(n_pairs, 1), dtype=np.int32)
        status = np.zeros(max(n_pairs, 1), dtype=np.int32)
        ms, need = C.c_double(), C.c_uint64()
        while True:
            out = np.zeros(max(cap, 1), dtype=ALNREG_DT)
            rc = lib.smem_matesw(self._h, n_pairs, codes.ctypes.data, offs.ctypes.data, regs.ctypes.data,
                                 reg_off.ctypes.data, C.cast(pe, C.c_void_p), pac.ctypes.data if pac is not None else None,
                                 int(l_pac), C.byref(opt), out.ctypes.data, cap, reg_off_out.ctypes.data,
                                 n_sw.ctypes.data, status.ctypes.data, C.byref(need), C.byref(ms))
            if rc == SMEM_E_CAPACITY and need.value > cap and grow:
                cap = int(need.value)
                continue
            if rc == SMEM_E_CAPACITY and need.value > cap:
                err = SmemError(f"smem_matesw failed: SMEM_E_CAPACITY: the lists need {need.value} regions")
                err.n_regs = int(need.value)
                raise err
            _check(rc, "smem_matesw")
            return out[:int(need.value)], reg_off_out, n_sw[:n_pairs], status[:n_pairs], ms.value

    @staticmethod
    def _pair_lists(what, regs, reg_off):
        reg_off = np.ascontiguousarray(reg_off, dtype=np.uint64)
        regs = np.ascontiguousarray(regs)
        if regs.dtype != ALNREG_DT:
            regs = np.frombuffer(regs.astype(np.uint8, copy=False).tobytes(), dtype=ALNREG_DT)
        if reg_off.size < 1 or reg_off.size % 2 != 1:
            raise SmemError(f"{what}: reg_off needs 2 n_pairs + 1 entries")
        if int(reg_off.max()) > regs.size:
            raise SmemError(f"{what}: reg_off ends past regs")
        return regs, reg_off, (reg_off.size - 1) // 2

    def pestat(self, regs, reg_off, l_pac: int, opt: "PestatOptT" = None) -> tuple:
        """mem_pestat (software/bwamem_pair.c:46-107) on this device (smem_pestat): reads 2p and
        2p + 1 are pair p, regs (ALNREG_DT) / reg_off each read's list after mem_sort_and_dedup.
        Returns (pes as four PESTAT_DT records, n_cand[4], kernel ms)."""
        regs, reg_off, n_pairs = self._pair_lists("pestat", regs, reg_off)
        if opt is None:
            opt = pestat_opt()
        pes = np.zeros(4, dtype=PESTAT_DT)
        n_cand = np.zeros(4, dtype=np.uint64)
        ms = C.c_double()
        _check(load().smem_pestat(self._h, n_pairs, regs.ctypes.data, reg_off.ctypes.data, int(l_pac), C.byref(opt),
                                  pes.ctypes.data, n_cand.ctypes.data, C.byref(ms)), "smem_pestat")
        return pes, n_cand, ms.value

    def pair(self, regs, reg_off, l_pac: int, pes, opt: "PairOptT" = None, ids=None, id0: int = 0) -> tuple:
        """mem_pair and the decision block of mem_sam_pe (software/bwamem_pair.c:177-236, 266-304,
        321-326) of every pair on this device (smem_pair): regs / reg_off each read's list after
        mem_mark_primary_se (Gpu.reg_finalize's order), pes what Gpu.pestat returned (PESTAT_DT),
        four PestatT or four (low, high, failed, avg, std) tuples, ids the pairs' ids (None: id0 + p).
        Returns (PAIR_SEL_DT per pair, kernel ms)."""
        regs, reg_off, n_pairs = self._pair_lists("pair", regs, reg_off)
        if isinstance(pes, np.ndarray) and pes.dtype == PESTAT_DT:
            pe = np.ascontiguousarray(pes)
        else:
            pe = np.zeros(4, dtype=PESTAT_DT)
            for r in range(4):
                x = pes[r]
                t = (x.low, x.high, x.failed, x.avg, x.std) if hasattr(x, "low") else tuple(x)
                pe[r]["low"], pe[r]["high"], pe[r]["failed"], pe[r]["avg"], pe[r]["std"] = t
        if pe.size != 4:
            raise SmemError("pair: pes needs four orientations")
        if opt is None:
            opt = pair_opt()
        if ids is not None:
            ids = np.ascontiguousarray(ids, dtype=np.int64)
            if ids.size != n_pairs:
                raise SmemError("pair: one id per pair")
        sel = np.zeros(max(n_pairs, 1), dtype=PAIR_SEL_DT)
        ms = C.c_double()
        _check(load().smem_pair(self._h, n_pairs, regs.ctypes.data, reg_off.ctypes.data,
                                ids.ctypes.data if ids is not None else None, int(id0), int(l_pac), pe.ctypes.data,
                                C.byref(opt), sel.ctypes.data, C.byref(ms)), "smem_pair")
        return sel[:n_pairs], ms.value

    def load_pac(self, pac, l_pac: int) -> None:
        """Keep the 2-bit .pac resident in HBM (smem_gpu_load_pac)."""
        pac = np.ascontiguousarray(pac, dtype=np.uint8)
        if pac.size < (l_pac + 3) // 4:
            raise SmemError("load_pac: pac holds fewer than (l_pac + 3) / 4 bytes")
        _check(load().smem_gpu_load_pac(self._h, pac.ctypes.data, int(l_pac)), "smem_gpu_load_pac")

    def load_contigs(self, offsets, lens, l_pac: int) -> None:
        """Keep the contig table (bns->anns[].offset / .len) resident for
        Batch.reg2aln (smem_gpu_load_contigs); it must tile [0, l_pac)."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        if offsets.size != lens.size:
            raise SmemError("load_contigs: one length per offset")
        _check(load().smem_gpu_load_contigs(self._h, offsets.size, offsets.ctypes.data, lens.ctypes.data, int(l_pac)),
               "smem_gpu_load_contigs")

    def load_contig_names(self, names) -> None:
        """Keep the contigs' names (bns->anns[].name) resident beside the table of
        load_contigs, one per contig (smem_gpu_load_contig_names): Batch.sam prints them."""
        data, off = pack_strings(names)
        _check(load().smem_gpu_load_contig_names(self._h, len(names), data.ctypes.data, off.ctypes.data),
               "smem_gpu_load_contig_names")

    def sam_text(self, codes, offs, names, quals, comments, aln_off, alns, rid, recs, cigar, md, ctg_offsets, ctg_names,
                 fin_status=None, rg_id=None, text_cap: int | None = None, grow: bool = True) -> "SamResults":
        """mem_reg2sam_se's text of every read over host buffers (smem_sam_text): names /
        comments as lists (comments None: none), quals a uint8 array by offs (None: '*'), alns
        as ALN_DT with rid (int32) and recs (SAM_REC_DT) per record, aln_off the reads' records,
        cigar / md the pools alns points into, the contigs' offsets and names.  The text buffer
        starts at text_cap bytes (default: a guess) and the call is repeated with the size the
        library reports when it is too small (grow=False: SmemError with .n_bytes instead)."""
        return self._sam_text(None, codes, offs, names, quals, comments, aln_off, alns, rid, recs, cigar, md, ctg_offsets,
                              ctg_names, fin_status, rg_id, text_cap, grow)

    def _sam_text(self, _sel, codes, offs, names, quals, comments, aln_off, alns, rid, recs, cigar, md, ctg_offsets,
                  ctg_names, fin_status, rg_id, text_cap, grow) -> "SamResults":
        """sam_text (_sel None) and sam_text_pe: one marshalling of the host buffers for both calls"""
        lib = load()
        fn = "smem_sam_text" if _sel is None else "smem_sam_text_pe"
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        n = offs.size - 1
        nm, nm_off = pack_strings(names)
        if quals is not None:
            quals = np.ascontiguousarray(quals, dtype=np.uint8)
            if quals.size < int(offs[-1]):
                raise SmemError("sam_text: one quality per base")
        cm = cm_off = None
        if comments is not None:
            cm, cm_off = pack_strings(comments)
        aln_off = np.ascontiguousarray(aln_off, dtype=np.uint64)
        alns = np.ascontiguousarray(alns, dtype=ALN_DT)
        rid = np.ascontiguousarray(rid, dtype=np.int32)
        recs = np.ascontiguousarray(recs, dtype=SAM_REC_DT)
        cigar = np.ascontiguousarray(cigar, dtype=np.uint32)
        md = np.ascontiguousarray(md, dtype=np.uint8)
        if len(names) != n or aln_off.size != n + 1 or (comments is not None and len(comments) != n):
            raise SmemError("sam_text: one name (and comment) per read, aln_off of n_reads + 1 entries")
        n_rec = int(aln_off[-1]) if n >= 0 and aln_off.size else 0
        if alns.size < n_rec or rid.size < n_rec or recs.size < n_rec:
            raise SmemError("sam_text: aln_off ends past the records")
        ctg_offsets = np.ascontiguousarray(ctg_offsets, dtype=np.int64)
        cn, cn_off = pack_strings(ctg_names)
        if len(ctg_names) != ctg_offsets.size:
            raise SmemError("sam_text: one name per contig")
        if fin_status is not None:
            fin_status = np.ascontiguousarray(fin_status, dtype=np.int32)
            if fin_status.size != n:
                raise SmemError("sam_text: one finalize status per read")
        opt = SamOptT(rg_id.encode("latin-1") if rg_id else None)
        cap = int(text_cap) if text_cap is not None else 2 * int(offs[-1]) + 160 * (n_rec + n) + 256
        text_off = np.zeros(n + 1, dtype=np.uint64)
        status = np.zeros(max(n, 1), dtype=np.int32)
        ms, nb = C.c_double(), C.c_uint64()

        def ptr(a):
            return a.ctypes.data if a is not None else None
        while True:
            text = np.zeros(max(cap, 1), dtype=np.uint8)
            args = (n, ptr(codes), ptr(offs), ptr(nm), ptr(nm_off), ptr(quals), ptr(cm), ptr(cm_off), ptr(aln_off),
                    ptr(alns), ptr(rid), ptr(recs), ptr(fin_status), ptr(cigar), cigar.size, ptr(md), md.size,
                    ctg_offsets.size, ptr(ctg_offsets), ptr(cn), ptr(cn_off), C.byref(opt), ptr(text), cap, ptr(text_off),
                    ptr(status), C.byref(nb), C.byref(ms))
            if _sel is None:
                rc = lib.smem_sam_text(self._h, *args)
            else:
                rc = lib.smem_sam_text_pe(self._h, _sel.size, ptr(_sel), *args)
            if rc == SMEM_E_CAPACITY and nb.value > cap and grow:
                cap = int(nb.value)
                continue
            if rc == SMEM_E_CAPACITY:
                err = SmemError(f"{fn} failed: SMEM_E_CAPACITY: the text needs {nb.value} bytes")
                err.n_bytes = int(nb.value)
                raise err
            _check(rc, fn)
            return SamResults(text[:int(nb.value)], text_off, status[:n], ms.value)

    def sam_text_pe(self, sel, codes, offs, names, quals, comments, aln_off, alns, rid, recs, cigar, md, ctg_offsets,
                    ctg_names, fin_status=None, rg_id=None, text_cap: int | None = None,
                    grow: bool = True) -> "SamResults":
        """The paired-end text of every pair over host buffers (smem_sam_text_pe: the tail of
        mem_sam_pe, mem_aln2sam with a mate): sam_text's arguments with sel, the PAIR_SEL_DT array
        Gpu.pair returns, one per pair; reads 2p and 2p + 1 are pair p.  Each read's records are
        the finalize selection's list in branch 0 and the one alignment of region z[e] (flag 0,
        xs = max(sub, csub)) in branch 1 and 2, where sel's mapq is printed.  Returns SamResults
        as sam_text; both reads of a pair left to the caller have status SAM_HOST."""
        sel = np.ascontiguousarray(sel, dtype=PAIR_SEL_DT)
        return self._sam_text(sel, codes, offs, names, quals, comments, aln_off, alns, rid, recs, cigar, md, ctg_offsets,
                              ctg_names, fin_status, rg_id, text_cap, grow)

    def chain2aln(self, pac, l_pac: int, codes, offs, chains, chain_off, seeds, opt) -> tuple:
        """mem_chain2aln_short / mem_chain2aln of every chain of every read
        (software/bwamem.c:1452-1460) on this device.  opt is a ctypes struct
        laid out as smem_aln_opt_t.  Returns (regions as 64-byte smem_alnreg_t
        records, reg_off[n_reads + 1], kernel ms)."""
        lib = load()
        if pac is not None:
            pac = np.ascontiguousarray(pac, dtype=np.uint8)
            if pac.size < (int(l_pac) + 3) // 4:
                raise SmemError("chain2aln: pac holds fewer than (l_pac + 3) / 4 bytes")
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        chain_off = np.ascontiguousarray(chain_off, dtype=np.uint64)
        chains = np.ascontiguousarray(chains, dtype=CHAIN_DT)
        seeds = np.ascontiguousarray(seeds, dtype=SEED_DT)
        if chain_off.size != offs.size or (chain_off.size and int(chain_off[-1]) > chains.size):
            raise SmemError("chain2aln: chain_off must have n_reads + 1 entries within chains")
        n = offs.size - 1
        cap = int(chains["n"].sum()) if chains.size else 0
        regs = np.zeros(max(cap, 1) * 64, dtype=np.uint8)
        reg_off = np.zeros(n + 1, dtype=np.uint64)
        ms = C.c_double()
        _check(lib.smem_chain2aln(self._h, n, codes.ctypes.data, offs.ctypes.data, chains.ctypes.data,
                                  chain_off.ctypes.data, seeds.ctypes.data, seeds.size,
                                  pac.ctypes.data if pac is not None else None, l_pac,
                                  C.byref(opt), regs.ctypes.data, reg_off.ctypes.data, C.byref(ms)), "smem_chain2aln")
        return regs[:int(reg_off[-1]) * 64], reg_off, ms.value

    def reg2aln(self, pac, l_pac: int, codes, offs, regs, reg_off, opt, cigar_cap: int | None = None,
                md_cap: int | None = None) -> tuple:
        """The alignment part of mem_reg2aln (software/bwamem.c:1504-1547) of
        every region on this device (smem_reg2aln): regs are smem_alnreg_t
        records (ALNREG_DT, or the raw bytes chain2aln returns), reg_off the
        regions of each read, pac None for the resident .pac.  Returns (alns
        as ALN_DT, cigar words, md bytes, kernel ms); region k's CIGAR is
        cigar[cigar_off : cigar_off + n_cigar] and its MD md[md_off : md_off +
        md_len].  The pools start at cigar_cap words / md_cap bytes (default:
        a guess from the regions) and the call is repeated with the sizes the
        library reports when they are too small."""
        lib = load()
        if pac is not None:
            pac = np.ascontiguousarray(pac, dtype=np.uint8)
            if pac.size < (int(l_pac) + 3) // 4:
                raise SmemError("reg2aln: pac holds fewer than (l_pac + 3) / 4 bytes")
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        reg_off = np.ascontiguousarray(reg_off, dtype=np.uint64)
        regs = np.ascontiguousarray(regs)
        if regs.dtype != ALNREG_DT:
            regs = np.frombuffer(regs.astype(np.uint8, copy=False).tobytes(), dtype=ALNREG_DT)
        if reg_off.size != offs.size or (reg_off.size and int(reg_off[-1]) > regs.size):
            raise SmemError("reg2aln: reg_off must have n_reads + 1 entries within regs")
        n = offs.size - 1
        n_regs = int(reg_off[-1]) if reg_off.size else 0
        alns = np.zeros(max(n_regs, 1), dtype=ALN_DT)
        cap_c = 8 * n_regs if cigar_cap is None else int(cigar_cap)
        cap_m = 24 * n_regs if md_cap is None else int(md_cap)
        ms = C.c_double()
        while True:
            cigar = np.zeros(max(cap_c, 1), dtype=np.uint32)
            md = np.zeros(max(cap_m, 1), dtype=np.uint8)
            nc, nm = C.c_uint64(), C.c_uint64()
            rc = lib.smem_reg2aln(self._h, n, codes.ctypes.data, offs.ctypes.data, regs.ctypes.data,
                                  reg_off.ctypes.data, pac.ctypes.data if pac is not None else None, l_pac,
                                  C.byref(opt), alns.ctypes.data, cigar.ctypes.data, cap_c, C.byref(nc),
                                  md.ctypes.data, cap_m, C.byref(nm), C.byref(ms))
            if rc == SMEM_E_CAPACITY and (nc.value > cap_c or nm.value > cap_m):
                cap_c, cap_m = max(cap_c, int(nc.value)), max(cap_m, int(nm.value))
                continue
            _check(rc, "smem_reg2aln")
            return alns[:n_regs], cigar[:int(nc.value)], md[:int(nm.value)], ms.value

    def reg_finalize(self, read_len, regs, reg_off, opt: FinOptT = None, ids=None, id0: int = 0) -> FinResults:
        """mem_sort_and_dedup, mem_mark_primary_se and the selection, MAPQ and
        flags of mem_reg2sam_se for every read's raw regions (smem_reg_finalize):
        regs as ALNREG_DT (or the raw bytes chain2aln returns), reg_off their
        reads, read_len the reads' lengths, ids the per-read hash ids (None:
        id0 + r).  regs[sel_idx] of the result is reg2aln's input."""
        lib = load()
        read_len = np.ascontiguousarray(read_len, dtype=np.int32)
        reg_off = np.ascontiguousarray(reg_off, dtype=np.uint64)
        regs = np.ascontiguousarray(regs)
        if regs.dtype != ALNREG_DT:
            regs = np.frombuffer(regs.astype(np.uint8, copy=False).tobytes(), dtype=ALNREG_DT)
        n = read_len.size
        if reg_off.size != n + 1 or int(reg_off[-1]) > regs.size:
            raise SmemError("reg_finalize: reg_off must have n_reads + 1 entries within regs")
        if ids is not None:
            ids = np.ascontiguousarray(ids, dtype=np.int64)
            if ids.size != n:
                raise SmemError("reg_finalize: one id per read")
        if opt is None:
            opt = fin_opt()
        cap = max(int(reg_off[-1]), 1)
        out = np.zeros(cap, dtype=ALNREG_DT)
        sel = np.zeros(cap, dtype=FIN_SEL_DT)
        sel_idx = np.zeros(cap, dtype=np.uint64)
        out_off = np.zeros(n + 1, dtype=np.uint64)
        sel_off = np.zeros(n + 1, dtype=np.uint64)
        status = np.zeros(max(n, 1), dtype=np.int32)
        ms = C.c_double()
        _check(lib.smem_reg_finalize(self._h, n, read_len.ctypes.data, regs.ctypes.data, reg_off.ctypes.data,
                                     ids.ctypes.data if ids is not None else None, int(id0), C.byref(opt),
                                     out.ctypes.data, out_off.ctypes.data, sel.ctypes.data, sel_idx.ctypes.data,
                                     sel_off.ctypes.data, status.ctypes.data, C.byref(ms)), "smem_reg_finalize")
        no, ns = int(out_off[-1]), int(sel_off[-1])
        return FinResults(out[:no], out_off, sel[:no], sel_idx[:ns], sel_off, status[:n], ms.value)

    def close(self) -> None:
        if self._h:
            load().smem_gpu_shutdown(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Batch:
    """A worker's device-resident reads and results (smem_batch_*)."""

    def __init__(self, gpu: Gpu, max_reads: int, max_bases: int, max_len: int):
        self._gpu = gpu
        self._h = C.c_void_p()
        _check(load().smem_batch_create(gpu._h, max_reads, max_bases, max_len, C.byref(self._h)), "smem_batch_create")

    def set_reads(self, codes: np.ndarray, offs: np.ndarray) -> None:
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        self._keep = (codes, offs)
        _check(load().smem_batch_set_reads_packed(self._h, offs.size - 1, codes.ctypes.data, offs.ctypes.data),
               "smem_batch_set_reads_packed")

    @property
    def n_reads(self) -> int:
        return int(self._keep[1].size - 1)

    def run(self, opt: Options = Options()) -> None:
        o = opt.c()
        _check(load().smem_batch_run(self._h, C.byref(o)), "smem_batch_run")

    def memory(self) -> tuple:
        """(device bytes, pinned host bytes) this batch holds (smem_batch_memory)."""
        d, h = C.c_uint64(), C.c_uint64()
        _check(load().smem_batch_memory(self._h, C.byref(d), C.byref(h)), "smem_batch_memory")
        return d.value, h.value

    def stats(self) -> dict:
        s = BatchStats()
        _check(load().smem_batch_stats(self._h, C.byref(s)), "smem_batch_stats")
        out = {k: getattr(s, k) for k, _ in BatchStats._fields_}
        if hasattr(load(), "smem_batch_sam_stats"):  # Batch.sam's, from their own struct (smem_batch_sam_stats)
            t = SamStats()
            _check(load().smem_batch_sam_stats(self._h, C.byref(t)), "smem_batch_sam_stats")
            out.update({k: getattr(t, k) for k, _ in SamStats._fields_})
        return out

    def sa(self, min_seed_len: int = 19, max_occ: int = 10000) -> None:
        """bwt_sa of every seed occurrence of the last run (smem_batch_sa)."""
        _check(load().smem_batch_sa(self._h, min_seed_len, max_occ), "smem_batch_sa")

    def chain(self, l_pac: int, w: int = 100, max_chain_gap: int = 10000, mask_level: float = 0.5,
              drop_ratio: float = 0.5, filter: bool = True) -> None:
        """mem_chain (+ mem_chain_flt) of every read of the last run, over
        the positions of the last sa() (smem_batch_chain)."""
        o = ChainOptT(w, max_chain_gap, mask_level, drop_ratio, int(bool(filter)))
        _check(load().smem_batch_chain(self._h, int(l_pac), C.byref(o)), "smem_batch_chain")

    def chain2aln(self, opt) -> None:
        """mem_chain2aln_short / mem_chain2aln of every chain of the last
        chain(filter=True), over the chains in HBM and the resident .pac
        (smem_batch_chain2aln); opt is laid out as smem_aln_opt_t."""
        _check(load().smem_batch_chain2aln(self._h, C.byref(opt)), "smem_batch_chain2aln")

    def reg_finalize(self, opt: FinOptT = None, ids=None, id0: int = 0) -> None:
        """Raw regions -> final regions, marks, selection, MAPQ and flags of
        every read of the last chain2aln(), over the regions in HBM
        (smem_batch_reg_finalize); fetch(FETCH_FIN) returns them as .fin."""
        if opt is None:
            opt = fin_opt()
        if ids is not None:
            ids = np.ascontiguousarray(ids, dtype=np.int64)
            if ids.size != self.n_reads:
                raise SmemError("reg_finalize: one id per read")
        _check(load().smem_batch_reg_finalize(self._h, ids.ctypes.data if ids is not None else None, int(id0),
                                              C.byref(opt)), "smem_batch_reg_finalize")

    def reg2aln(self, opt, idx=None, idx_off=None) -> None:
        """CIGAR, NM, MD, position and contig of every record of the last
        reg_finalize(), over the final regions in HBM (smem_batch_reg2aln);
        opt is laid out as smem_aln_opt_t.  idx / idx_off: the caller's own
        records instead of the stage's selection, as indices into the final
        regions with per-read offsets.  fetch(FETCH_ALN) returns them as .aln."""
        if (idx is None) != (idx_off is None):
            raise SmemError("reg2aln: idx and idx_off go together")
        pi = po = None
        if idx is not None:
            idx = np.ascontiguousarray(idx, dtype=np.uint64)
            idx_off = np.ascontiguousarray(idx_off, dtype=np.uint64)
            if idx_off.size != self.n_reads + 1 or int(idx_off[-1]) != idx.size:
                raise SmemError("reg2aln: idx_off must have n_reads + 1 entries and end at idx.size")
            pi, po = idx.ctypes.data, idx_off.ctypes.data
        _check(load().smem_batch_reg2aln(self._h, C.byref(opt), pi, po), "smem_batch_reg2aln")

    def set_read_text(self, names, quals=None, comments=None) -> None:
        """The names (one per read, at most 255 bytes), qualities (a uint8 array over all
        reads in batch order, or None: '*') and comments (a list, or None) Batch.sam prints
        (smem_batch_set_read_text); a later set_reads ends them."""
        n = self.n_reads
        if len(names) != n or (comments is not None and len(comments) != n):
            raise SmemError("set_read_text: one name (and comment) per read")
        nm, nm_off = pack_strings(names)
        q = None
        if quals is not None:
            q = np.ascontiguousarray(quals, dtype=np.uint8)
            if q.size != int(self._keep[1][-1] - self._keep[1][0]):
                raise SmemError("set_read_text: one quality per base")
        cm = cm_off = None
        if comments is not None:
            cm, cm_off = pack_strings(comments)
        _check(load().smem_batch_set_read_text(self._h, nm.ctypes.data, nm_off.ctypes.data,
                                               q.ctypes.data if q is not None else None,
                                               cm.ctypes.data if cm is not None else None,
                                               cm_off.ctypes.data if cm_off is not None else None),
               "smem_batch_set_read_text")

    def sam(self, rg_id=None) -> None:
        """mem_reg2sam_se's text of every read of the last reg2aln() (the stage's own
        selection, with a contig table and names, after set_read_text), in HBM
        (smem_batch_sam); fetch(FETCH_SAM) returns it as .sam."""
        opt = SamOptT(rg_id.encode("latin-1") if rg_id else None)
        _check(load().smem_batch_sam(self._h, C.byref(opt)), "smem_batch_sam")

    def debug_words(self, n_words: int) -> np.ndarray:
        out = np.zeros(n_words, dtype=np.uint64)
        rc = load().smem_batch_debug(self._h, out.ctypes.data, n_words)
        if rc < 0:
            _check(rc, "smem_batch_debug")
        return out[:rc]

    def fetch(self, mask: int | None = None) -> Results:
        """Copy the outputs back (smem_batch_fetch: every stage that ran; with
        `mask`, smem_batch_fetch_mask: only the FETCH_* outputs named) and
        return copies of them."""
        lib = load()
        if mask is None:
            _check(lib.smem_batch_fetch(self._h), "smem_batch_fetch")
        else:
            _check(lib.smem_batch_fetch_mask(self._h, int(mask)), "smem_batch_fetch_mask")
        n = int(self._keep[1].size - 1)
        if mask is None or mask & FETCH_INTV:
            res = _results_of(lib, self._h, n)
        else:
            res = Results(None, None, None, None)
        ni = int(res.intv_off[-1]) if res.intv_off is not None else int(self.stats()["n_intv"])
        pos = C.POINTER(C.c_uint64)()
        oo = C.POINTER(C.c_uint64)()
        no = C.c_uint64()
        if lib.smem_batch_sa_results(self._h, C.byref(pos), C.byref(oo), C.byref(no)) == 0:
            n_occ = int(no.value)
            res.occ_off = np.ctypeslib.as_array(oo, shape=(ni + 1,)).copy()
            res.sa_pos = np.ctypeslib.as_array(pos, shape=(max(n_occ, 1),))[:n_occ].copy()
        ch, sd = C.c_void_p(), C.c_void_p()
        cho = C.POINTER(C.c_uint64)()
        nch, nsd = C.c_uint64(), C.c_uint64()
        if lib.smem_batch_chain_results(self._h, C.byref(ch), C.byref(cho), C.byref(sd), C.byref(nch),
                                        C.byref(nsd)) == 0:
            nc, ns = int(nch.value), int(nsd.value)
            res.chain_off = np.ctypeslib.as_array(cho, shape=(n + 1,)).copy()
            res.chains = np.frombuffer((C.c_char * (max(nc, 1) * CHAIN_DT.itemsize)).from_address(ch.value),
                                       dtype=CHAIN_DT)[:nc].copy()
            res.seeds = np.frombuffer((C.c_char * (max(ns, 1) * SEED_DT.itemsize)).from_address(sd.value),
                                      dtype=SEED_DT)[:ns].copy()
        rg = C.c_void_p()
        ro = C.POINTER(C.c_uint64)()
        nr = C.c_uint64()
        if lib.smem_batch_aln_results(self._h, C.byref(rg), C.byref(ro), C.byref(nr)) == 0:
            k = int(nr.value)
            res.reg_off = np.ctypeslib.as_array(ro, shape=(n + 1,)).copy()
            res.regs = np.frombuffer((C.c_char * (max(k, 1) * 64)).from_address(rg.value), dtype=np.uint8)[:k * 64].copy()
        fr, fs = C.c_void_p(), C.c_void_p()
        fo, fi, fso = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint64)()
        fst = C.POINTER(C.c_int32)()
        nf, nfs = C.c_uint64(), C.c_uint64()
        if lib.smem_batch_fin_results(self._h, C.byref(fr), C.byref(fo), C.byref(fs), C.byref(fi), C.byref(fso),
                                      C.byref(fst), C.byref(nf), C.byref(nfs)) == 0:
            k, ks = int(nf.value), int(nfs.value)
            res.fin = FinResults(
                np.frombuffer((C.c_char * (max(k, 1) * 64)).from_address(fr.value), dtype=ALNREG_DT)[:k].copy(),
                np.ctypeslib.as_array(fo, shape=(n + 1,)).copy(),
                np.frombuffer((C.c_char * (max(k, 1) * 12)).from_address(fs.value), dtype=FIN_SEL_DT)[:k].copy(),
                np.ctypeslib.as_array(fi, shape=(max(ks, 1),))[:ks].copy(),
                np.ctypeslib.as_array(fso, shape=(n + 1,)).copy(),
                np.ctypeslib.as_array(fst, shape=(max(n, 1),))[:n].copy(), self.stats()["fin_ms"])
        al, cg, mdp = C.c_void_p(), C.POINTER(C.c_uint32)(), C.c_void_p()
        ri, ao = C.POINTER(C.c_int32)(), C.POINTER(C.c_uint64)()
        ncw, nmb, nal = C.c_uint64(), C.c_uint64(), C.c_uint64()
        if lib.smem_batch_aln2_results(self._h, C.byref(al), C.byref(ri), C.byref(ao), C.byref(cg), C.byref(ncw),
                                       C.byref(mdp), C.byref(nmb), C.byref(nal)) == 0:
            k, kc, km = int(nal.value), int(ncw.value), int(nmb.value)
            res.aln = AlnResults(
                np.frombuffer((C.c_char * (max(k, 1) * ALN_DT.itemsize)).from_address(al.value), dtype=ALN_DT)[:k].copy(),
                np.ctypeslib.as_array(ri, shape=(max(k, 1),))[:k].copy(),
                np.ctypeslib.as_array(ao, shape=(n + 1,)).copy(),
                np.ctypeslib.as_array(cg, shape=(max(kc, 1),))[:kc].copy(),
                np.frombuffer((C.c_char * max(km, 1)).from_address(mdp.value), dtype=np.uint8)[:km].copy())
        tx, to, ts, tb = C.c_void_p(), C.POINTER(C.c_uint64)(), C.POINTER(C.c_int32)(), C.c_uint64()
        if lib.smem_batch_sam_results(self._h, C.byref(tx), C.byref(to), C.byref(ts), C.byref(tb)) == 0:
            k = int(tb.value)
            res.sam = SamResults(
                np.frombuffer((C.c_char * max(k, 1)).from_address(tx.value), dtype=np.uint8)[:k].copy(),
                np.ctypeslib.as_array(to, shape=(n + 1,)).copy(),
                np.ctypeslib.as_array(ts, shape=(max(n, 1),))[:n].copy(), self.stats()["sam_ms"])
        return res

    def close(self) -> None:
        if self._h:
            load().smem_batch_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def unpack_pintv(p: np.ndarray) -> np.ndarray:
    """(N, 4) uint32 smem_pintv_t entries -> (N, 4) uint64 bwtintv_t (smem_pintv_unpack)."""
    p = p.astype(np.uint64)
    w = p[:, 3]
    out = np.empty((p.shape[0], 4), dtype=np.uint64)
    out[:, 0] = (w & np.uint64(3)) << np.uint64(32) | p[:, 0]
    out[:, 1] = ((w >> np.uint64(2)) & np.uint64(3)) << np.uint64(32) | p[:, 1]
    out[:, 2] = ((w >> np.uint64(4)) & np.uint64(3)) << np.uint64(32) | p[:, 2]
    out[:, 3] = ((w >> np.uint64(6)) & np.uint64(8191)) << np.uint64(32) | (w >> np.uint64(19))
    return out


def _results_of(lib, bh, n: int, packed: bool = False) -> Results:
    """Copies of a fetched batch's interval lists (smem_batch_results, or the
    packed view unpacked)."""
    iv = C.POINTER(Intv)()
    pv = C.c_void_p()
    io = C.POINTER(C.c_uint64)()
    cn = C.POINTER(C.c_uint32)()
    co = C.POINTER(C.c_uint64)()
    if packed:
        _check(lib.smem_batch_results_packed(bh, C.byref(pv), C.byref(io), C.byref(cn), C.byref(co)),
               "smem_batch_results_packed")
    else:
        _check(lib.smem_batch_results(bh, C.byref(iv), C.byref(io), C.byref(cn), C.byref(co)), "smem_batch_results")
    intv_off = np.ctypeslib.as_array(io, shape=(n + 1,)).copy()
    call_off = np.ctypeslib.as_array(co, shape=(n + 1,)).copy()
    ni, nc = int(intv_off[-1]), int(call_off[-1])
    if packed:
        raw = np.ctypeslib.as_array(C.cast(pv, C.POINTER(C.c_uint32)), shape=(max(ni, 1) * 4,))[:ni * 4]
        intv = unpack_pintv(raw.reshape(ni, 4))
    else:
        intv = (np.ctypeslib.as_array(C.cast(iv, C.POINTER(C.c_uint64)), shape=(max(ni, 1) * 4,))[:ni * 4]
                .reshape(ni, 4).copy())
    call_n = np.ctypeslib.as_array(cn, shape=(max(nc, 1),))[:nc].copy()
    return Results(intv, intv_off, call_n, call_off)


def seed(gpu: Gpu, codes: np.ndarray, offs: np.ndarray, opt: Options = Options()) -> Results:
    """Seed all reads on the GPU (one batch) and return the results."""
    offs = np.asarray(offs, dtype=np.uint64)
    lens = np.diff(offs)
    b = gpu.batch(max(1, offs.size - 1), max(1, int(offs[-1] - offs[0])), max(1, int(lens.max()) if lens.size else 1))
    try:
        b.set_reads(codes, offs)
        b.run(opt)
        return b.fetch()
    finally:
        b.close()
