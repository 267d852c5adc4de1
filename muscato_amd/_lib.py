"""ctypes loader of libmuscato_hip.so.  Fails loudly: there is no CPU fallback."""
from __future__ import annotations

import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# MUSC_LIB_PATH: another build of the same library (kernel experiments)
LIB_PATH = os.environ.get("MUSC_LIB_PATH") or os.path.join(HERE, "libmuscato_hip.so")

MUSC_MAX_WINDOWS = 16


class MuscHit(ctypes.Structure):
    _fields_ = [("read_idx", ctypes.c_uint32), ("gene_idx", ctypes.c_uint32),
                ("pos", ctypes.c_uint32), ("nmiss", ctypes.c_uint32)]


class MuscParams(ctypes.Structure):
    _fields_ = [
        ("n_windows", ctypes.c_int32),
        ("windows", ctypes.c_int32 * MUSC_MAX_WINDOWS),
        ("window_width", ctypes.c_int32),
        ("pmatch", ctypes.c_double),
        ("min_dinuc", ctypes.c_int32),
        ("max_read_length", ctypes.c_int32),
        ("max_matches", ctypes.c_int32),
        ("match_mode", ctypes.c_int32),
        ("mmtol", ctypes.c_int32),
        ("apply_mmtol", ctypes.c_int32),
        ("max_mismatch_p1", ctypes.c_int32),
        ("skip_block_check", ctypes.c_int32),
        ("n_shards", ctypes.c_int32),
        ("reserved", ctypes.c_int32 * 2),
    ]


class MuscStats(ctypes.Structure):
    _fields_ = [
        ("n_reads", ctypes.c_uint64), ("n_read_windows", ctypes.c_uint64),
        ("n_candidates", ctypes.c_uint64), ("n_pairs", ctypes.c_uint64), ("n_accepted", ctypes.c_uint64),
        ("n_hits", ctypes.c_uint64), ("n_overflow_blocks", ctypes.c_uint64),
        ("confirm_bytes", ctypes.c_uint64),
        ("confirm_launches", ctypes.c_uint32), ("n_batches", ctypes.c_uint32),
        ("ms_screen", ctypes.c_float), ("ms_scan", ctypes.c_float), ("match_variant", ctypes.c_uint32),
        ("ms_confirm", ctypes.c_float), ("ms_select", ctypes.c_float), ("ms_total", ctypes.c_float),
        ("ms_index_build", ctypes.c_float), ("ms_read_prep", ctypes.c_float),
        ("n_descriptors", ctypes.c_uint64),
        ("index_kind", ctypes.c_uint32), ("match_launches", ctypes.c_uint32),
        ("n_overflow_entries", ctypes.c_uint64), ("match_bytes", ctypes.c_uint64),
        ("match_bytes_strict", ctypes.c_uint64), ("index_bytes", ctypes.c_uint64),
    ]


class MuscFastqPrep(ctypes.Structure):
    _fields_ = [
        ("n_records", ctypes.c_uint64), ("n_short", ctypes.c_uint64), ("n_reads", ctypes.c_uint64), ("n_unique", ctypes.c_uint64),
        ("max_len", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
        ("name_off", ctypes.POINTER(ctypes.c_uint64)), ("seq_off", ctypes.POINTER(ctypes.c_uint64)),
        ("name_len", ctypes.POINTER(ctypes.c_uint32)), ("seq_len", ctypes.POINTER(ctypes.c_uint32)),
        ("order", ctypes.POINTER(ctypes.c_uint32)), ("ustart", ctypes.POINTER(ctypes.c_uint32)),
    ]


class MuscReadNames(ctypes.Structure):
    _fields_ = [
        ("text_bytes", ctypes.c_uint64), ("line_bytes", ctypes.c_uint64),
        ("n_single", ctypes.c_uint64), ("n_counted", ctypes.c_uint64), ("n_sorted", ctypes.c_uint64),
        ("n_pairs", ctypes.c_uint64),
        ("key_passes", ctypes.c_uint32), ("ms_names", ctypes.c_float),
        ("ranked", ctypes.POINTER(ctypes.c_uint32)),
    ]


class MuscDbTextInfo(ctypes.Structure):
    _fields_ = [
        ("n_targets", ctypes.c_uint64), ("n_bases", ctypes.c_uint64), ("n_odd", ctypes.c_uint64),
        ("first_odd_target", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
        ("n_text_bytes", ctypes.c_uint64), ("n_chunks", ctypes.c_uint64),
        ("ms_decode", ctypes.c_float), ("ms_parse", ctypes.c_float),
    ]


class MuscTargetsPrepInfo(ctypes.Structure):
    _fields_ = [
        ("n_lines", ctypes.c_uint64), ("n_records", ctypes.c_uint64), ("n_targets", ctypes.c_uint64),
        ("n_dropped", ctypes.c_uint64), ("stop_line", ctypes.c_uint64), ("n_subx", ctypes.c_uint64),
        ("n_seq_bytes", ctypes.c_uint64), ("n_id_bytes", ctypes.c_uint64),
        ("ms", ctypes.c_float), ("reserved", ctypes.c_uint32),
    ]


_int, _i32, _u32, _u64, _f32 = ctypes.c_int, ctypes.c_int32, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_float
_vp, _str, _P = ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER
_TEXT_RANGE = [_vp, _int, _u64, _u64, _vp, _u64, _int, _P(_u64)]          # (ctx, which, rec0, nrec, dst, capacity, dst_on_device, &nbytes)
_LAST_MS = [_vp, _P(_f32), _P(_f32)]
_GATHER = [_P(_vp), _int, _P(_u64), _P(_vp), _P(_u64)]
_SZ_WRITE = [_vp, _vp, _u64, _int, _vp, _u64, _int, _P(_u64)]

# The binding, stated once: every prototype of include/muscato_hip.h in the header's order, name -> (restype, argtypes).
# tests/test_abi.py holds each row to the header type for type, and the seven structs above to a compiled C program.
PROTOTYPES = {
    "musc_abi_version": (_int, []),
    "musc_init": (_int, [_int, _P(_vp)]),
    "musc_destroy": (None, [_vp]),
    "musc_last_error": (_str, [_vp]),
    "musc_reload_env": (_int, [_vp]),
    "musc_db_load_ascii": (_int, [_vp, _vp, _vp, _u32, _int]),
    "musc_db_load_packed": (_int, [_vp, _vp, _vp, _vp, _u32]),
    "musc_db_build_index": (_int, [_vp, _i32]),
    "musc_db_build_index_for": (_int, [_vp, _P(MuscParams), _i32]),
    "musc_db_set_partition_bases": (_int, [_vp, _u64]),
    "musc_db_partitions": (_int, [_vp, _vp, _u32, _P(_u32)]),
    "musc_reads_load_ascii": (_int, [_vp, _vp, _vp, _u64, _int]),
    "musc_reads_load_packed": (_int, [_vp, _vp, _vp, _vp, _u64]),
    "musc_reads_load_packed32": (_int, [_vp, _vp, _vp, _vp, _u32, _u64, _int]),
    "musc_reads_sort_unique": (_int, [_vp, _vp, _vp, _u64, _int, _P(_vp), _P(_vp), _P(_u64)]),
    "musc_reads_prep_fastq": (_int, [_vp, _vp, _u64, _int, _i32, _i32, _P(MuscFastqPrep)]),
    "musc_fastq_prep_free": (None, [_P(MuscFastqPrep)]),
    "musc_reads_names_order": (_int, [_vp, _vp, _u64, _int, _vp, _vp, _u64, _vp, _vp, _u64, _vp]),
    "musc_reads_prep_fastq_names": (_int, [_vp, _vp, _u64, _int, _i32, _i32, _P(MuscFastqPrep), _P(MuscReadNames)]),
    "musc_reads_names_text": (_int, _TEXT_RANGE),
    "musc_match_device": (_int, [_vp, _P(MuscParams), _P(_u64)]),
    "musc_hits_copy": (_int, [_vp, _vp, _u64, _int]),
    "musc_hits_copy_packed": (_int, [_vp, _vp, _u64, _int, _u64, _P(_i32)]),
    "musc_hits_unpack": (_int, [_vp, _vp, _u64, _int, _P(_i32), _vp]),
    "musc_hits_copy_compact": (_int, [_vp, _vp, _u64, _vp, _u64, _int, _P(_i32)]),
    "musc_match": (_int, [_vp, _P(MuscParams), _P(_vp), _P(_u64)]),
    "musc_free_hits": (None, [_vp]),
    "musc_get_stats": (_int, [_vp, _P(MuscStats)]),
    "musc_results_set_gene_text": (_int, [_vp, _vp, _vp, _vp, _u32]),
    "musc_results_set_read_text": (_int, [_vp, _vp, _vp, _u64]),
    "musc_results_order": (_int, [_vp, _vp, _u64, _int, _P(_u64), _P(_u64)]),
    "musc_results_hits": (_int, [_vp, _vp, _u64, _int]),
    "musc_results_text": (_int, [_vp, _u64, _u64, _vp, _u64, _int, _P(_u64)]),
    "musc_results_last_ms": (_int, _LAST_MS),
    "musc_results_number_key": (_int, [_u32, _u32, _P(_u64)]),
    "musc_side_prepare": (_int, [_vp, _P(_u64), _P(_u64)]),
    "musc_side_text": (_int, _TEXT_RANGE),
    "musc_side_last_ms": (_int, _LAST_MS),
    "musc_last_instance": (_int, [_vp, _P(_u32)]),
    "musc_instances": (_int, [_P(_u32), _u32, _P(_u32)]),
    "musc_stream_plan": (_int, [_u64, _u32, _u32, _vp, _vp, _u64, _P(_u64), _P(_u64)]),
    "musc_overflow_probes": (_int, [_vp, _P(_vp), _P(_vp), _P(_u64)]),
    "musc_free_u32": (None, [_vp]),
    "musc_maxmatches_apply": (_int, [_vp, _int, _P(_u64), _P(_u64), _P(_u64)]),
    "musc_maxmatches_last_ms": (_int, [_vp, _P(_f32)]),
    "musc_maxmatches_last_detail": (_int, [_vp, _P(_u64), _P(_f32)]),
    "musc_gather": (_int, _GATHER),
    "musc_gather_rccl": (_int, _GATHER),
    "musc_rccl_probe": (_int, [_str, _u64]),
    "musc_sz_decode": (_int, [_vp, _vp, _u64, _vp, _u64, _int, _P(_u64)]),
    "musc_db_load_text": (_int, [_vp, _vp, _u64, _int, _int, _P(MuscDbTextInfo)]),
    "musc_targets_prep": (_int, [_vp, _vp, _u64, _int, _int, _int, _P(MuscTargetsPrepInfo)]),
    "musc_targets_prep_text": (_int, [_vp, _int, _u64, _u64, _vp, _int]),
    "musc_targets_prep_load": (_int, [_vp, _P(MuscDbTextInfo)]),
    "musc_targets_prep_free": (_int, [_vp]),
    "musc_sz_frame": (_int, _SZ_WRITE),
    "musc_sz_compress": (_int, _SZ_WRITE),
    "musc_targets_prep_sz": (_int, [_vp, _int, _int, _vp, _u64, _int, _P(_u64)]),
}
SYMBOLS = list(PROTOTYPES)

# `which` of musc_side_text (include/muscato_hip.h)
SIDE_NONMATCH, SIDE_GENESTATS, SIDE_READSTATS = 0, 1, 2

_lib = None


def load() -> ctypes.CDLL:
    """Load the HIP library; raise (never fall back) if it is missing or incomplete."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "muscato_amd: %s is missing -- build it with `python -m muscato_amd.build` "
            "(hipcc, gfx950).  There is no CPU fallback." % LIB_PATH)
    # torch ships a HIP runtime of its own; this library links the system one.  Both work in one
    # process when torch's opens the device first, and torch reports "no ROCm-capable device" when it
    # comes second.  A process that has torch loaded gets that order here, whatever the caller does
    # next (the library itself never imports torch).
    import sys
    torch = sys.modules.get("torch")
    if torch is not None:
        try:
            if torch.cuda.is_available():
                torch.cuda.init()
        except Exception:
            pass
    lib = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in PROTOTYPES.items():
        if not hasattr(lib, name):
            raise ImportError("muscato_amd: %s does not export %s" % (LIB_PATH, name))
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, list(argtypes)
    _lib = lib
    return lib
