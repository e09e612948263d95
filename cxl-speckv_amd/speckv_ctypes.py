"""ctypes binding of libcxlspeckv.so.

Same class, constructor, attributes and methods as the reference's binding
(reference host/python/speckv_ctypes.py:7-98) so callers written against it run
unchanged; the ``ext_*`` methods bind the additive entry points of
include/speckv_ext.h when the loaded library exports them.
"""
import ctypes
from ctypes import (c_char_p, c_float, c_int, c_int32, c_size_t, c_uint8, c_uint16, c_uint32, c_uint64, c_void_p)


def as_arr(v, t, n):
    """v as the C array argument `t v[n]`: a ctypes array as it is, a numpy array by its own data pointer (no copy), a sequence copied"""
    return v if isinstance(v, ctypes.Array) else (c_void_p(v.ctypes.data) if hasattr(v, "ctypes") else (t * n)(*v))


class SpeckvError(RuntimeError):
    """RuntimeError carrying the speckv_status_t code."""

    def __init__(self, what, status):
        super().__init__(f"{what} failed: {status}")
        self.status = status


class PageInfo(ctypes.Structure):
    """speckv_ext_page_info_t (include/speckv_ext.h)."""
    _fields_ = [("virt_page_id", c_uint64), ("phys_page_id", c_uint64), ("page_size", c_uint32),
                ("flags", c_uint32), ("pool_device", c_int32), ("scheme", c_uint32), ("rec_bytes", c_uint32),
                ("scale", c_float), ("pool_addr", c_uint64), ("cache_addr", c_uint64),
                ("access_count", c_uint32), ("aux_offset", c_uint32)]


class DmaDesc(ctypes.Structure):
    """speckv_dma_desc_t == reference SpeckvDmaDesc (host/include/speckv_driver.hpp:9-14)."""
    _fields_ = [("fpga_addr", c_uint64), ("gpu_addr", c_uint64), ("bytes", c_uint32), ("flags", c_uint32)]


SLOT_ELEM_FP16, SLOT_ELEM_BF16 = 0, 1


class SlotRows(ctypes.Structure):
    """speckv_ext_slot_rows_t (include/speckv_ext.h)."""
    _fields_ = [("elem", c_uint32), ("reserved", c_uint32), ("d_held_in", c_void_p), ("d_held_out", c_void_p),
                ("held_layer_stride_bytes", c_uint64)]


class Stats(ctypes.Structure):
    """speckv_ext_stats_t (include/speckv_ext.h)."""
    _fields_ = [(n, c_uint64) for n in (
        "l1_hits", "l1_misses", "l2_hits", "l2_misses", "l3_accesses", "migrations_l1_to_l3",
        "migrations_l3_to_l1", "total_prefetches", "successful_prefetches", "mispredictions",
        "total_compressions", "total_decompressions", "compressed_bytes", "original_bytes",
        "total_allocations", "total_deallocations", "current_allocated_bytes", "peak_allocated_bytes",
        "dma_submitted", "dma_completed", "pool_bytes_reserved", "cache_bytes_reserved")] + \
        [(n, c_uint32) for n in ("prefetch_depth", "compression_scheme", "quant_mode", "n_pool_devices")] + \
        [("pool_migrated_pages", c_uint64), ("prefetch_dropped", c_uint64), ("copy_engine_runs", c_uint64),
         ("copy_engine_bytes", c_uint64), ("pool_bytes_in_use", c_uint64), ("written_pages", c_uint64),
         ("sealed_allocations", c_uint64), ("compactions", c_uint64), ("flat_decoder_fetches", c_uint64),
         ("copied_pages", c_uint64)]


_u32p = ctypes.POINTER(c_uint32)
_u64p = ctypes.POINTER(c_uint64)

_EXT_SIGNATURES = {
    "speckv_ext_stream_is_capturing": [c_void_p, ctypes.POINTER(c_int)],
    "speckv_ext_set_quant_mode": [c_int],
    "speckv_ext_translate": [c_uint64, c_uint64, ctypes.POINTER(PageInfo)],
    "speckv_ext_fetch_desc": [c_uint64, c_uint64, ctypes.POINTER(DmaDesc)],
    "speckv_ext_set_layout": [c_uint64, c_uint32, c_uint32, c_uint32, c_uint32, c_uint32],
    "speckv_ext_write": [c_uint64, c_uint64, c_void_p, c_size_t, c_int],
    "speckv_ext_read": [c_uint64, c_uint64, c_void_p, c_size_t, c_int],
    "speckv_ext_write_strided": [c_uint64, c_uint64, c_uint64, c_uint64, c_void_p, c_void_p],
    "speckv_ext_write_strided_batch": [c_void_p, c_void_p, c_void_p, c_uint32, c_uint64, c_uint64, c_void_p],
    "speckv_ext_write_async": [c_uint64, c_uint64, c_void_p, c_size_t, c_void_p],
    "speckv_ext_write_runs": [c_uint64, c_void_p, c_void_p, c_uint32, c_uint64, c_void_p],
    "speckv_ext_write_pairs": [c_void_p, c_void_p, c_void_p, c_uint32, c_uint64, c_uint32, c_uint64, c_void_p],
    "speckv_ext_read_pairs": [c_void_p, c_void_p, c_void_p, c_uint32, c_uint64, c_uint32, c_uint64, c_void_p],
    "speckv_ext_read_slots": [c_void_p, c_void_p, c_void_p, c_void_p, c_uint32, c_void_p, c_uint64, c_void_p, c_uint32, c_uint32, c_uint64,
                              c_uint64, c_void_p],
    "speckv_ext_write_slots": [c_void_p, c_void_p, c_void_p, c_void_p, c_uint32, c_void_p, c_uint64, c_void_p, c_uint32, c_uint32, c_uint64,
                               c_uint64, c_void_p],
    "speckv_ext_read_slots_ex": [c_void_p, c_void_p, c_void_p, c_void_p, c_uint32, c_void_p, c_uint64, c_void_p, c_uint32, c_uint32, c_uint64,
                                 c_uint64, c_void_p, c_void_p],
    "speckv_ext_write_slots_ex": [c_void_p, c_void_p, c_void_p, c_void_p, c_uint32, c_void_p, c_uint64, c_void_p, c_uint32, c_uint32, c_uint64,
                                  c_uint64, c_void_p, c_void_p],
    "speckv_ext_read_slots_kmul": [c_void_p, c_void_p, c_void_p, c_void_p, c_uint32, c_void_p, c_uint64, c_void_p, c_uint32, c_uint32, c_uint64,
                                   c_uint64, c_void_p, c_void_p, c_uint64, c_void_p],
    "speckv_ext_write_slots_kmul": [c_void_p, c_void_p, c_void_p, c_void_p, c_uint32, c_void_p, c_uint64, c_void_p, c_uint32, c_uint32, c_uint64,
                                    c_uint64, c_void_p, c_void_p, c_uint64, c_void_p],
    "speckv_ext_read_slots_kv": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_uint32, c_void_p, c_uint64, c_void_p, c_uint32, c_uint32,
                                 c_uint64, c_uint64, c_void_p, c_void_p],
    "speckv_ext_write_slots_kv": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_uint32, c_void_p, c_uint64, c_void_p, c_uint32, c_uint32,
                                  c_uint64, c_uint64, c_void_p, c_void_p],
    "speckv_ext_copy_runs": [c_void_p, c_void_p, c_void_p, c_uint32, c_void_p, c_uint32, c_void_p],
    "speckv_ext_read_pairs_kv": [c_void_p, c_void_p, c_void_p, c_void_p, c_uint32, c_uint64, c_uint32, c_uint64, c_void_p],
    "speckv_ext_copy_runs_kv": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_uint32, c_void_p, c_uint32, c_void_p],
    "speckv_ext_attend_chunk": [c_uint32, c_void_p, c_uint32, c_void_p, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_uint64,
                                c_uint64, c_void_p, c_void_p, c_void_p, c_uint64, ctypes.c_float, c_void_p, c_void_p, c_void_p],
    "speckv_ext_attend_chunk_masked": [c_uint32, c_void_p, c_uint32, c_void_p, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_uint64,
                                       c_uint64, c_void_p, c_void_p, c_void_p, c_uint64, c_void_p, c_uint32, ctypes.c_float, c_void_p, c_void_p,
                                       c_void_p],
    "speckv_ext_attend_chunk_split": [c_uint32, c_void_p, c_uint32, c_void_p, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_uint64,
                                      c_uint64, c_void_p, c_void_p, c_void_p, c_uint64, c_void_p, c_uint32, c_uint32, ctypes.c_float, c_void_p,
                                      c_void_p, c_void_p],
    "speckv_ext_chunk_split_plan": [c_uint32, c_void_p, c_void_p, c_uint32, c_uint32, c_uint32, c_void_p, c_void_p],
    "speckv_ext_codec_launch_shape": [c_uint64, c_uint32, c_void_p, c_void_p, c_void_p],
    "speckv_ext_fetch_sweep_next": [c_uint64, c_uint64, c_uint32, c_uint32, c_uint64, c_uint64, c_int, c_int, c_void_p, c_void_p, c_void_p],
    "speckv_ext_attend_chunk_window": [c_uint32, c_void_p, c_uint32, c_void_p, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_uint64,
                                       c_uint64, c_void_p, c_void_p, c_void_p, c_uint64, c_uint32, c_uint32, ctypes.c_float, c_void_p, c_void_p,
                                       c_void_p],
    "speckv_ext_chunk_window_walk": [c_uint32, c_void_p, c_void_p, c_void_p, c_uint32, c_uint32, c_void_p, c_void_p],
    "speckv_ext_attend_chunk_tree_window": [c_uint32, c_void_p, c_uint32, c_void_p, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p,
                                            c_uint64, c_uint64, c_void_p, c_void_p, c_void_p, c_uint64, c_void_p, c_uint32, c_void_p, c_uint32,
                                            c_uint32, ctypes.c_float, c_void_p, c_void_p, c_void_p],
    "speckv_ext_attend_chunk_kv": [c_uint32, c_void_p, c_void_p, c_uint32, c_void_p, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_uint64, c_uint64, c_void_p, c_void_p, c_void_p, c_uint64, c_void_p, c_uint32, c_void_p, c_uint32,
                                   c_uint32, ctypes.c_float, c_void_p, c_void_p, c_void_p],
    "speckv_ext_attend_prefix_fold": [c_uint32, c_void_p, c_void_p, c_uint32, c_void_p, c_uint32, c_uint32, c_void_p, c_void_p, c_uint32,
                                      ctypes.c_float, c_void_p, c_void_p, c_void_p],
    "speckv_ext_attend_prefix_fold_window": [c_uint32, c_void_p, c_void_p, c_uint32, c_void_p, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p,
                                             c_void_p, c_uint32, c_uint32, ctypes.c_float, c_void_p, c_void_p, c_void_p],
    "speckv_ext_attend_prefix_fold_kv": [c_uint32, c_void_p, c_void_p, c_void_p, c_uint32, c_void_p, c_uint32, c_uint32, c_void_p, c_void_p,
                                         c_void_p, c_void_p, c_uint32, c_uint32, ctypes.c_float, c_void_p, c_void_p, c_void_p],
    "speckv_ext_prefix_window_walk": [c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_uint32, c_void_p, c_void_p],
    "speckv_ext_fetch_range": [c_uint64, c_uint64, c_uint64, c_void_p, c_int, c_void_p],
    "speckv_ext_fetch_range_engine": [c_uint64, c_uint64, c_uint64, c_void_p, c_int, c_void_p, c_int],
    "speckv_ext_bind_request": [c_uint32, c_uint64, c_uint32],
    "speckv_ext_fetch_list": [c_uint64, c_void_p, c_uint32, c_void_p, c_int, c_void_p],
    "speckv_ext_access_batch": [c_uint64, _u64p, c_uint32, ctypes.POINTER(c_void_p)],
    "speckv_ext_prefetch_batch": [c_uint32, _u32p, ctypes.POINTER(c_uint16), _u32p, _u32p],
    "speckv_ext_prefetch_flush": [_u32p],
    "speckv_ext_prefetch_lookup": [c_uint64, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_uint32, c_void_p, c_void_p],
    "speckv_ext_prefetch_legacy_addrs": [c_uint32, c_uint32, _u64p, _u32p],
    "speckv_ext_verify": [c_uint32, c_int32, ctypes.POINTER(c_int32), c_uint32, _u32p, _u32p],
    "speckv_ext_verify_batch": [c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "speckv_ext_get_prefetch_depth": [_u32p],
    "speckv_ext_poll_complete": [_u32p],
    "speckv_ext_sync": [],
    "speckv_ext_codec_compress": [c_void_p, c_uint64, c_void_p, c_uint64, c_void_p, c_void_p, c_int, c_int, c_void_p],
    "speckv_ext_codec_decompress": [c_void_p, c_uint64, c_void_p, c_void_p, c_uint64, c_void_p, c_int, c_int, c_int, c_void_p],
    "speckv_ext_codec_compress_tensor": [c_void_p, c_uint64, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_void_p],
    "speckv_ext_codec_decompress_tensor": [c_void_p, c_uint64, ctypes.c_float, c_void_p, c_uint64, c_int, c_void_p, c_void_p, c_size_t, c_int, c_void_p],
    "speckv_ext_qk_scores_fp8": [c_uint64, c_uint32, c_void_p, c_uint32, c_uint32, c_uint32, c_void_p, c_void_p],
    "speckv_ext_qk_scores_fp8_layers": [c_uint64, c_uint32, c_uint32, c_void_p, c_uint32, c_uint32, c_uint32, c_void_p, c_void_p],
    "speckv_ext_attend_fp8": [c_uint64, c_uint32, c_uint32, c_void_p, c_uint32, c_uint32, c_uint32, ctypes.c_float, c_void_p, c_void_p, c_void_p],
    "speckv_ext_attend_fp8_batch": [c_uint32, ctypes.POINTER(c_uint64), c_uint32, c_void_p, c_uint32, _u32p, ctypes.c_float, c_void_p, c_void_p, c_void_p],
    "speckv_ext_attend_kv_batch": [c_uint32, c_void_p, c_void_p, c_uint32, c_void_p, c_uint32, c_void_p, ctypes.c_float, c_void_p, c_void_p, c_void_p],
    "speckv_ext_attend_kv_batch_window": [c_uint32, c_void_p, c_void_p, c_uint32, c_void_p, c_uint32, c_void_p, c_void_p, c_uint32, ctypes.c_float, c_void_p,
                                          c_void_p, c_void_p],
    "speckv_ext_attend_int4_batch": [c_uint32, ctypes.POINTER(c_uint64), c_uint32, c_void_p, c_uint32, _u32p, ctypes.c_float, c_void_p, c_void_p, c_void_p],
    "speckv_ext_attend_batch_plan": [c_uint32, ctypes.POINTER(c_uint64), _u32p, c_uint32, c_void_p, c_size_t, c_void_p],
    "speckv_ext_attend_batch_plan_window": [c_uint32, ctypes.POINTER(c_uint64), _u32p, _u32p, c_uint32, c_uint32, c_void_p, c_size_t, c_void_p],
    "speckv_ext_attend_batch_window": [c_int, c_uint32, ctypes.POINTER(c_uint64), c_uint32, c_void_p, c_uint32, _u32p, _u32p, c_uint32, ctypes.c_float,
                                       c_void_p, c_void_p, c_void_p],
    "speckv_ext_decode_window_range": [c_uint32, c_uint32, _u32p, _u32p, _u32p],
    "speckv_ext_attend_fp8_planned": [c_void_p, c_uint32, c_uint32, c_void_p, c_uint32, c_uint32, ctypes.c_float, c_void_p, c_void_p, c_void_p],
    "speckv_ext_attend_int4_planned": [c_void_p, c_uint32, c_uint32, c_void_p, c_uint32, c_uint32, ctypes.c_float, c_void_p, c_void_p, c_void_p],
    "speckv_ext_attend_fold_tail": [c_uint32, c_void_p, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_uint64, ctypes.c_float, c_void_p, c_void_p, c_void_p],
    "speckv_ext_attend_kv_spec": [c_uint32, c_void_p, c_void_p, c_uint32, c_void_p, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_uint64, c_uint64,
                                  c_void_p, c_uint32, ctypes.c_float, c_void_p, c_void_p, c_void_p],
    "speckv_ext_attend_kv_spec_window": [c_uint32, c_void_p, c_void_p, c_uint32, c_void_p, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_uint32,
                                         c_void_p, c_void_p, c_uint64, c_uint64, c_void_p, c_uint32, ctypes.c_float, c_void_p, c_void_p, c_void_p],
    "speckv_ext_spec_window_range": [c_uint32, c_uint32, _u32p, ctypes.POINTER(ctypes.c_int32), _u32p],
    "speckv_ext_attend_fold_held": [c_uint32, c_void_p, c_uint32, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_uint64, c_uint64, c_void_p, c_void_p,
                                    ctypes.c_float, c_void_p, c_void_p, c_void_p],
    "speckv_ext_attend_fold_masked": [c_uint32, c_void_p, c_uint32, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_uint64, c_uint64, c_void_p, c_uint32,
                                      ctypes.c_float, c_void_p, c_void_p, c_void_p],
    "speckv_ext_attend_int4": [c_uint64, c_uint32, c_uint32, c_void_p, c_uint32, c_uint32, c_uint32, ctypes.c_float, c_void_p, c_void_p, c_void_p],
    "speckv_ext_attend_mx4": [c_uint64, c_uint32, c_uint32, c_void_p, c_uint32, c_uint32, c_uint32, ctypes.c_float, c_void_p, c_void_p, c_void_p],
    "speckv_ext_attend_mx4_batch": [c_uint32, ctypes.POINTER(c_uint64), c_uint32, c_void_p, c_uint32, _u32p, ctypes.c_float, c_void_p, c_void_p, c_void_p],
    "speckv_ext_attend_mx4_planned": [c_void_p, c_uint32, c_uint32, c_void_p, c_uint32, c_uint32, ctypes.c_float, c_void_p, c_void_p, c_void_p],
    "speckv_ext_attend_planned_layers": [c_int, c_void_p, c_uint32, c_uint32, c_uint32, c_void_p, c_uint32, c_uint32, ctypes.c_float, c_void_p, c_void_p, c_uint32,
                                         c_void_p, c_void_p, c_void_p, c_void_p, c_uint64, c_void_p],
    "speckv_ext_attend_planned_tail": [c_int, c_void_p, c_uint32, c_uint32, c_void_p, c_uint32, c_uint32, ctypes.c_float, c_void_p, c_void_p, c_uint32,
                                       c_void_p, c_void_p, c_void_p, c_void_p, c_uint64, c_void_p],
    "speckv_ext_promote_to_l1": [c_uint64, c_uint64],
    "speckv_ext_demote_to_l3": [c_uint64, c_uint64],
    "speckv_ext_migrate": [c_uint64, c_uint64, c_uint64, c_uint32],
    "speckv_ext_compact": [c_uint64, _u64p, _u64p],
    "speckv_ext_predictor_load": [c_void_p, c_void_p, c_uint32, c_int],
    "speckv_ext_predict_batch": [c_uint32, c_void_p, c_uint32, c_void_p, c_void_p, c_void_p],
    "speckv_ext_predictor_load_lstm": [c_void_p, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int],
    "speckv_ext_stats": [ctypes.POINTER(Stats)],
    "speckv_ext_stats_sized": [c_void_p, c_size_t, ctypes.POINTER(c_size_t)],
}


EXT_ABI_VERSION = 6        # SPECKV_EXT_ABI_VERSION of include/speckv_ext.h
CHUNK_SPLITS_MAX = 64      # SPECKV_CHUNK_SPLITS_MAX: the most pieces speckv_ext_attend_chunk_split cuts a sequence's stored positions into
HELD_MAX = 17              # SPECKV_HELD_MAX: positions speckv_ext_attend_fold_held takes per sequence (one left over + 16 new ones)


def bind_ext(lib):
    """Attach argtypes/restype of every speckv_ext_* symbol the library exports."""
    found = []
    for name, args in _EXT_SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            continue
        fn.argtypes, fn.restype = args, c_int
        found.append(name)
    for name, res, args in (("speckv_ext_layer_compression_ratio", ctypes.c_double, [c_uint32]), ("speckv_ext_backend", c_char_p, []),
                            ("speckv_ext_attend_plan_bytes", c_size_t, [c_uint32]),
                            ("speckv_ext_attend_plan_window_bytes", c_size_t, [c_uint32]),
                            ("speckv_ext_codec_tensor_workspace_bytes", c_size_t, [c_uint64]),
                            ("speckv_ext_codec_tensor_decode_workspace_bytes", c_size_t, [c_uint64])):
        try:
            fn = getattr(lib, name)
        except AttributeError:
            continue
        fn.restype = res
        fn.argtypes = args
        found.append(name)
    # the structs of include/speckv_ext.h are mirrored by hand in this file: a library built from another header revision
    # would write past (or short of) them
    try:
        ver = lib.speckv_ext_abi_version
    except AttributeError:
        ver = None
    if ver is not None:
        ver.restype, ver.argtypes = c_uint32, []
        if ver() != EXT_ABI_VERSION:
            raise RuntimeError(f"libcxlspeckv.so speaks speckv_ext ABI {ver()}, this binding {EXT_ABI_VERSION}: rebuild the library")
        found.append("speckv_ext_abi_version")
    return found


class SpeckvLib:
    def __init__(self, path: str, dev_path: str = "/dev/speckv0"):
        from .build import load_library
        self.lib = load_library(path)

        # typedef uint64_t speckv_handle_t;
        self.handle_t = c_uint64

        self.lib.speckv_init.argtypes = [c_char_p]
        self.lib.speckv_init.restype = c_int
        self.lib.speckv_finalize.argtypes = []
        self.lib.speckv_finalize.restype = None

        class AllocHint(ctypes.Structure):
            _fields_ = [("preferred_node", c_uint32), ("reserved", c_uint32)]
        self.AllocHint = AllocHint

        self.lib.speckv_alloc.argtypes = [c_size_t, ctypes.POINTER(AllocHint), ctypes.POINTER(self.handle_t)]
        self.lib.speckv_alloc.restype = c_int
        self.lib.speckv_free.argtypes = [self.handle_t]
        self.lib.speckv_free.restype = c_int
        self.lib.speckv_access.argtypes = [self.handle_t, c_uint64, c_size_t, ctypes.POINTER(c_void_p)]
        self.lib.speckv_access.restype = c_int
        self.lib.speckv_prefetch.argtypes = [c_uint32, c_uint16, c_uint32, c_uint32, ctypes.POINTER(c_int32), c_uint32]
        self.lib.speckv_prefetch.restype = c_int
        self.lib.speckv_set_prefetch_depth.argtypes = [c_uint32]
        self.lib.speckv_set_prefetch_depth.restype = c_int
        self.lib.speckv_set_compression_scheme.argtypes = [c_int]
        self.lib.speckv_set_compression_scheme.restype = c_int
        self.ext = bind_ext(self.lib)

        ret = self.lib.speckv_init(dev_path.encode("ascii"))
        if ret != 0:
            raise SpeckvError("speckv_init", ret)

    # ---- the reference surface (speckv_ctypes.py:64-98) -------------
    def alloc(self, bytes_needed, preferred_node=0):
        hint = self.AllocHint(preferred_node, 0)
        handle = self.handle_t()
        ret = self.lib.speckv_alloc(bytes_needed, ctypes.byref(hint), ctypes.byref(handle))
        if ret != 0:
            raise SpeckvError("speckv_alloc", ret)
        return handle.value

    def free(self, handle):
        ret = self.lib.speckv_free(handle)
        if ret != 0:
            raise SpeckvError("speckv_free", ret)

    def access(self, handle, offset, length):
        gpu_ptr = c_void_p()
        ret = self.lib.speckv_access(handle, offset, length, ctypes.byref(gpu_ptr))
        if ret != 0:
            raise SpeckvError("speckv_access", ret)
        return gpu_ptr.value

    def prefetch(self, req_id, layer, cur_pos, depth_k, tokens):
        arr = (c_int32 * len(tokens))(*tokens)
        ret = self.lib.speckv_prefetch(req_id, layer, cur_pos, depth_k, arr, len(tokens))
        if ret != 0:
            raise SpeckvError("speckv_prefetch", ret)

    def set_prefetch_depth(self, depth_k):
        ret = self.lib.speckv_set_prefetch_depth(depth_k)
        if ret != 0:
            raise SpeckvError("speckv_set_prefetch_depth", ret)

    def set_compression_scheme(self, scheme):
        ret = self.lib.speckv_set_compression_scheme(scheme)
        if ret != 0:
            raise SpeckvError("speckv_set_compression_scheme", ret)

    # ---- additions ---------------------------------------------------
    def finalize(self):
        self.lib.speckv_finalize()

    def _ext(self, name, *args):
        ret = getattr(self.lib, name)(*args)
        if ret != 0:
            raise SpeckvError(name, ret)

    def translate(self, handle, offset):
        info = PageInfo()
        self._ext("speckv_ext_translate", handle, offset, ctypes.byref(info))
        return info

    def fetch_desc(self, handle, offset):
        d = DmaDesc()
        self._ext("speckv_ext_fetch_desc", handle, offset, ctypes.byref(d))
        return d

    def set_layout(self, handle, num_tokens, num_layers, num_heads, head_dim, bytes_per_element):
        self._ext("speckv_ext_set_layout", handle, num_tokens, num_layers, num_heads, head_dim, bytes_per_element)

    def set_quant_mode(self, mode):
        self._ext("speckv_ext_set_quant_mode", mode)

    def write(self, handle, offset, src_ptr, nbytes, on_device):
        self._ext("speckv_ext_write", handle, offset, c_void_p(src_ptr), nbytes, int(on_device))

    def write_strided(self, handle, first_page, page_step, n_pages, d_src, stream=None):
        self._ext("speckv_ext_write_strided", handle, first_page, page_step, n_pages, c_void_p(d_src), c_void_p(stream or 0))

    def write_strided_batch(self, handles, first_pages, d_srcs, page_step, n_pages_each, stream):
        """One launch for a batch of allocations: handles[i] gets pages first_pages[i] + j*page_step from d_srcs[i] + j*4096."""
        n = len(handles)
        hs, fs, ps = as_arr(handles, c_uint64, n), as_arr(first_pages, c_uint64, n), as_arr(d_srcs, c_void_p, n)     # numpy uint64 arrays pass as they are
        self._ext("speckv_ext_write_strided_batch", hs, fs, ps, n, page_step, n_pages_each, c_void_p(stream))

    def write_async(self, handle, offset, d_src, nbytes, stream):
        """A contiguous page range from a device buffer, asynchronously on `stream` (no device-wide wait)."""
        self._ext("speckv_ext_write_async", handle, offset, c_void_p(d_src), nbytes, c_void_p(stream or 0))

    def write_runs(self, handle, first_pages, d_srcs, n_pages_each, stream):
        """Several page runs of one allocation in ONE launch: run r = n_pages_each pages from first_pages[r], read from d_srcs[r]."""
        n = len(first_pages)
        self._ext("speckv_ext_write_runs", handle, (c_uint64 * n)(*first_pages), (c_void_p * n)(*d_srcs), n, n_pages_each,
                  c_void_p(stream))

    def write_pairs(self, handles, first_pages, rows, page_step, n_layers, layer_stride, stream):
        """The commit of a multi-position step in ONE launch: pair i = pages first_pages[i] + j*page_step (j < 2*n_layers) of
        handles[i], each page read from two rows -- rows[i] = (K even, K odd, V even, V odd) device addresses, layer_stride bytes
        apart per layer.  handles / first_pages: uint64 arrays of n; rows: a uint64 array [n][4] (numpy arrays pass as they are)."""
        n = len(handles)
        if not hasattr(rows, "ctypes") and not isinstance(rows, ctypes.Array):
            rows = [p for r in rows for p in r]
        hs, fs, rs = as_arr(handles, c_uint64, n), as_arr(first_pages, c_uint64, n), as_arr(rows, c_uint64, 4 * n)
        self._ext("speckv_ext_write_pairs", hs, fs, rs, n, page_step, n_layers, layer_stride, c_void_p(stream))

    def read_pairs(self, handles, first_pages, rows, page_step, n_layers, layer_stride, stream):
        """write_pairs read backwards, in ONE launch (the rollback of committed positions): pair i = pages first_pages[i] + j*page_step
        (j < 2*n_layers) of handles[i], each page decoded into two rows -- rows[i] = (K even, K odd, V even, V odd) device addresses,
        layer_stride bytes apart per layer; an address of 0 = that row is not wanted and is not written.  Arguments as write_pairs."""
        n = len(handles)
        if not hasattr(rows, "ctypes") and not isinstance(rows, ctypes.Array):
            rows = [p for r in rows for p in r]
        hs, fs, rs = as_arr(handles, c_uint64, n), as_arr(first_pages, c_uint64, n), as_arr(rows, c_uint64, 4 * n)
        self._ext("speckv_ext_read_pairs", hs, fs, rs, n, page_step, n_layers, layer_stride, c_void_p(stream))

    def _slots(self, entry, handles, first_tokens, n_tokens, slot_begins, d_slots, n_slots, caches, layer_begin, kind_stride, page_step, stream):
        n, nl = len(handles), len(caches)
        hs, fs, ns, bs = (as_arr(x, c_uint64, n) for x in (handles, first_tokens, n_tokens, slot_begins))
        self._ext(entry, hs, fs, ns, bs, n, c_void_p(d_slots), n_slots, as_arr(caches, c_uint64, nl), layer_begin, nl, kind_stride, page_step,
                  c_void_p(stream))

    def read_slots(self, handles, first_tokens, n_tokens, slot_begins, d_slots, n_slots, caches, layer_begin, kind_stride, page_step, stream):
        """Pool -> paged cache in ONE launch (speckv_ext_read_slots): span i = positions [first_tokens[i], + n_tokens[i]) of handles[i],
        row t of it decoded into slot d_slots[slot_begins[i] + t] (d_slots: the address of an int64 device array) of every layer
        layer_begin + l -- caches[l] = that layer's base address, K plane at 0, V plane at kind_stride bytes, 2048 bytes per slot; a slot
        < 0 or >= n_slots is skipped.  handles .. slot_begins, caches: numpy uint64 arrays, ctypes arrays or sequences."""
        self._slots("speckv_ext_read_slots", handles, first_tokens, n_tokens, slot_begins, d_slots, n_slots, caches, layer_begin, kind_stride,
                    page_step, stream)

    def write_slots(self, handles, first_tokens, n_tokens, slot_begins, d_slots, n_slots, caches, layer_begin, kind_stride, page_step, stream):
        """Paged cache -> pool in ONE launch (speckv_ext_write_slots): read_slots backwards, whole pairs only (first_tokens and n_tokens
        even); a slot < 0 or >= n_slots is stored as a row of zeros.  Arguments as read_slots."""
        self._slots("speckv_ext_write_slots", handles, first_tokens, n_tokens, slot_begins, d_slots, n_slots, caches, layer_begin, kind_stride,
                    page_step, stream)

    def _slots_ex(self, entry, handles, first_tokens, n_tokens, slot_begins, d_slots, n_slots, caches, layer_begin, kind_stride, page_step,
                  stream, elem, held_in, held_out, held_stride, reserved=0, k_mul=(), v_handles=None):
        n, nl = len(handles), len(caches)
        hs, fs, ns, bs = (as_arr(x, c_uint64, n) for x in (handles, first_tokens, n_tokens, slot_begins))
        if v_handles is not None:                                                      # the _kv entries: two handle arrays in front
            hs = (hs, as_arr(v_handles, c_uint64, n))
        hin = None if held_in is None else as_arr(held_in, c_uint64, 2 * n)            # (kept alive across the call)
        hout = None if held_out is None else as_arr(held_out, c_uint64, 2 * n)
        at = lambda a: None if a is None else (a.value if isinstance(a, c_void_p) else ctypes.addressof(a))
        rows = SlotRows(elem, reserved, at(hin), at(hout), held_stride)
        self._ext(entry, *(hs if v_handles is not None else (hs,)), fs, ns, bs, n, c_void_p(d_slots), n_slots, as_arr(caches, c_uint64, nl),
                  layer_begin, nl, kind_stride, page_step,
                  ctypes.cast(ctypes.pointer(rows), c_void_p), *k_mul, c_void_p(stream))     # k_mul: the _kmul entries' two arguments

    def read_slots_ex(self, handles, first_tokens, n_tokens, slot_begins, d_slots, n_slots, caches, layer_begin, kind_stride, page_step,
                      stream, elem=SLOT_ELEM_FP16, held_in=None, held_stride=0, held_out=None, reserved=0):
        """read_slots for caches whose rows hold `elem` (SLOT_ELEM_FP16 / SLOT_ELEM_BF16: the decoded fp16 value rounded once to bf16)
        and for spans whose last, even position lives in a held fp16 row (speckv_ext_read_slots_ex): held_in = 2 * len(handles)
        device addresses (K, V per span; 0 = none), the row of layer layer_begin + l at + l * held_stride bytes.  held_out and
        reserved exist to be refused."""
        self._slots_ex("speckv_ext_read_slots_ex", handles, first_tokens, n_tokens, slot_begins, d_slots, n_slots, caches, layer_begin,
                       kind_stride, page_step, stream, elem, held_in, held_out, held_stride, reserved)

    def write_slots_ex(self, handles, first_tokens, n_tokens, slot_begins, d_slots, n_slots, caches, layer_begin, kind_stride, page_step,
                       stream, elem=SLOT_ELEM_FP16, held_in=None, held_stride=0, held_out=None, reserved=0):
        """write_slots for caches whose rows hold `elem` (a bf16 element is rounded once to fp16, and that is encoded) and for odd
        edges (speckv_ext_write_slots_ex): held_in[2i + kind] = the fp16 row of position first_tokens[i] - 1 (first odd),
        held_out[2i + kind] = where the odd last position goes as fp16 instead of being encoded (first + n odd).  Arguments as
        read_slots_ex."""
        self._slots_ex("speckv_ext_write_slots_ex", handles, first_tokens, n_tokens, slot_begins, d_slots, n_slots, caches, layer_begin,
                       kind_stride, page_step, stream, elem, held_in, held_out, held_stride, reserved)

    def read_slots_kmul(self, handles, first_tokens, n_tokens, slot_begins, d_slots, n_slots, caches, layer_begin, kind_stride, page_step,
                        stream, elem=SLOT_ELEM_FP16, held_in=None, held_stride=0, held_out=None, reserved=0, k_mul=0, k_mul_stride=0):
        """read_slots_ex with a per-channel factor on K (speckv_ext_read_slots_kmul): k_mul = the device address of fp16 [heads][128]
        factor rows, the row of layer layer_begin + l at + l * k_mul_stride bytes; every decoded K element (the fp16 bits fetch_range
        writes) and every K element of a held-in row is multiplied by its channel's factor, the exact product rounded once to `elem`.
        V is not touched.  k_mul = 0 (None): the read_slots_ex call."""
        self._slots_ex("speckv_ext_read_slots_kmul", handles, first_tokens, n_tokens, slot_begins, d_slots, n_slots, caches, layer_begin,
                       kind_stride, page_step, stream, elem, held_in, held_out, held_stride, reserved, (c_void_p(k_mul or None), k_mul_stride))

    def write_slots_kmul(self, handles, first_tokens, n_tokens, slot_begins, d_slots, n_slots, caches, layer_begin, kind_stride, page_step,
                         stream, elem=SLOT_ELEM_FP16, held_in=None, held_stride=0, held_out=None, reserved=0, k_mul=0, k_mul_stride=0):
        """write_slots_ex with a per-channel factor on K (speckv_ext_write_slots_kmul): what is encoded, and what goes into a held-out
        row, is fp16(cache element * factor) -- the exact product of the fp16 or bf16 element rounded once; a held-in row is pool-side
        already and is not multiplied.  Arguments as read_slots_kmul."""
        self._slots_ex("speckv_ext_write_slots_kmul", handles, first_tokens, n_tokens, slot_begins, d_slots, n_slots, caches, layer_begin,
                       kind_stride, page_step, stream, elem, held_in, held_out, held_stride, reserved, (c_void_p(k_mul or None), k_mul_stride))

    def read_slots_kv(self, k_handles, v_handles, first_tokens, n_tokens, slot_begins, d_slots, n_slots, caches, layer_begin, kind_stride,
                      page_step, stream, elem=SLOT_ELEM_FP16, held_in=None, held_stride=0, held_out=None, reserved=0):
        """read_slots_ex for the split pool (speckv_ext_read_slots_kv): span i = positions of the FP8_E4M3 allocation k_handles[i],
        whose rows go to the K plane of the caches, and of the MXFP4 allocation v_handles[i], whose rows go to the V plane; the page
        of (layer, position) is layer * page_step + position // 2 in either.  ONE launch.  Everything else as read_slots_ex."""
        self._slots_ex("speckv_ext_read_slots_kv", k_handles, first_tokens, n_tokens, slot_begins, d_slots, n_slots, caches, layer_begin,
                       kind_stride, page_step, stream, elem, held_in, held_out, held_stride, reserved, v_handles=v_handles)

    def write_slots_kv(self, k_handles, v_handles, first_tokens, n_tokens, slot_begins, d_slots, n_slots, caches, layer_begin, kind_stride,
                       page_step, stream, elem=SLOT_ELEM_FP16, held_in=None, held_stride=0, held_out=None, reserved=0):
        """write_slots_ex for the split pool (speckv_ext_write_slots_kv): the K plane's rows are encoded as FP8_E4M3 into
        k_handles[i], the V plane's as MXFP4 into v_handles[i], in ONE launch.  Arguments as read_slots_kv."""
        self._slots_ex("speckv_ext_write_slots_kv", k_handles, first_tokens, n_tokens, slot_begins, d_slots, n_slots, caches, layer_begin,
                       kind_stride, page_step, stream, elem, held_in, held_out, held_stride, reserved, v_handles=v_handles)

    def copy_runs(self, src, dst, n_pages, run_firsts, stream):
        """The stored records of pages [run_firsts[r], run_firsts[r] + n_pages[i]), every run r, copied from allocation src[i] to the same
        pages of allocation dst[i] in ONE launch, nothing decoded (a request forked from another one's positions).  src, dst, n_pages:
        one entry per pair; numpy uint64 arrays, ctypes arrays or sequences.  One source may feed several destinations; a destination
        appears once and is no source of the same call."""
        n, m = len(src), len(run_firsts)
        ss, ds, ns, fs = as_arr(src, c_uint64, n), as_arr(dst, c_uint64, n), as_arr(n_pages, c_uint64, n), as_arr(run_firsts, c_uint64, m)
        self._ext("speckv_ext_copy_runs", ss, ds, ns, n, fs, m, c_void_p(stream))

    def read_pairs_kv(self, k_handles, v_handles, first_pages, rows, page_step, n_layers, layer_stride, stream):
        """read_pairs for the split pool in ONE launch (speckv_ext_read_pairs_kv): pair i = page first_pages[i] + l*page_step of the
        FP8_E4M3 allocation k_handles[i] and of the MXFP4 allocation v_handles[i] for every REAL layer l < n_layers, decoded into
        rows[i] = (K even, K odd, V even, V odd) device addresses + l*layer_stride; an address of 0 = that row is not wanted.
        Arguments as read_pairs behind the second handle array."""
        n = len(k_handles)
        if not hasattr(rows, "ctypes") and not isinstance(rows, ctypes.Array):
            rows = [p for r in rows for p in r]
        ks, vs, fs, rs = as_arr(k_handles, c_uint64, n), as_arr(v_handles, c_uint64, n), as_arr(first_pages, c_uint64, n), as_arr(rows, c_uint64, 4 * n)
        self._ext("speckv_ext_read_pairs_kv", ks, vs, fs, rs, n, page_step, n_layers, layer_stride, c_void_p(stream))

    def copy_runs_kv(self, k_src, v_src, k_dst, v_dst, n_pages, run_firsts, stream):
        """copy_runs for the split pool in ONE launch (speckv_ext_copy_runs_kv): the stored records of pages [run_firsts[r], run_firsts[r]
        + n_pages[i]), every run r, copied from k_src[i] to k_dst[i] (FP8_E4M3) and from v_src[i] to v_dst[i] (MXFP4).  A destination
        appears once across k_dst and v_dst together and is no source of the same call.  Arguments as copy_runs behind the handle
        arrays."""
        n, m = len(k_src), len(run_firsts)
        hs = [as_arr(x, c_uint64, n) for x in (k_src, v_src, k_dst, v_dst)]
        ns, fs = as_arr(n_pages, c_uint64, n), as_arr(run_firsts, c_uint64, m)
        self._ext("speckv_ext_copy_runs_kv", *hs, ns, n, fs, m, c_void_p(stream))

    def _chunk(self, entry, handles, layer, d_q, C, rows_per_pos, pos_end, n_q, d_k_new, d_v_new, seq_stride, pos_stride, tail_idx, d_k_tail,
               d_v_tail, tail_stride, form, sm_scale, d_out, d_lse, stream):
        """One call of a chunk-attention entry: the 16 arguments all five share (n_seq from handles, then up to tail_stride), `form` -- the
        entry's own arguments, already as C values -- in their place in front of sm_scale, and the four that close every entry."""
        n = len(handles)
        self._ext(entry, n, as_arr(handles, c_uint64, n), layer, c_void_p(d_q), C, rows_per_pos, as_arr(pos_end, c_uint32, n),
                  as_arr(n_q, c_uint32, n), c_void_p(d_k_new), c_void_p(d_v_new), seq_stride, pos_stride,
                  None if tail_idx is None else as_arr(tail_idx, c_int32, n), c_void_p(d_k_tail or None), c_void_p(d_v_tail or None), tail_stride,
                  *form, sm_scale, c_void_p(d_out), c_void_p(d_lse or None), c_void_p(stream))

    def attend_chunk(self, handles, layer, d_q, C, rows_per_pos, pos_end, n_q, d_k_new, d_v_new, seq_stride, pos_stride, tail_idx, d_k_tail,
                     d_v_tail, tail_stride, sm_scale, d_out, d_lse, stream):
        """Causal attention of a chunk of n_q[i] <= C new positions per sequence over its pos_end[i] stored positions, its held odd last
        position (tail_idx[i] >= 0: that row of d_k_tail / d_v_tail) and the new positions themselves, ONE launch for any chunk length
        (speckv_ext_attend_chunk; the query stays fp16).  handles, pos_end, n_q, tail_idx: one entry per sequence -- numpy arrays
        (uint64 / uint32 / int32), ctypes arrays or sequences; tail_idx may be None.  Strides in fp16 elements; d_lse may be 0."""
        self._chunk("speckv_ext_attend_chunk", handles, layer, d_q, C, rows_per_pos, pos_end, n_q, d_k_new, d_v_new, seq_stride, pos_stride,
                    tail_idx, d_k_tail, d_v_tail, tail_stride, (), sm_scale, d_out, d_lse, stream)

    def attend_chunk_masked(self, handles, layer, d_q, C, rows_per_pos, pos_end, n_q, d_k_new, d_v_new, seq_stride, pos_stride, tail_idx,
                            d_k_tail, d_v_tail, tail_stride, d_mask, mask_words, sm_scale, d_out, d_lse, stream):
        """attend_chunk for new positions that form a tree (speckv_ext_attend_chunk_masked): d_mask = device uint32 [n][C][mask_words], bit
        t of a query position's row = HELD position t (the tail, if any, is 0; new position a is base + a) is visible to it, under the
        causal bound t < base + j + 1; a row whose own bit is clear is not written.  mask_words >= (C + 32) // 32.  The other arguments
        as attend_chunk."""
        self._chunk("speckv_ext_attend_chunk_masked", handles, layer, d_q, C, rows_per_pos, pos_end, n_q, d_k_new, d_v_new, seq_stride,
                    pos_stride, tail_idx, d_k_tail, d_v_tail, tail_stride, (c_void_p(d_mask or None), mask_words), sm_scale, d_out, d_lse, stream)

    def attend_chunk_split(self, handles, layer, d_q, C, rows_per_pos, pos_end, n_q, d_k_new, d_v_new, seq_stride, pos_stride, tail_idx,
                           d_k_tail, d_v_tail, tail_stride, d_mask, mask_words, n_splits, sm_scale, d_out, d_lse, stream):
        """attend_chunk (d_mask 0) / attend_chunk_masked with the stored positions of a sequence split across the chip
        (speckv_ext_attend_chunk_split): n_splits 1 = whole sequences (the other two entries' launch and bits), N = that many pieces
        per sequence (from the sequence alone), 0 = the library's rule (chunk_split_plan; from the whole call).  With pieces: a piece
        launch and a merge on `stream`; a row's bits depend on its sequence's piece count.  The other arguments as
        attend_chunk_masked."""
        self._chunk("speckv_ext_attend_chunk_split", handles, layer, d_q, C, rows_per_pos, pos_end, n_q, d_k_new, d_v_new, seq_stride,
                    pos_stride, tail_idx, d_k_tail, d_v_tail, tail_stride, (c_void_p(d_mask or None), mask_words, n_splits), sm_scale, d_out,
                    d_lse, stream)

    def chunk_split_plan(self, pos_end, n_q, rows_per_pos, n_splits=0, n_cus=0):
        """The piece rule of attend_chunk_split (speckv_ext_chunk_split_plan; works without init): (pieces, tiles_per_piece), one entry
        per sequence.  n_cus 0: the engine's device, 256 without an engine."""
        n = len(pos_end)
        pe, nq = (c_uint32 * n)(*[int(x) for x in pos_end]), (c_uint32 * n)(*[int(x) for x in n_q])
        pieces, tpp = (c_uint32 * n)(), (c_uint32 * n)()
        self._ext("speckv_ext_chunk_split_plan", n, pe, nq, rows_per_pos, n_splits, n_cus, pieces, tpp)
        return list(pieces), list(tpp)

    def attend_chunk_window(self, handles, layer, d_q, C, rows_per_pos, pos_end, n_q, d_k_new, d_v_new, seq_stride, pos_stride, tail_idx,
                            d_k_tail, d_v_tail, tail_stride, window, n_splits, sm_scale, d_out, d_lse, stream):
        """attend_chunk_split without a mask for a sliding-window (local) layer (speckv_ext_attend_chunk_window): query position j at the
        absolute position P = pos_end + base + j sees the positions [max(0, P + 1 - window), P]; window 0 = none.  A window under which
        no row loses a position issues attend_chunk_split's launches and bits; otherwise a query block walks only the tiles its rows
        see (chunk_window_walk) and n_splits cuts the pool tiles that are left.  The other arguments as attend_chunk_split."""
        self._chunk("speckv_ext_attend_chunk_window", handles, layer, d_q, C, rows_per_pos, pos_end, n_q, d_k_new, d_v_new, seq_stride,
                    pos_stride, tail_idx, d_k_tail, d_v_tail, tail_stride, (window, n_splits), sm_scale, d_out, d_lse, stream)

    def attend_chunk_tree_window(self, handles, layer, d_q, C, rows_per_pos, pos_end, n_q, d_k_new, d_v_new, seq_stride, pos_stride, tail_idx,
                                 d_k_tail, d_v_tail, tail_stride, d_mask, mask_words, d_depth, window, n_splits, sm_scale, d_out, d_lse, stream):
        """attend_chunk_split with a mask for a draft tree on a sliding-window (local) layer (speckv_ext_attend_chunk_tree_window):
        d_depth = device uint32 [n][C], the depth of every node; node j at the absolute position P = pos_end + base + depth[j] sees the
        STORED positions [max(0, P + 1 - window), pos_end) and of the held positions what d_mask says -- the caller folds the window
        into the mask (SpeckvKVConnector.chunk_tree_masks(window=...)), so both come from the same tree.  window 0, or one that cuts
        nothing, issues attend_chunk_split's launches and bits.  The other arguments as attend_chunk_split."""
        self._chunk("speckv_ext_attend_chunk_tree_window", handles, layer, d_q, C, rows_per_pos, pos_end, n_q, d_k_new, d_v_new, seq_stride,
                    pos_stride, tail_idx, d_k_tail, d_v_tail, tail_stride,
                    (c_void_p(d_mask or None), mask_words, c_void_p(d_depth or None), window, n_splits), sm_scale, d_out, d_lse, stream)

    def attend_chunk_kv(self, k_handles, v_handles, layer, d_q, C, rows_per_pos, pos_end, n_q, d_k_new, d_v_new, seq_stride, pos_stride,
                        tail_idx, d_k_tail, d_v_tail, tail_stride, d_mask, mask_words, d_depth, window, n_splits, sm_scale, d_out, d_lse, stream):
        """The chunk attention over a split pool (speckv_ext_attend_chunk_kv): K of `layer` = region `layer` (num_tokens / 2 pages) of the
        FP8 allocation k_handles[i], V = region `layer` of the MXFP4 allocation v_handles[i], ONE launch.  d_mask 0 = the causal form
        (d_depth ignored, window as attend_chunk_window); a mask with a window needs d_depth (attend_chunk_tree_window); n_splits as
        attend_chunk_split.  The other arguments as attend_chunk."""
        n = len(v_handles if k_handles is None else k_handles)             # (None: a NULL array, for the library to refuse)
        handles = lambda h: None if h is None else as_arr(h, c_uint64, n)
        self._ext("speckv_ext_attend_chunk_kv", n, handles(k_handles), handles(v_handles), layer, c_void_p(d_q), C,
                  rows_per_pos, as_arr(pos_end, c_uint32, n), as_arr(n_q, c_uint32, n), c_void_p(d_k_new), c_void_p(d_v_new), seq_stride,
                  pos_stride, None if tail_idx is None else as_arr(tail_idx, c_int32, n), c_void_p(d_k_tail or None),
                  c_void_p(d_v_tail or None), tail_stride, c_void_p(d_mask or None), mask_words, c_void_p(d_depth or None), window, n_splits,
                  sm_scale, c_void_p(d_out), c_void_p(d_lse or None), c_void_p(stream))

    def attend_prefix_fold(self, prefix_handles, first_member, layer, d_q, C, rows_per_pos, prefix_len, n_q, n_splits, sm_scale, d_out, d_lse,
                           stream):
        """Shared-prefix attention folded into the members' own result (speckv_ext_attend_prefix_fold): group g = the allocation
        prefix_handles[g] and the members [first_member[g], first_member[g + 1]) of the call (first_member: n_groups + 1 entries,
        ascending from 0).  Member m brings n_q[m] <= C positions (rows [m][j] of d_q fp16 / d_out fp32 / d_lse, the chunk entries'
        layout) that see the stored positions [0, prefix_len[m]) (even) of its group's prefix; d_out / d_lse hold what the member
        attended on its own (out = 0, lse = -inf: nothing) and are replaced by the softmax over both.  n_splits as attend_chunk_split.
        prefix_handles, first_member, prefix_len, n_q: numpy arrays (uint64 / uint32), ctypes arrays or sequences; d_lse is required."""
        n = len(prefix_handles)
        m = len(prefix_len)
        self._ext("speckv_ext_attend_prefix_fold", n, as_arr(prefix_handles, c_uint64, n), as_arr(first_member, c_uint32, n + 1), layer,
                  c_void_p(d_q), C, rows_per_pos, as_arr(prefix_len, c_uint32, m), as_arr(n_q, c_uint32, m), n_splits, sm_scale,
                  c_void_p(d_out), c_void_p(d_lse or None), c_void_p(stream))

    def attend_prefix_fold_window(self, prefix_handles, first_member, layer, d_q, C, rows_per_pos, prefix_len, n_q, own_seen, d_depth, window,
                                  n_splits, sm_scale, d_out, d_lse, stream):
        """attend_prefix_fold on a sliding-window (local) layer (speckv_ext_attend_prefix_fold_window): own_seen[m] = the member's own
        positions its query position of depth 0 sees, itself included; d_depth = device uint32 [n_members][C] (0 / None: the row of
        position j has depth j); the row of depth d sees [max(0, prefix_len[m] + own_seen[m] + d - window), prefix_len[m]) of the
        prefix and is dead where that is empty.  window 0, or one that cuts nothing, issues attend_prefix_fold's launches.  The other
        arguments as attend_prefix_fold; own_seen like prefix_len."""
        n = len(prefix_handles)
        m = len(prefix_len)
        self._ext("speckv_ext_attend_prefix_fold_window", n, as_arr(prefix_handles, c_uint64, n), as_arr(first_member, c_uint32, n + 1), layer,
                  c_void_p(d_q), C, rows_per_pos, as_arr(prefix_len, c_uint32, m), as_arr(n_q, c_uint32, m),
                  None if own_seen is None else as_arr(own_seen, c_uint32, m), c_void_p(d_depth or None), window, n_splits, sm_scale,
                  c_void_p(d_out), c_void_p(d_lse or None), c_void_p(stream))

    def attend_prefix_fold_kv(self, k_handles, v_handles, first_member, layer, d_q, C, rows_per_pos, prefix_len, n_q, own_seen, d_depth, window,
                              n_splits, sm_scale, d_out, d_lse, stream):
        """attend_prefix_fold_window over a split pool (speckv_ext_attend_prefix_fold_kv): the prefix of group g = region `layer`
        (num_tokens / 2 pages) of the FP8 allocation k_handles[g] for K and of the MXFP4 allocation v_handles[g] for V.  window 0 (own_seen
        may then be None), or one that cuts nothing, issues the unwindowed launches.  The other arguments as attend_prefix_fold_window."""
        n = len(v_handles if k_handles is None else k_handles)             # (None: a NULL array, for the library to refuse)
        m = len(prefix_len)
        handles = lambda h: None if h is None else as_arr(h, c_uint64, n)
        self._ext("speckv_ext_attend_prefix_fold_kv", n, handles(k_handles), handles(v_handles), as_arr(first_member, c_uint32, n + 1), layer,
                  c_void_p(d_q), C, rows_per_pos, as_arr(prefix_len, c_uint32, m), as_arr(n_q, c_uint32, m),
                  None if own_seen is None else as_arr(own_seen, c_uint32, m), c_void_p(d_depth or None), window, n_splits, sm_scale,
                  c_void_p(d_out), c_void_p(d_lse or None), c_void_p(stream))

    def prefix_window_walk(self, first_member, prefix_len, own_seen, n_q, window):
        """The walk rule of attend_prefix_fold_window (speckv_ext_prefix_window_walk; works without init, needs no device):
        (first_tile, n_tiles), one entry per group -- (0, 0) for a group none of whose members still sees its prefix.
        own_seen: one count per member, or None (zeros)."""
        n, m = len(first_member) - 1, len(prefix_len)
        arr = lambda xs, k: (c_uint32 * max(k, 1))(*[int(x) for x in xs])
        first, count = (c_uint32 * max(n, 1))(), (c_uint32 * max(n, 1))()
        self._ext("speckv_ext_prefix_window_walk", n, arr(first_member, n + 1), arr(prefix_len, m),
                  None if own_seen is None else arr(own_seen, m), arr(n_q, m), window, first, count)
        return list(first)[:n], list(count)[:n]

    def chunk_window_walk(self, pos_end, base, n_q, rows_per_pos, window):
        """The walk rule of attend_chunk_window (speckv_ext_chunk_window_walk; works without init, needs no device): (first_tile,
        n_tiles), one entry per (sequence, query block) -- the sequences in order, ceil(n_q / (64 // rows_per_pos)) blocks each.
        base: 0 / 1 held tail positions per sequence, or None."""
        n = len(pos_end)
        per = 64 // rows_per_pos if rows_per_pos in (1, 2, 4, 8, 16) else 64
        total = sum((int(x) + per - 1) // per for x in n_q)
        pe, nq = (c_uint32 * n)(*[int(x) for x in pos_end]), (c_uint32 * n)(*[int(x) for x in n_q])
        bs = None if base is None else (c_uint32 * n)(*[int(x) for x in base])
        first, count = (c_uint32 * max(total, 1))(), (c_uint32 * max(total, 1))()
        self._ext("speckv_ext_chunk_window_walk", n, pe, bs, nq, rows_per_pos, window, first, count)
        return list(first)[:total], list(count)[:total]

    def read(self, handle, offset, dst_ptr, nbytes, on_device):
        self._ext("speckv_ext_read", handle, offset, c_void_p(dst_ptr), nbytes, int(on_device))

    ENGINE_AUTO, ENGINE_KERNEL, ENGINE_COPY = 0, 1, 2

    def fetch_range(self, handle, first_page, n_pages, d_dst, out_f32=False, stream=None, engine=None):
        """engine: None/0 = chosen per batch, 1 = fused peer-load + decompress kernel, 2 = copy engines + local decompress."""
        if engine:
            self._ext("speckv_ext_fetch_range_engine", handle, first_page, n_pages, c_void_p(d_dst), int(out_f32),
                      c_void_p(stream or 0), int(engine))
        else:
            self._ext("speckv_ext_fetch_range", handle, first_page, n_pages, c_void_p(d_dst), int(out_f32), c_void_p(stream or 0))

    def bind_request(self, req_id, handle, local_req=0):
        self._ext("speckv_ext_bind_request", req_id, handle, local_req)

    def fetch_list(self, handle, d_pages, n, d_dst, out_f32=False, stream=None):
        self._ext("speckv_ext_fetch_list", handle, c_void_p(d_pages), n, c_void_p(d_dst), int(out_f32), c_void_p(stream or 0))

    def access_batch(self, handle, offsets):
        n = len(offsets)
        offs = (c_uint64 * n)(*offsets)
        out = (c_void_p * n)()
        self._ext("speckv_ext_access_batch", handle, offs, n, out)
        return [p or 0 for p in out]

    def prefetch_batch(self, req_ids, layers, cur_pos, depth_k=None):
        """Sequences of ints, or contiguous numpy arrays (uint32 / uint16 / uint32 / uint32) passed without a copy."""
        n = len(req_ids)
        if hasattr(req_ids, "ctypes"):
            as_p = lambda a, t: a.ctypes.data_as(ctypes.POINTER(t))
            self._ext("speckv_ext_prefetch_batch", n, as_p(req_ids, c_uint32), as_p(layers, c_uint16), as_p(cur_pos, c_uint32),
                      as_p(depth_k, c_uint32) if depth_k is not None else None)
            return
        k = (c_uint32 * n)(*depth_k) if depth_k is not None else None
        self._ext("speckv_ext_prefetch_batch", n, (c_uint32 * n)(*req_ids), (c_uint16 * n)(*layers),
                  (c_uint32 * n)(*cur_pos), k)

    def prefetch_flush(self, want_count=True):
        """Submit the queued look-ahead requests (device-side pipeline).  want_count=False only submits; True also
        waits for the page count (not for the data)."""
        if not want_count:
            self._ext("speckv_ext_prefetch_flush", None)
            return None
        n = c_uint32()
        self._ext("speckv_ext_prefetch_flush", ctypes.byref(n))
        return n.value

    def verify(self, req_id, actual_token, predicted=None):
        """predicted=None: verify against the engine's own prediction for req_id."""
        hit, depth = c_uint32(), c_uint32()
        if predicted is None:
            self._ext("speckv_ext_verify", req_id, actual_token, None, 0, ctypes.byref(hit), ctypes.byref(depth))
        else:
            arr = (c_int32 * max(len(predicted), 1))(*predicted)
            self._ext("speckv_ext_verify", req_id, actual_token, arr, len(predicted), ctypes.byref(hit), ctypes.byref(depth))
        return bool(hit.value), depth.value

    def predictor_load(self, emb_ptr, wout_ptr, vocab, on_device):
        self._ext("speckv_ext_predictor_load", c_void_p(emb_ptr), c_void_p(wout_ptr), vocab, int(on_device))

    def predictor_load_lstm(self, emb_ptr, vocab, w_ih, w_hh, b_ih, b_hh, wout_ptr, out_bias_ptr, on_device):
        """A real LSTM cell (PyTorch nn.LSTM layout): w_ih / w_hh / b_ih / b_hh are lists of pointers, one per layer."""
        n = len(w_ih)
        arr = lambda ps: (c_void_p * n)(*ps)
        self._ext("speckv_ext_predictor_load_lstm", c_void_p(emb_ptr), vocab, n, arr(w_ih), arr(w_hh), arr(b_ih), arr(b_hh),
                  c_void_p(wout_ptr), c_void_p(out_bias_ptr or 0), int(on_device))

    def predict_batch(self, n, d_hist, k, d_tok, d_conf, stream=None):
        self._ext("speckv_ext_predict_batch", n, c_void_p(d_hist), k, c_void_p(d_tok), c_void_p(d_conf), c_void_p(stream or 0))

    def prefetch_depth(self):
        d = c_uint32()
        self._ext("speckv_ext_get_prefetch_depth", ctypes.byref(d))
        return d.value

    def poll_complete(self):
        d = c_uint32()
        self._ext("speckv_ext_poll_complete", ctypes.byref(d))
        return d.value

    def sync(self):
        self._ext("speckv_ext_sync")

    def qk_scores_fp8(self, handle, layer, d_q_f16, g, pos_begin, pos_end, d_out, stream=None):
        self._ext("speckv_ext_qk_scores_fp8", handle, layer, c_void_p(d_q_f16), g, pos_begin, pos_end,
                  c_void_p(d_out), c_void_p(stream or 0))

    def qk_scores_fp8_layers(self, handle, layer_begin, n_layers, d_q_f16, g, pos_begin, pos_end, d_out, stream=None):
        self._ext("speckv_ext_qk_scores_fp8_layers", handle, layer_begin, n_layers, c_void_p(d_q_f16), g, pos_begin,
                  pos_end, c_void_p(d_out), c_void_p(stream or 0))

    def attend_fp8(self, handle, layer_begin, n_layers, d_q_f16, g, pos_begin, pos_end, sm_scale, d_out, d_lse=None,
                   stream=None):
        self._ext("speckv_ext_attend_fp8", handle, layer_begin, n_layers, c_void_p(d_q_f16), g, pos_begin, pos_end,
                  ctypes.c_float(sm_scale), c_void_p(d_out), c_void_p(d_lse or 0), c_void_p(stream or 0))

    def attend_fp8_batch(self, handles, layer, d_q_f16, g, pos_end, sm_scale, d_out, d_lse=None, stream=None):
        """handles / pos_end: sequences of ints, or ready ctypes arrays (c_uint64 / c_uint32) that a caller reuses over
        the layers of a decode step."""
        n = len(handles)
        hs = handles if isinstance(handles, ctypes.Array) else (c_uint64 * n)(*handles)
        pe = pos_end if isinstance(pos_end, ctypes.Array) else (c_uint32 * n)(*pos_end)
        self._ext("speckv_ext_attend_fp8_batch", n, hs, layer, c_void_p(d_q_f16), g, pe, ctypes.c_float(sm_scale),
                  c_void_p(d_out), c_void_p(d_lse or 0), c_void_p(stream or 0))

    def attend_kv_batch(self, k_handles, v_handles, layer, d_q_f16, g, pos_end, sm_scale, d_out, d_lse=None, stream=None):
        """One decode step of a batch over a split pool (speckv_ext_attend_kv_batch): K of `layer` = region `layer` (num_tokens / 2 pages) of
        the FP8 allocation k_handles[i], V = region `layer` of the MXFP4 allocation v_handles[i]; d_q_f16 [n][heads][g][128] fp16, d_out
        [n][heads][g][128] fp32, d_lse optional [n][heads][g].  k_handles / v_handles / pos_end: numpy arrays (uint64 / uint32), ctypes
        arrays or sequences; None stands for a NULL array (for the library to refuse)."""
        n = len(pos_end if k_handles is None and v_handles is None else (v_handles if k_handles is None else k_handles))
        handles = lambda h: None if h is None else as_arr(h, c_uint64, n)
        self._ext("speckv_ext_attend_kv_batch", n, handles(k_handles), handles(v_handles), layer, c_void_p(d_q_f16), g,
                  None if pos_end is None else as_arr(pos_end, c_uint32, n), ctypes.c_float(sm_scale), c_void_p(d_out), c_void_p(d_lse or 0),
                  c_void_p(stream or 0))

    def attend_kv_batch_window(self, k_handles, v_handles, layer, d_q_f16, g, pos_end, q_pos, window, sm_scale, d_out, d_lse=None, stream=None):
        """attend_kv_batch for a sliding-window layer (speckv_ext_attend_kv_batch_window): member i has q_pos[i] + 1 positions (pos_end[i] = that
        & ~1 stored, an odd one more in the caller's tail) and its query sees the last `window` of them; every member is walked from its
        window's tile in both allocations.  window 0 (q_pos may then be None), or a window that cuts no member: the launches of
        attend_kv_batch.  Arrays as there; None stands for a NULL array."""
        n = len(pos_end if k_handles is None and v_handles is None else (v_handles if k_handles is None else k_handles))
        handles = lambda h: None if h is None else as_arr(h, c_uint64, n)
        u32 = lambda a: None if a is None else as_arr(a, c_uint32, n)
        self._ext("speckv_ext_attend_kv_batch_window", n, handles(k_handles), handles(v_handles), layer, c_void_p(d_q_f16), g, u32(pos_end),
                  u32(q_pos), window, ctypes.c_float(sm_scale), c_void_p(d_out), c_void_p(d_lse or 0), c_void_p(stream or 0))

    def attend_kv_spec(self, k_handles, v_handles, layer, d_q_f16, g, rows_per_pos, pos_end, d_k_held, d_v_held, seq_stride_elems, pos_stride_elems,
                       d_mask, mask_stride, sm_scale, d_out, d_lse=None, stream=None):
        """One multi-position step of a batch over a split pool (speckv_ext_attend_kv_spec): attend_kv_batch with g = n_q x rows_per_pos
        query rows per kv head, and the positions held outside the pool (fp16 rows as attend_fold_held takes them, visibility from the
        uint32 words d_mask[i * mask_stride + j] as attend_fold_masked takes them) folded in inside the same launch.  Arrays as
        attend_kv_batch; 0 / None stands for a NULL pointer (for the library to refuse)."""
        n = len(pos_end if k_handles is None and v_handles is None else (v_handles if k_handles is None else k_handles))
        handles = lambda h: None if h is None else as_arr(h, c_uint64, n)
        self._ext("speckv_ext_attend_kv_spec", n, handles(k_handles), handles(v_handles), layer, c_void_p(d_q_f16), g, rows_per_pos,
                  None if pos_end is None else as_arr(pos_end, c_uint32, n), c_void_p(d_k_held or 0), c_void_p(d_v_held or 0), seq_stride_elems,
                  pos_stride_elems, c_void_p(d_mask or 0), mask_stride, ctypes.c_float(sm_scale), c_void_p(d_out), c_void_p(d_lse or 0),
                  c_void_p(stream or 0))

    def attend_kv_spec_window(self, k_handles, v_handles, layer, d_q_f16, g, rows_per_pos, pos_end, length, d_depth, window, d_k_held, d_v_held,
                              seq_stride_elems, pos_stride_elems, d_mask, mask_stride, sm_scale, d_out, d_lse=None, stream=None):
        """attend_kv_spec on a sliding-window layer (speckv_ext_attend_kv_spec_window): `length` = the committed positions of every
        sequence (pos_end[i] or pos_end[i] + 1), d_depth = the device table of node depths strided like d_mask, window = W; the stored
        positions are masked per query row by its depth, the held ones by d_mask as ever.  window = 0: attend_kv_spec.  Arrays as
        attend_kv_batch; 0 / None stands for a NULL pointer (for the library to refuse)."""
        n = len(pos_end if k_handles is None and v_handles is None else (v_handles if k_handles is None else k_handles))
        handles = lambda h: None if h is None else as_arr(h, c_uint64, n)
        u32 = lambda a: None if a is None else as_arr(a, c_uint32, n)
        self._ext("speckv_ext_attend_kv_spec_window", n, handles(k_handles), handles(v_handles), layer, c_void_p(d_q_f16), g, rows_per_pos, u32(pos_end),
                  u32(length), c_void_p(d_depth or 0), window, c_void_p(d_k_held or 0), c_void_p(d_v_held or 0), seq_stride_elems, pos_stride_elems,
                  c_void_p(d_mask or 0), mask_stride, ctypes.c_float(sm_scale), c_void_p(d_out), c_void_p(d_lse or 0), c_void_p(stream or 0))

    def attend_int4_batch(self, handles, layer, d_q_f16, g, pos_end, sm_scale, d_out, d_lse=None, stream=None):
        """handles / pos_end: sequences of ints, or ready ctypes arrays (c_uint64 / c_uint32) that a caller reuses over
        the layers of a decode step."""
        n = len(handles)
        hs = handles if isinstance(handles, ctypes.Array) else (c_uint64 * n)(*handles)
        pe = pos_end if isinstance(pos_end, ctypes.Array) else (c_uint32 * n)(*pos_end)
        self._ext("speckv_ext_attend_int4_batch", n, hs, layer, c_void_p(d_q_f16), g, pe, ctypes.c_float(sm_scale),
                  c_void_p(d_out), c_void_p(d_lse or 0), c_void_p(stream or 0))

    def attend_fold_tail(self, n_rows, d_rows, heads, g, d_q_f16, d_k_tail, d_v_tail, tail_stride_elems, sm_scale, d_out, d_lse,
                         stream=None):
        """Fold the not-yet-stored position (fp16 K / V tails) into out / lse of rows d_rows (0 / None: all, in order)."""
        self._ext("speckv_ext_attend_fold_tail", n_rows, c_void_p(d_rows or 0), heads, g, c_void_p(d_q_f16), c_void_p(d_k_tail),
                  c_void_p(d_v_tail), tail_stride_elems, ctypes.c_float(sm_scale), c_void_p(d_out), c_void_p(d_lse), c_void_p(stream or 0))

    def attend_fold_held(self, n_rows, d_rows, heads, g, rows_per_pos, d_q_f16, d_k_held, d_v_held, seq_stride_elems, pos_stride_elems, d_base,
                         d_n_q, sm_scale, d_out, d_lse, stream=None):
        """Fold the positions held outside the pool causally into out / lse of rows d_rows (0 / None: all, in order): query position
        j = row // rows_per_pos of sequence i sees held positions 0 .. d_base[i] + j; positions >= d_n_q[i] (0 / None: none) untouched."""
        self._ext("speckv_ext_attend_fold_held", n_rows, c_void_p(d_rows or 0), heads, g, rows_per_pos, c_void_p(d_q_f16), c_void_p(d_k_held),
                  c_void_p(d_v_held), seq_stride_elems, pos_stride_elems, c_void_p(d_base or 0), c_void_p(d_n_q or 0), ctypes.c_float(sm_scale),
                  c_void_p(d_out), c_void_p(d_lse or 0), c_void_p(stream or 0))

    def attend_fold_masked(self, n_rows, d_rows, heads, g, rows_per_pos, d_q_f16, d_k_held, d_v_held, seq_stride_elems, pos_stride_elems, d_mask,
                           mask_stride, sm_scale, d_out, d_lse, stream=None):
        """attend_fold_held with visibility from a mask table (a tree of drafts): query position j = row // rows_per_pos of sequence i sees
        the held positions whose bits are set in the uint32 word d_mask[i * mask_stride + j]; a word of 0 leaves the position untouched."""
        self._ext("speckv_ext_attend_fold_masked", n_rows, c_void_p(d_rows or 0), heads, g, rows_per_pos, c_void_p(d_q_f16), c_void_p(d_k_held),
                  c_void_p(d_v_held), seq_stride_elems, pos_stride_elems, c_void_p(d_mask or 0), mask_stride, ctypes.c_float(sm_scale),
                  c_void_p(d_out), c_void_p(d_lse or 0), c_void_p(stream or 0))

    def attend_plan_bytes(self, n_seq):
        return int(self.lib.speckv_ext_attend_plan_bytes(n_seq))

    def attend_batch_plan(self, handles, pos_end, max_pos_end, d_plan, plan_bytes, stream):
        """Once per decode step, outside any graph capture: the per-sequence descriptors of the step (valid for every
        layer) written to the device buffer d_plan."""
        n = len(handles)
        hs = handles if isinstance(handles, ctypes.Array) else (c_uint64 * n)(*handles)
        pe = pos_end if isinstance(pos_end, ctypes.Array) else (c_uint32 * n)(*pos_end)
        self._ext("speckv_ext_attend_batch_plan", n, hs, pe, max_pos_end, c_void_p(d_plan), plan_bytes, c_void_p(stream))

    # ---- the batch and planned forms under a sliding window (include/speckv_ext.h)
    def attend_plan_window_bytes(self, n_seq):
        return int(self.lib.speckv_ext_attend_plan_window_bytes(n_seq))

    def attend_batch_plan_window(self, handles, pos_end, q_pos, window, max_pos_end, d_plan, plan_bytes, stream):
        """attend_batch_plan for a sliding-window layer: member i has q_pos[i] + 1 positions (pos_end[i] = that & ~1 stored, an odd one more in
        the caller's tail) and its query sees the last `window` of them.  The planned entries run over the plan as over any other; d_plan
        holds attend_plan_window_bytes(n) bytes."""
        n = len(handles)
        hs = handles if isinstance(handles, ctypes.Array) else (c_uint64 * n)(*handles)
        pe = pos_end if isinstance(pos_end, ctypes.Array) else (c_uint32 * n)(*[int(x) for x in pos_end])
        qp = q_pos if isinstance(q_pos, ctypes.Array) else (c_uint32 * n)(*[int(x) for x in q_pos])
        self._ext("speckv_ext_attend_batch_plan_window", n, hs, pe, qp, window, max_pos_end, c_void_p(d_plan), plan_bytes, c_void_p(stream))

    def attend_batch_window(self, scheme, handles, layer, d_q_f16, g, pos_end, q_pos, window, sm_scale, d_out, d_lse=None, stream=None):
        """attend_{fp8,int4,mx4}_batch for a sliding-window layer (scheme: 4 FP8_E4M3, 3 INT4_G32, 5 MXFP4); pos_end / q_pos as
        attend_batch_plan_window.  window 0: the entry without one."""
        n = len(handles)
        hs = handles if isinstance(handles, ctypes.Array) else (c_uint64 * n)(*handles)
        pe = pos_end if isinstance(pos_end, ctypes.Array) else (c_uint32 * n)(*[int(x) for x in pos_end])
        qp = None if q_pos is None else q_pos if isinstance(q_pos, ctypes.Array) else (c_uint32 * n)(*[int(x) for x in q_pos])
        self._ext("speckv_ext_attend_batch_window", scheme, n, hs, layer, c_void_p(d_q_f16), g, pe, qp, window, ctypes.c_float(sm_scale),
                  c_void_p(d_out), c_void_p(d_lse or 0), c_void_p(stream))

    def decode_window_range(self, length, window):
        """The walk rule of the windowed decode attention (speckv_ext_decode_window_range; works without init, needs no device): (begin, skip,
        n_pages) of a member of `length` positions, the step's own included, under `window` (0: none)."""
        b, k, n = c_uint32(0), c_uint32(0), c_uint32(0)
        self._ext("speckv_ext_decode_window_range", length, window, ctypes.byref(b), ctypes.byref(k), ctypes.byref(n))
        return b.value, k.value, n.value

    def spec_window_range(self, length, window):
        """The walk rule of attend_kv_spec_window (speckv_ext_spec_window_range; works without init, needs no device): (begin, rel, n_pages)
        of a member of `length` committed positions under `window` >= 1; rel is signed."""
        b, r, n = c_uint32(0), ctypes.c_int32(0), c_uint32(0)
        self._ext("speckv_ext_spec_window_range", length, window, ctypes.byref(b), ctypes.byref(r), ctypes.byref(n))
        return b.value, r.value, n.value

    def attend_planned(self, scheme, d_plan, n_seq, layer, d_q_f16, g, max_pos_end, sm_scale, d_out, d_lse, stream):
        """One layer of a planned batch: kernel launches only (capturable).  scheme: 4 (FP8_E4M3) or 3 (INT4_G32)."""
        name = {4: "speckv_ext_attend_fp8_planned", 3: "speckv_ext_attend_int4_planned", 5: "speckv_ext_attend_mx4_planned"}[scheme]
        self._ext(name, c_void_p(d_plan), n_seq, layer, c_void_p(d_q_f16), g, max_pos_end, ctypes.c_float(sm_scale),
                  c_void_p(d_out), c_void_p(d_lse or 0), c_void_p(stream))

    def attend_planned_layers(self, scheme, d_plan, n_seq, layer_begin, n_layers, d_q_f16, g, max_pos_end, sm_scale, d_out, d_lse, stream, n_tail=0,
                              d_tail_rows=0, d_tail_idx=0, d_k_tail=0, d_v_tail=0, tail_stride_elems=0):
        """Several layers of a planned batch in one call: q [n_layers][n_seq][heads][g][128], out / lse likewise."""
        self._ext("speckv_ext_attend_planned_layers", scheme, c_void_p(d_plan), n_seq, layer_begin, n_layers, c_void_p(d_q_f16), g, max_pos_end,
                  ctypes.c_float(sm_scale), c_void_p(d_out), c_void_p(d_lse or 0), n_tail, c_void_p(d_tail_rows or 0), c_void_p(d_tail_idx or 0),
                  c_void_p(d_k_tail or 0), c_void_p(d_v_tail or 0), tail_stride_elems, c_void_p(stream))

    def attend_planned_tail(self, scheme, d_plan, n_seq, layer, d_q_f16, g, max_pos_end, sm_scale, d_out, d_lse, n_tail, d_tail_rows, d_tail_idx,
                            d_k_tail, d_v_tail, tail_stride_elems, stream):
        """attend_planned + the position still held outside the pool (fp16 rows [n_tail][layers][heads][128]) in one call: folded in by
        the MXFP4 attention kernel itself, by one fold launch inside the call for the other formats."""
        self._ext("speckv_ext_attend_planned_tail", scheme, c_void_p(d_plan), n_seq, layer, c_void_p(d_q_f16), g, max_pos_end, ctypes.c_float(sm_scale),
                  c_void_p(d_out), c_void_p(d_lse), n_tail, c_void_p(d_tail_rows or 0), c_void_p(d_tail_idx or 0), c_void_p(d_k_tail or 0),
                  c_void_p(d_v_tail or 0), tail_stride_elems, c_void_p(stream))

    def attend_int4(self, handle, layer_begin, n_layers, d_q_f16, g, pos_begin, pos_end, sm_scale, d_out, d_lse=None,
                    stream=None):
        self._ext("speckv_ext_attend_int4", handle, layer_begin, n_layers, c_void_p(d_q_f16), g, pos_begin, pos_end,
                  ctypes.c_float(sm_scale), c_void_p(d_out), c_void_p(d_lse or 0), c_void_p(stream or 0))

    def attend_mx4(self, handle, layer_begin, n_layers, d_q_f16, g, pos_begin, pos_end, sm_scale, d_out, d_lse=None,
                   stream=None):
        self._ext("speckv_ext_attend_mx4", handle, layer_begin, n_layers, c_void_p(d_q_f16), g, pos_begin, pos_end,
                  ctypes.c_float(sm_scale), c_void_p(d_out), c_void_p(d_lse or 0), c_void_p(stream or 0))

    def attend_mx4_batch(self, handles, layer, d_q_f16, g, pos_end, sm_scale, d_out, d_lse=None, stream=None):
        n = len(handles)
        hs = handles if isinstance(handles, ctypes.Array) else (c_uint64 * n)(*handles)
        pe = pos_end if isinstance(pos_end, ctypes.Array) else (c_uint32 * n)(*pos_end)
        self._ext("speckv_ext_attend_mx4_batch", n, hs, layer, c_void_p(d_q_f16), g, pe, ctypes.c_float(sm_scale),
                  c_void_p(d_out), c_void_p(d_lse or 0), c_void_p(stream or 0))

    def stream_is_capturing(self, stream):
        """True while `stream` (a hipStream_t value) is being captured into a HIP graph"""
        out = ctypes.c_int(0)
        self._ext("speckv_ext_stream_is_capturing", c_void_p(stream or 0), ctypes.byref(out))
        return bool(out.value)

    def set_tuning(self, key, value):
        """A launch-form switch of the library (speckv_ext_set_tuning: the environment is read once per process)."""
        self.lib.speckv_ext_set_tuning.argtypes = [ctypes.c_char_p, ctypes.c_longlong]
        self.lib.speckv_ext_set_tuning.restype = ctypes.c_int
        if self.lib.speckv_ext_set_tuning(key.encode(), int(value)) != 0:
            raise ValueError(f"speckv_ext_set_tuning: no such key {key!r}")

    def codec_launch_shape(self, n_blocks, n_cus=0):
        """The shape of a block-codec launch of n_blocks under the tuning in force (speckv_ext_codec_launch_shape; works without init):
        (grid, per_wave, wave_step).  n_cus 0: the device's CUs, 256 without a device."""
        grid, per_wave, step = c_uint32(), c_uint64(), c_uint64()
        self._ext("speckv_ext_codec_launch_shape", int(n_blocks), int(n_cus), ctypes.byref(grid), ctypes.byref(per_wave), ctypes.byref(step))
        return grid.value, per_wave.value, step.value

    def fetch_sweep_next(self, prev, first, n, capturing=False, mode=-1):
        """The direction and store marking fetch_range gives a kernel-path launch (speckv_ext_fetch_sweep_next; works without init).
        prev = the allocation's previous fetch (first, n, descending, valid), or None; mode < 0: the tuning key fetch_sweep in force.
        Returns (descending, keep_stores, (first, n, descending, valid))."""
        pf, pn, pd, pv = prev if prev is not None else (0, 0, 0, 0)
        down, keep, state = c_uint32(), c_uint32(), (c_uint64 * 4)()
        self._ext("speckv_ext_fetch_sweep_next", int(pf), int(pn), int(pd), int(pv), int(first), int(n), int(bool(capturing)), int(mode),
                  ctypes.byref(down), ctypes.byref(keep), state)
        return down.value, keep.value, tuple(int(v) for v in state)

    def promote_to_l1(self, handle, offset):
        return self.lib.speckv_ext_promote_to_l1(handle, offset) == 0

    def demote_to_l3(self, handle, offset):
        return self.lib.speckv_ext_demote_to_l3(handle, offset) == 0

    def migrate(self, handle, first_page, n_pages, target_pool):
        self._ext("speckv_ext_migrate", handle, first_page, n_pages, target_pool)

    def compact(self, handle):
        """Seal an allocation (pack its INT8_DELTA_RLE records, free the slots).  Returns (pool bytes before, after)."""
        before, after = c_uint64(), c_uint64()
        self._ext("speckv_ext_compact", handle, ctypes.byref(before), ctypes.byref(after))
        return before.value, after.value

    def stats(self):
        s = Stats()
        n = c_size_t()
        self._ext("speckv_ext_stats_sized", ctypes.byref(s), ctypes.sizeof(s), ctypes.byref(n))
        if n.value != ctypes.sizeof(s):
            raise RuntimeError(f"speckv_ext_stats_sized wrote {n.value} bytes, the binding's struct has {ctypes.sizeof(s)}")
        return s
