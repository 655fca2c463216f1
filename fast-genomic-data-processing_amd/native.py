"""ctypes binding of libmgx.so -- mirrors include/*.h one to one."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


class MgxError(RuntimeError):
    pass


def lib_path():
    return os.path.join(_HERE, "libmgx.so")


class PairHMMInput(C.Structure):
    _fields_ = [
        ("n_reads", C.c_uint64), ("read_off", C.c_void_p), ("bases", C.c_void_p),
        ("qual", C.c_void_p), ("ins", C.c_void_p), ("del_", C.c_void_p), ("gcp", C.c_void_p),
        ("n_haps", C.c_uint64), ("hap_off", C.c_void_p), ("hap_bases", C.c_void_p),
        ("n_pairs", C.c_uint64), ("pair_read", C.c_void_p), ("pair_hap", C.c_void_p),
    ]


class PairHMMWire(C.Structure):
    _fields_ = [
        ("n_reads", C.c_uint64), ("n_haps", C.c_uint64), ("n_pairs", C.c_uint64),
        ("read_off", C.c_void_p), ("hap_off", C.c_void_p), ("pair_read", C.c_void_p), ("pair_hap", C.c_void_p),
        ("w_qual", C.c_uint8), ("w_ins", C.c_uint8), ("w_del", C.c_uint8), ("w_gcp", C.c_uint8), ("gcp_const", C.c_uint8),
        ("pad_", C.c_uint8 * 3),
        ("bases4", C.c_void_p), ("qual", C.c_void_p), ("ins", C.c_void_p), ("del_", C.c_void_p), ("gcp", C.c_void_p),
        ("hap4", C.c_void_p),
    ]


class PairHMMStats(C.Structure):
    _fields_ = [
        ("n_pairs", C.c_uint64), ("cells", C.c_uint64), ("alg_bytes", C.c_uint64),
        ("n_rerun_f64", C.c_uint64), ("n_launches_f32", C.c_uint32), ("n_launches_f64", C.c_uint32),
        ("n_runs_timed", C.c_uint32), ("ms_f32", C.c_float), ("ms_f64", C.c_float), ("ms_f32_dominant", C.c_float),
        ("dominant_cells", C.c_uint64), ("dominant_alg_bytes", C.c_uint64),
        ("dominant_kernel", C.c_char * 64), ("n_exact", C.c_uint64),
        ("n_nhap_f32", C.c_uint64), ("n_form_deferred_f32", C.c_uint64),
    ]


class QueueConfig(C.Structure):
    _fields_ = [("n_devices", C.c_uint32), ("devices", C.c_void_p), ("lanes_per_device", C.c_uint32),
                ("depth", C.c_uint32), ("batch_pairs", C.c_uint32), ("flags", C.c_uint)]


class QueueStats(C.Structure):
    _fields_ = [("n_pairs", C.c_uint64), ("n_batches", C.c_uint64), ("cells", C.c_uint64),
                ("bytes_h2d", C.c_uint64), ("bytes_d2h", C.c_uint64), ("seconds", C.c_double),
                ("pack_seconds", C.c_double), ("wait_seconds", C.c_double), ("n_lanes", C.c_uint32),
                ("batches_per_device", C.c_uint64 * 16)]


class ReadModel(C.Structure):
    _fields_ = [("pcr_rate_factor", C.c_int), ("base_quality_threshold", C.c_int), ("constant_gcp", C.c_int),
                ("log10_mismapping_rate", C.c_double), ("max_error_per_base", C.c_double)]


# every symbol include/mgx_pairhmm.h declares: name -> (restype, argtypes)
PAIRHMM_SYMBOLS = {
    "mgx_last_error": (C.c_char_p, []),
    "mgx_pairhmm_create": (C.c_int, [C.c_int, C.c_uint, C.POINTER(C.c_void_p)]),
    "mgx_pairhmm_destroy": (None, [C.c_void_p]),
    "mgx_pairhmm_compute": (C.c_int, [C.c_void_p, C.POINTER(PairHMMInput), C.c_void_p]),
    "mgx_pairhmm_compute_regions": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "mgx_pairhmm_batch_create": (C.c_int, [C.c_void_p, C.POINTER(PairHMMInput), C.POINTER(C.c_void_p)]),
    "mgx_pairhmm_batch_run": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mgx_pairhmm_batch_results": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mgx_pairhmm_batch_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(PairHMMStats)]),
    "mgx_pairhmm_batch_destroy": (None, [C.c_void_p, C.c_void_p]),
    "mgx_pairhmm_sync": (C.c_int, [C.c_void_p]),
    "mgx_read_model_defaults": (None, [C.c_void_p]),
    "mgx_pairhmm_region": (C.c_int, [C.c_void_p, C.POINTER(PairHMMInput), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mgx_pairhmm_regions": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mgx_pairhmm_queue_create": (C.c_int, [C.POINTER(QueueConfig), C.POINTER(C.c_void_p)]),
    "mgx_pairhmm_queue_destroy": (None, [C.c_void_p]),
    "mgx_pairhmm_queue_run": (C.c_int, [C.c_void_p, C.POINTER(PairHMMInput), C.c_void_p, C.c_void_p]),
    "mgx_pairhmm_queue_run_range": (C.c_int, [C.c_void_p, C.POINTER(PairHMMInput), C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]),
    "mgx_pairhmm_queue_run_regions": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "mgx_pairhmm_queue_stats": (C.c_int, [C.c_void_p, C.POINTER(QueueStats)]),
    "mgx_pairhmm_pack_batch": (C.c_int, [C.POINTER(PairHMMInput), C.c_uint64, C.c_uint64, C.c_void_p, C.c_size_t,
                                         C.POINTER(PairHMMInput), C.POINTER(C.c_size_t)]),
    "mgx_pairhmm_pack_batch_wire": (C.c_int, [C.POINTER(PairHMMInput), C.c_uint64, C.c_uint64, C.c_void_p, C.c_size_t,
                                              C.POINTER(PairHMMWire), C.POINTER(C.c_size_t)]),
    "mgx_pairhmm_wire_expand_host": (C.c_int, [C.POINTER(PairHMMWire)] + [C.c_void_p] * 6),
    "mgx_pairhmm_batch_read_inputs": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_void_p] * 6),
    "mgx_pairhmm_regions_modified_inputs": (C.c_int, [C.c_void_p, C.c_uint32] + [C.c_void_p] * 7),
    "mgx_pairhmm_table_f32": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "mgx_pairhmm_table_f64": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
}

SYMBOLS = dict(PAIRHMM_SYMBOLS)


def load():
    """Loads libmgx.so (never falls back to anything else)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        raise MgxError(
            f"{path} is missing: build it with `python __graft_entry__.py build` "
            "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    # The sort pipeline overlaps its three sorts on three HIP streams; the runtime maps streams onto
    # GPU_MAX_HW_QUEUES hardware queues (default 4) and two streams on one queue serialise, which is
    # what happens once another context (PairHMM, torch) holds streams in the same process.  Only takes
    # effect if the HIP runtime has not been initialised yet; an explicit setting is respected.
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
    lib = C.CDLL(path)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)       # AttributeError if the ABI and the header diverge
        fn.restype = res
        fn.argtypes = args
    _LIB = lib
    return lib


def check(rc):
    if rc != 0:
        msg = load().mgx_last_error()
        raise MgxError(f"libmgx error {rc}: {msg.decode() if msg else ''}")


# ---- include/mgx_sortdedup.h -------------------------------------------------------------------
class RawRecords(C.Structure):
    _fields_ = [
        ("n_records", C.c_uint64), ("flag", C.c_void_p), ("tid", C.c_void_p), ("pos", C.c_void_p),
        ("cigar_off", C.c_void_p), ("cigar", C.c_void_p), ("qual_off", C.c_void_p), ("qual", C.c_void_p),
        ("qname_off", C.c_void_p), ("qname", C.c_void_p), ("n_targets", C.c_uint32), ("target_len", C.c_void_p),
    ]


class SortDedupStats(C.Structure):
    _fields_ = [
        ("n_records", C.c_uint64), ("n_double", C.c_uint64), ("n_single", C.c_uint64), ("n_dup_records", C.c_uint64),
        ("key_bits_coord", C.c_uint32), ("key_bits_pair1", C.c_uint32), ("key_bits_pair2", C.c_uint32),
        ("n_radix_passes", C.c_uint32), ("ms_total", C.c_float), ("ms_radix_scatter", C.c_float),
        ("radix_scatter_bytes", C.c_uint64), ("alg_bytes", C.c_uint64),
        ("ms_scatter_records", C.c_float), ("n_scatter_records", C.c_uint32), ("scatter_records_bytes", C.c_uint64),
        ("n_key_hist_launches", C.c_uint32), ("pad_", C.c_uint32),
        # which paths the returned pipeline pass took
        ("n_near", C.c_uint32), ("n_multi_far", C.c_uint32), ("n_multi_single", C.c_uint32), ("n_multi_near", C.c_uint32),
        ("n_long_far", C.c_uint32), ("n_long_single", C.c_uint32), ("n_long_near", C.c_uint32),
        ("n_builds", C.c_uint32), ("n_pipeline_runs", C.c_uint32), ("bitmap_tiled", C.c_uint32),
        ("packed_coord", C.c_uint32), ("packed_pair", C.c_uint32), ("near_by_position", C.c_uint32), ("pad2_", C.c_uint32),
    ]


class SortDedupShard(C.Structure):
    _fields_ = [("n_order", C.c_uint64), ("order_coord", C.c_void_p), ("order_arrival", C.c_void_p),
                ("n_mark", C.c_uint64), ("mark_recs", C.c_void_p), ("mark_arrival", C.c_void_p),
                ("n_marks", C.c_uint64), ("marks", C.c_void_p), ("order_base", C.c_uint64),
                ("coord_lo", C.c_uint64), ("coord_hi", C.c_uint64)]


SORTDEDUP_SYMBOLS = {
    "mgx_sortdedup_route": (C.c_int, [C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint32, C.c_int, C.POINTER(C.c_void_p)]),
    "mgx_sortdedup_routed_shard": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(SortDedupShard)]),
    "mgx_sortdedup_routed_free": (None, [C.c_void_p]),
    "mgx_sortdedup_upload_shard": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(SortDedupShard)]),
    "mgx_sortdedup_merge": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mgx_sortdedup_pack": (C.c_int, [C.POINTER(RawRecords), C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]),
    "mgx_sortdedup_pack_scored": (C.c_int, [C.POINTER(RawRecords), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]),
    "mgx_sortdedup_create": (C.c_int, [C.c_int, C.c_uint, C.POINTER(C.c_void_p)]),
    "mgx_sortdedup_destroy": (None, [C.c_void_p]),
    "mgx_sortdedup_upload": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]),
    "mgx_sortdedup_upload_begin": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64]),
    "mgx_sortdedup_upload_chunk": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]),
    "mgx_sortdedup_upload_end": (C.c_int, [C.c_void_p, C.c_uint64]),
    "mgx_sortdedup_run": (C.c_int, [C.c_void_p]),
    "mgx_sortdedup_results": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "mgx_sortdedup_stats": (C.c_int, [C.c_void_p, C.POINTER(SortDedupStats)]),
    "mgx_sortdedup_sort_mark": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
}
SYMBOLS.update(SORTDEDUP_SYMBOLS)


# ---- include/mgx_smithwaterman.h ---------------------------------------------------------------
class SwParams(C.Structure):
    _fields_ = [("match", C.c_int32), ("mismatch", C.c_int32), ("gap_open", C.c_int32), ("gap_extend", C.c_int32)]


class SwInput(C.Structure):
    _fields_ = [("n_pairs", C.c_uint64), ("ref_off", C.c_void_p), ("ref", C.c_void_p), ("alt_off", C.c_void_p),
                ("alt", C.c_void_p), ("strategy", C.c_void_p)]


class SwStats(C.Structure):
    _fields_ = [("n_pairs", C.c_uint64), ("cells", C.c_uint64), ("n_launches", C.c_uint32), ("ms_fill", C.c_float),
                ("ms_trace", C.c_float), ("backtrace_bytes", C.c_uint64), ("n_pairs_i16", C.c_uint64),
                ("n_pairs_strip", C.c_uint64), ("n_strips", C.c_uint64)]


SMITHWATERMAN_SYMBOLS = {
    "mgx_sw_create": (C.c_int, [C.c_int, C.c_uint, C.POINTER(C.c_void_p)]),
    "mgx_sw_destroy": (None, [C.c_void_p]),
    "mgx_sw_align_batch": (C.c_int, [C.c_void_p, C.POINTER(SwParams), C.POINTER(SwInput), C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "mgx_sw_align": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                               C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint8]),
    "mgx_sw_stats": (C.c_int, [C.c_void_p, C.POINTER(SwStats)]),
}
SYMBOLS.update(SMITHWATERMAN_SYMBOLS)


# ---- include/mgx_realign.h ------------------------------------------------------------------------
REALIGN_NOT_ALIGNED = -2 ** 31


class RealignStats(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("n_kept", C.c_uint64), ("n_verbatim", C.c_uint64), ("n_sw_pairs", C.c_uint64),
                ("ms_best", C.c_float), ("ms_verbatim", C.c_float), ("ms_gather", C.c_float)]


TO_REF_OK, TO_REF_DROPPED, TO_REF_UNCHANGED, TO_REF_THROWS, TO_REF_UNDEFINED, TO_REF_NO_ROOM = range(6)


class ToRefInput(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("read_off", C.c_void_p), ("read_bases", C.c_void_p), ("sw_offset", C.c_void_p),
                ("sw_cigar_off", C.c_void_p), ("sw_cigar", C.c_void_p), ("read_hap", C.c_void_p), ("n_haps", C.c_uint64),
                ("hap_cigar_off", C.c_void_p), ("hap_cigar", C.c_void_p), ("hap_start", C.c_void_p), ("read_ref", C.c_void_p),
                ("n_refs", C.c_uint64), ("ref_off", C.c_void_p), ("ref_bases", C.c_void_p), ("reference_start", C.c_void_p),
                ("hard_clips", C.c_void_p)]


class ToRefRegion(C.Structure):
    _fields_ = [("hap_cigar_off", C.c_void_p), ("hap_cigar", C.c_void_p), ("hap_start", C.c_void_p), ("ref_hap", C.c_uint32),
                ("reference_start", C.c_int32), ("hard_clips", C.c_void_p)]


class RealignToRefStats(C.Structure):
    _fields_ = [("n_status", C.c_uint64 * 6), ("ms_to_ref", C.c_float)]


REALIGN_SYMBOLS = {
    "mgx_read_to_ref": (C.c_int, [C.c_void_p, C.POINTER(ToRefInput), C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "mgx_realign_regions_to_ref": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(SwParams),
                                             C.c_uint8, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "mgx_realign_to_ref_stats": (C.c_int, [C.c_void_p, C.POINTER(RealignToRefStats)]),
    "mgx_pairhmm_best_alleles": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mgx_realign_regions": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(SwParams),
                                      C.c_uint8, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "mgx_realign_stats": (C.c_int, [C.c_void_p, C.POINTER(RealignStats)]),
}
SYMBOLS.update(REALIGN_SYMBOLS)


# ---- include/mgx_bgzf.h ---------------------------------------------------------------------------
class BgzfStats(C.Structure):
    _fields_ = [("n_blocks", C.c_uint64), ("bytes_in", C.c_uint64), ("bytes_out", C.c_uint64), ("n_stored", C.c_uint64),
                ("ms_kernels", C.c_float), ("ms_pack", C.c_float)]


BGZF_SYMBOLS = {
    "mgx_bgzf_create": (C.c_int, [C.c_int, C.c_uint, C.POINTER(C.c_void_p)]),
    "mgx_bgzf_destroy": (None, [C.c_void_p]),
    "mgx_bgzf_batch_create": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(C.c_void_p)]),
    "mgx_bgzf_batch_destroy": (None, [C.c_void_p, C.c_void_p]),
    "mgx_bgzf_batch_input": (C.c_void_p, [C.c_void_p]),
    "mgx_bgzf_batch_offsets": (C.c_void_p, [C.c_void_p]),
    "mgx_bgzf_batch_submit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    "mgx_bgzf_batch_wait": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "mgx_bgzf_bound": (C.c_uint64, [C.c_uint64, C.c_uint64]),
    "mgx_bgzf_compress": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p]),
    "mgx_bgzf_stats": (C.c_int, [C.c_void_p, C.POINTER(BgzfStats)]),
    "mgx_bgzf_prepare": (C.c_int, [C.c_void_p]),
    "mgx_bgzf_device_memory": (C.c_int, [C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "mgx_bgzf_store_reserve": (C.c_int, [C.c_void_p, C.c_uint64]),
    "mgx_bgzf_store_create": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "mgx_bgzf_store_destroy": (None, [C.c_void_p]),
    "mgx_bgzf_store_put": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "mgx_bgzf_store_emit": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}


class BgzfInflateStats(C.Structure):
    _fields_ = [("n_blocks", C.c_uint64), ("bytes_in", C.c_uint64), ("bytes_out", C.c_uint64), ("ms_kernel", C.c_float)]


BGZF_SYMBOLS.update({
    "mgx_bgzf_scan_blocks": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_int)]),
    "mgx_bgzf_inflate_batch_create": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.POINTER(C.c_void_p)]),
    "mgx_bgzf_inflate_batch_destroy": (None, [C.c_void_p, C.c_void_p]),
    "mgx_bgzf_inflate_batch_input": (C.c_void_p, [C.c_void_p]),
    "mgx_bgzf_inflate_batch_offsets": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "mgx_bgzf_inflate_batch_submit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    "mgx_bgzf_inflate_batch_wait": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "mgx_bgzf_decompress": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "mgx_bgzf_inflate_stats": (C.c_int, [C.c_void_p, C.POINTER(BgzfInflateStats)]),
})
BGZF_SINK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p)
SYMBOLS.update(BGZF_SYMBOLS)


# ---- include/mgx_bam.h ----------------------------------------------------------------------------
class BamKey(C.Structure):
    _fields_ = [("d5", C.c_int64), ("tid", C.c_int32), ("pos", C.c_int32), ("end", C.c_int32), ("flag", C.c_uint16), ("score", C.c_uint16),
                ("tile", C.c_uint16), ("x", C.c_uint16), ("y", C.c_uint16), ("same_qname", C.c_uint8), ("redo", C.c_uint8)]


class BamHeader(C.Structure):
    _fields_ = [("first", C.c_uint64), ("text_off", C.c_uint64), ("text_len", C.c_uint64), ("n_ref", C.c_uint32), ("pad_", C.c_uint32)]


class BamStats(C.Structure):
    _fields_ = [("n_tiles", C.c_uint64), ("n_tiles_rewalked", C.c_uint64), ("n_redo", C.c_uint64), ("n_rounds", C.c_uint32),
                ("ms_index", C.c_float), ("ms_keys", C.c_float)]


BAM_SYMBOLS = {
    "mgx_bam_parse_header": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(BamHeader), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mgx_bam_walk_host": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "mgx_bam_keys_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    "mgx_bam_keys_rules": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    "mgx_bam_keys_redo": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    "mgx_bam_pack_keys": (C.c_int, [C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]),
    "mgx_bam_batch_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_int32, C.POINTER(C.c_void_p)]),
    "mgx_bam_batch_destroy": (None, [C.c_void_p, C.c_void_p]),
    "mgx_bam_batch_input": (C.c_void_p, [C.c_void_p]),
    "mgx_bam_batch_submit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64]),
    "mgx_bam_batch_wait": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "mgx_bam_scan": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_int32, C.c_uint64, C.c_void_p, C.c_void_p,
                               C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "mgx_bam_stats": (C.c_int, [C.c_void_p, C.POINTER(BamStats)]),
}
SYMBOLS.update(BAM_SYMBOLS)


# ---- include/mgx_sam.h ----------------------------------------------------------------------------
class SamStats(C.Structure):
    _fields_ = [("n_lines", C.c_uint64), ("n_declined", C.c_uint64), ("bytes_in", C.c_uint64), ("bytes_out", C.c_uint64),
                ("n_tiles", C.c_uint64), ("ms_lines", C.c_float), ("ms_encode", C.c_float), ("ms_keys", C.c_float)]


_U64P = C.POINTER(C.c_uint64)
SAM_SYMBOLS = {
    "mgx_sam_table_create": (C.c_int, [C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "mgx_sam_table_destroy": (None, [C.c_void_p]),
    "mgx_sam_lines_host": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, _U64P]),
    "mgx_sam_encode_rules": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, _U64P, _U64P, _U64P]),
    "mgx_sam_encode_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, _U64P, _U64P, _U64P, _U64P]),
    "mgx_sam_batch_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_void_p)]),
    "mgx_sam_batch_destroy": (None, [C.c_void_p, C.c_void_p]),
    "mgx_sam_batch_input": (C.c_void_p, [C.c_void_p]),
    "mgx_sam_batch_submit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "mgx_sam_batch_wait": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                     C.POINTER(C.c_void_p), _U64P, _U64P, C.POINTER(C.c_void_p)]),
    "mgx_sam_batch_device_records": (C.c_uint64, [C.c_void_p]),
    "mgx_sam_encode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p, _U64P, _U64P, _U64P]),
    "mgx_sam_stats": (C.c_int, [C.c_void_p, C.POINTER(SamStats)]),
    "mgx_bgzf_store_put_device": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, _U64P]),
}
SYMBOLS.update(SAM_SYMBOLS)


# ---- include/mgx_activity.h -----------------------------------------------------------------------
class ActivityInput(C.Structure):
    _fields_ = [("interval_start", C.c_int32), ("n_loci", C.c_uint32), ("ref_bases", C.c_void_p), ("n_reads", C.c_uint64),
                ("read_start", C.c_void_p), ("cigar_off", C.c_void_p), ("cigar", C.c_void_p), ("base_off", C.c_void_p),
                ("bases", C.c_void_p), ("quals", C.c_void_p), ("flags", C.c_void_p), ("mate_start", C.c_void_p), ("sample", C.c_void_p),
                ("act_start", C.c_void_p), ("act_stop", C.c_void_p)]


class ActivityParams(C.Structure):
    _fields_ = [("has_normal", C.c_int32), ("genotype_germline_sites", C.c_int32), ("min_callable_depth", C.c_int32),
                ("pcr_error_qual", C.c_int32), ("min_base_quality", C.c_int32), ("flags", C.c_uint32), ("initial_log_odds", C.c_double)]


class ActivityStats(C.Structure):
    _fields_ = [("n_loci", C.c_uint64), ("n_elements", C.c_uint64), ("n_active", C.c_uint64), ("n_callable", C.c_uint64),
                ("n_launches", C.c_uint32), ("ms_elements", C.c_float), ("ms_locus", C.c_float)]


class ActivityRegionParams(C.Structure):
    _fields_ = [("max_prob_propagation", C.c_int32), ("padding", C.c_int32), ("min_region_size", C.c_int32), ("max_region_size", C.c_int32),
                ("max_filter_size", C.c_int32), ("adaptive_filter_size", C.c_int32), ("flags", C.c_uint32), ("n_band_weights", C.c_uint32),
                ("active_prob_threshold", C.c_double), ("sigma", C.c_double), ("band_weights", C.c_void_p)]


class ActivityRegionStats(C.Structure):
    _fields_ = [("n_states", C.c_uint64), ("n_runs", C.c_uint64), ("n_regions", C.c_uint64), ("n_launches", C.c_uint32),
                ("ms_band", C.c_float), ("ms_cut", C.c_float)]


ACTIVITY_SYMBOLS = {
    "mgx_activity_region_params_defaults": (None, [C.POINTER(ActivityRegionParams)]),
    "mgx_activity_band_weights": (C.c_int, [C.POINTER(ActivityRegionParams), C.c_void_p, C.c_uint32, C.POINTER(C.c_int32)]),
    "mgx_activity_profile_regions": (C.c_int, [C.c_void_p, C.c_int32, C.c_uint32, C.c_void_p, C.c_int64, C.POINTER(ActivityRegionParams), C.c_void_p,
                                               C.c_uint64, _U64P, C.c_void_p, C.c_uint64, _U64P]),
    "mgx_activity_interval_regions": (C.c_int, [C.c_void_p, C.POINTER(ActivityInput), C.POINTER(ActivityParams), C.c_int64, C.POINTER(ActivityRegionParams),
                                                C.c_void_p, C.c_uint64, _U64P, C.c_void_p, C.c_uint64, _U64P, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mgx_activity_region_stats": (C.c_int, [C.c_void_p, C.POINTER(ActivityRegionStats)]),
    "mgx_activity_create": (C.c_int, [C.c_int, C.c_uint32, C.POINTER(C.c_void_p)]),
    "mgx_activity_destroy": (None, [C.c_void_p]),
    "mgx_activity_params_defaults": (None, [C.POINTER(ActivityParams)]),
    "mgx_activity_interval": (C.c_int, [C.c_void_p, C.POINTER(ActivityInput), C.POINTER(ActivityParams), C.c_void_p, C.c_void_p, C.c_void_p]),
    "mgx_activity_stats": (C.c_int, [C.c_void_p, C.POINTER(ActivityStats)]),
    "mgx_activity_last_elements": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
}
SYMBOLS.update(ACTIVITY_SYMBOLS)
