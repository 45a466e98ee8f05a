"""ctypes binding of libfemhip.so (include/fem_hip.h).  One Device == one fem_dev handle == one GPU."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_HIP = None

#: every symbol include/fem_hip.h declares
ABI_SYMBOLS = [
    "fem_dev_open", "fem_dev_close", "fem_strerror", "fem_dev_last_error", "fem_dev_limits",
    "fem_dev_upload_index", "fem_dev_upload_reference", "fem_dev_build_index", "fem_dev_fetch_index",
    "fem_dev_map_batch_submit", "fem_dev_map_batch_wait",
    "fem_dev_stage_reads", "fem_dev_stage_info", "fem_dev_stage_front", "fem_dev_acquire_stage", "fem_dev_commit_stage", "fem_dev_commit_stage_uniform", "fem_dev_packed_layout", "fem_dev_commit_stage_packed", "fem_dev_map_staged", "fem_dev_sync", "fem_dev_fetch_stats", "fem_dev_fetch", "fem_dev_fetch_packed",
    "fem_dev_fetch_records", "fem_dev_seed_kernel", "fem_dev_index_info",
    "fem_dev_upload_reference_names", "fem_dev_acquire_text_stage", "fem_dev_commit_text_stage", "fem_dev_commit_names_stage", "fem_dev_sam_quals", "fem_dev_reserve_text", "fem_dev_reserve_batch", "fem_set_blocking_waits", "fem_dev_fetch_sam", "fem_dev_fetch_sam_nowait", "fem_dev_sam_wait",
    "fem_dev_set_timing", "fem_dev_reset_timing", "fem_dev_kernel_time", "fem_dev_copy_bandwidth",
    "fem_dev_h2d_bandwidth", "fem_dbg_live_bytes",
    "fem_device_numa", "fem_bind_thread_near_device",
    "fem_dev_allreduce_stats",
    "fem_dev_set_pairs", "fem_dev_fetch_pairs", "fem_dev_pair_count", "fem_dev_estimate_insert",
    "fem_dev_set_orientation", "fem_dev_estimate_library",
    "fem_dev_set_rescue", "fem_dev_rescue_count", "fem_dev_set_rescue_discordant", "fem_dev_rescue_discordant_count", "fem_dev_set_mapq",
    "fem_dev_set_unmapped", "fem_dev_unmapped_count",
    "fem_dev_set_report", "fem_dev_filtered_count", "fem_dev_set_tags", "fem_dev_set_mate_tags", "fem_dev_set_sam_seq",
    "fem_dev_set_xa", "fem_dev_xa_count",
    "fem_dev_set_trim", "fem_dev_fetch_trim", "fem_dev_trim_count",
    "fem_dev_set_adapter", "fem_dev_fetch_adapter", "fem_dev_adapter_count",
    "fem_dev_set_pair_overlap", "fem_dev_fetch_pair_overlap", "fem_dev_pair_overlap_count",
    "fem_dev_set_coverage", "fem_dev_coverage_layout", "fem_dev_fetch_coverage", "fem_dev_reset_coverage", "fem_dbg_stage_ms",
    "fem_dev_fetch_bam", "fem_dev_fetch_bam_nowait", "fem_dev_bam_wait", "fem_dev_bgzf_compress",
]


class FemError(RuntimeError):
    pass


class Params(C.Structure):
    """fem_params == FEMArgs of the reference (src/utils.h:63-70); map always uses k=12, step=3."""
    _fields_ = [("k", C.c_int32), ("step", C.c_int32), ("e", C.c_int32), ("a", C.c_int32)]


class _ReadBatch(C.Structure):
    _fields_ = [("bases", C.c_void_p), ("offsets", C.c_void_p), ("n_reads", C.c_uint64)]


class _BatchResult(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("n_candidates", C.c_uint64), ("cand_begin", C.c_void_p),
                ("cand_count", C.c_void_p), ("cand", C.c_void_p), ("ed", C.c_void_p), ("end", C.c_void_p),
                ("stats", C.c_uint64 * 5)]


class _BatchPacked(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("n_candidates", C.c_uint64), ("count", C.c_void_p), ("seg_begin", C.c_void_p),
                ("cand", C.c_void_p), ("ed", C.c_void_p), ("end", C.c_void_p), ("big", C.c_void_p), ("n_big", C.c_uint32),
                ("stats", C.c_uint64 * 5)]


class _BatchRecords(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("n_records", C.c_uint64), ("rec_begin", C.c_void_p), ("flag", C.c_void_p),
                ("tid", C.c_void_p), ("pos0", C.c_void_p), ("nm", C.c_void_p), ("cigar_off", C.c_void_p),
                ("cigar", C.c_void_p), ("md_off", C.c_void_p), ("md", C.c_void_p), ("stats", C.c_uint64 * 5)]


class _BatchSam(C.Structure):
    _fields_ = [("text", C.c_void_p), ("len", C.c_uint64), ("n_reads", C.c_uint64), ("n_records", C.c_uint64),
                ("n_asserted", C.c_uint64), ("stats", C.c_uint64 * 5)]


class _BatchBam(C.Structure):
    _fields_ = [("data", C.c_void_p), ("len", C.c_uint64), ("raw_len", C.c_uint64), ("n_blocks", C.c_uint64),
                ("n_records", C.c_uint64), ("n_asserted", C.c_uint64), ("stats", C.c_uint64 * 5)]


class _PairParams(C.Structure):
    _fields_ = [("min_insert", C.c_int32), ("max_insert", C.c_int32)]


class _InsertEstimate(C.Structure):
    _fields_ = [("n_pairs", C.c_uint64), ("n_unique", C.c_uint64), ("n_informative", C.c_uint64),
                ("q25", C.c_int32), ("q50", C.c_int32), ("q75", C.c_int32),
                ("min_insert", C.c_int32), ("max_insert", C.c_int32), ("estimated", C.c_int32)]


class _LibraryEstimate(C.Structure):
    _fields_ = [("by", _InsertEstimate * 3), ("orientation", C.c_int32)]


class _RescueParams(C.Structure):
    _fields_ = [("max_edits", C.c_int32)]


class _ReportParams(C.Structure):
    _fields_ = [("strata", C.c_int32), ("max_hits", C.c_int32)]


class _TrimParams(C.Structure):
    _fields_ = [("trim5", C.c_int32), ("trim3", C.c_int32), ("qual", C.c_int32)]


class _AdapterParams(C.Structure):
    _fields_ = [("seq1", C.c_char_p), ("seq2", C.c_char_p), ("min_overlap", C.c_int32), ("err_pct", C.c_int32)]


class _PairOverlapParams(C.Structure):
    _fields_ = [("min_overlap", C.c_int32), ("err_pct", C.c_int32)]


class _CoverageParams(C.Structure):
    _fields_ = [("window", C.c_int32), ("all_hits", C.c_int32), ("min_mapq", C.c_int32)]


#: fem_dbg_stage_ms stages (include/fem_hip.h)
STAGE_TEXT = 3
STAGE_COVERAGE = 12


class _TagParams(C.Structure):
    _fields_ = [("read_group", C.c_char_p), ("hit_tags", C.c_int32)]


class _BatchPairs(C.Structure):
    _fields_ = [("n_pairs", C.c_uint64), ("n_records", C.c_uint64), ("rec_begin", C.c_void_p), ("flag", C.c_void_p),
                ("tid", C.c_void_p), ("pos0", C.c_void_p), ("nm", C.c_void_p), ("cigar_off", C.c_void_p),
                ("cigar", C.c_void_p), ("md_off", C.c_void_p), ("md", C.c_void_p), ("mate_tid", C.c_void_p),
                ("mate_pos0", C.c_void_p), ("tlen", C.c_void_p), ("n_proper", C.c_uint64), ("stats", C.c_uint64 * 5)]


def hip_library_path():
    # FEM_HIP_LIBRARY: another build of the same library (ablation / tuning builds under gpurun_out/, measurement only)
    return os.environ.get("FEM_HIP_LIBRARY") or os.path.join(_HERE, "csrc", "libfemhip.so")


def load_hip():
    """Load libfemhip.so; raise loudly if it has not been built (no fallback of any kind)."""
    global _HIP
    if _HIP is not None:
        return _HIP
    path = hip_library_path()
    if not os.path.exists(path):
        raise FemError("libfemhip.so is missing (%s): run `python -c 'import __graft_entry__ as g; g.build()'` "
                       "or `make -C fem_amd/csrc`" % path)
    L = C.CDLL(path)
    vp, u64, i32 = C.c_void_p, C.c_uint64, C.c_int32
    L.fem_dev_open.argtypes = [C.c_int, C.POINTER(vp)]
    L.fem_dev_close.argtypes = [vp]
    L.fem_strerror.restype = C.c_char_p
    L.fem_strerror.argtypes = [C.c_int]
    L.fem_dev_last_error.restype = C.c_char_p
    L.fem_dev_last_error.argtypes = [vp]
    L.fem_dev_limits.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(i32)]
    L.fem_dev_upload_index.argtypes = [vp, i32, i32, vp, u64, vp, u64]
    L.fem_dev_upload_reference.argtypes = [vp, C.c_uint32, C.POINTER(vp), vp]
    L.fem_dev_build_index.argtypes = [vp, i32, i32, vp, vp, u64, C.POINTER(u64)]
    L.fem_dev_fetch_index.argtypes = [vp, vp, vp, u64]
    L.fem_dev_map_batch_submit.argtypes = [vp, C.c_int, C.POINTER(Params), C.POINTER(_ReadBatch)]
    L.fem_dev_map_batch_wait.argtypes = [vp, C.c_int, C.POINTER(_BatchResult)]
    L.fem_dev_stage_reads.argtypes = [vp, C.c_int, C.POINTER(_ReadBatch)]
    L.fem_dev_acquire_stage.argtypes = [vp, C.c_int, u64, u64, C.POINTER(vp), C.POINTER(vp)]
    L.fem_dev_commit_stage.argtypes = [vp, C.c_int, u64, C.c_uint32]
    L.fem_dev_commit_stage_uniform.argtypes = [vp, C.c_int, u64, C.c_uint32]
    L.fem_dev_packed_layout.argtypes = [u64, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(u64), C.POINTER(u64)]
    L.fem_dev_commit_stage_packed.argtypes = [vp, C.c_int, u64, C.c_uint32, u64]
    L.fem_dev_map_staged.argtypes = [vp, C.c_int, C.POINTER(Params)]
    L.fem_dev_sync.argtypes = [vp, C.c_int]
    L.fem_dev_fetch_stats.argtypes = [vp, C.c_int, vp]
    L.fem_dev_fetch.argtypes = [vp, C.c_int, C.POINTER(_BatchResult)]
    L.fem_dev_fetch_packed.argtypes = [vp, C.c_int, C.POINTER(_BatchPacked)]
    L.fem_dev_fetch_records.argtypes = [vp, C.c_int, C.POINTER(_BatchRecords)]
    L.fem_dev_index_info.argtypes = [vp, C.c_char_p, u64]
    L.fem_dev_seed_kernel.restype = C.c_char_p
    L.fem_dev_seed_kernel.argtypes = [vp, C.POINTER(Params)]
    L.fem_dev_set_timing.argtypes = [vp, C.c_int]
    L.fem_dev_reset_timing.argtypes = [vp]
    L.fem_dev_kernel_time.argtypes = [vp, C.c_int, C.POINTER(C.c_double), C.POINTER(u64)]
    L.fem_dev_copy_bandwidth.argtypes = [vp, u64, C.c_int, C.POINTER(C.c_double)]
    L.fem_dev_h2d_bandwidth.argtypes = [vp, u64, C.c_int, C.POINTER(C.c_double)]
    L.fem_dev_allreduce_stats.argtypes = [C.POINTER(vp), C.c_int, vp]
    L.fem_dev_upload_reference_names.argtypes = [vp, C.c_uint32, C.c_char_p, vp]
    L.fem_dev_acquire_text_stage.argtypes = [vp, C.c_int, u64, u64, u64, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.fem_dev_commit_text_stage.argtypes = [vp, C.c_int, u64, u64]
    if hasattr(L, "fem_dev_commit_names_stage"):
        L.fem_dev_commit_names_stage.argtypes = [vp, C.c_int, u64, u64]
        L.fem_dev_sam_quals.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(u64)]
    L.fem_dev_reserve_text.argtypes = [vp, C.c_int, u64, u64, u64, u64]
    if hasattr(L, "fem_dev_reserve_batch"):  # (FEM_HIP_LIBRARY may name an older build of the library: measurement only)
        L.fem_dev_reserve_batch.argtypes = [vp, C.c_int, u64, u64, C.c_uint32, C.POINTER(Params)]
    L.fem_dev_fetch_sam.argtypes = [vp, C.c_int, C.POINTER(_BatchSam)]
    L.fem_dev_fetch_sam_nowait.argtypes = [vp, C.c_int, C.POINTER(_BatchSam)]
    L.fem_dev_sam_wait.argtypes = [vp, C.c_int]
    L.fem_dev_stage_info.argtypes = [vp, C.c_int, C.POINTER(u64), C.POINTER(C.c_int32)]
    if hasattr(L, "fem_dev_stage_front"):
        L.fem_dev_stage_front.argtypes = [vp, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    if hasattr(L, "fem_dev_set_pairs"):
        L.fem_dev_set_pairs.argtypes = [vp, C.c_int, C.POINTER(_PairParams)]
        L.fem_dev_fetch_pairs.argtypes = [vp, C.c_int, C.POINTER(_BatchPairs)]
        L.fem_dev_pair_count.argtypes = [vp, C.c_int, C.POINTER(u64)]
    if hasattr(L, "fem_dev_estimate_insert"):
        L.fem_dev_estimate_insert.argtypes = [vp, C.c_int, C.POINTER(_InsertEstimate)]
    if hasattr(L, "fem_dev_set_orientation"):
        L.fem_dev_set_orientation.argtypes = [vp, C.c_int, C.c_int]
        L.fem_dev_estimate_library.argtypes = [vp, C.c_int, C.POINTER(_LibraryEstimate)]
    if hasattr(L, "fem_dev_set_rescue"):
        L.fem_dev_set_rescue.argtypes = [vp, C.c_int, C.POINTER(_RescueParams)]
        L.fem_dev_rescue_count.argtypes = [vp, C.c_int, C.POINTER(u64)]
    if hasattr(L, "fem_dev_set_rescue_discordant"):
        L.fem_dev_set_rescue_discordant.argtypes = [vp, C.c_int, C.c_int]
        L.fem_dev_rescue_discordant_count.argtypes = [vp, C.c_int, C.POINTER(u64)]
    if hasattr(L, "fem_dev_set_mapq"):
        L.fem_dev_set_mapq.argtypes = [vp, C.c_int, C.c_int]
    if hasattr(L, "fem_dev_set_unmapped"):
        L.fem_dev_set_unmapped.argtypes = [vp, C.c_int, C.c_int]
        L.fem_dev_unmapped_count.argtypes = [vp, C.c_int, C.POINTER(u64)]
    if hasattr(L, "fem_dev_set_report"):
        L.fem_dev_set_report.argtypes = [vp, C.c_int, C.POINTER(_ReportParams)]
        L.fem_dev_filtered_count.argtypes = [vp, C.c_int, C.POINTER(u64)]
    if hasattr(L, "fem_dev_set_tags"):
        L.fem_dev_set_tags.argtypes = [vp, C.c_int, C.POINTER(_TagParams)]
    if hasattr(L, "fem_dev_set_mate_tags"):
        L.fem_dev_set_mate_tags.argtypes = [vp, C.c_int, C.c_int]
    if hasattr(L, "fem_dev_set_sam_seq"):
        L.fem_dev_set_sam_seq.argtypes = [vp, C.c_int, C.c_int]
    if hasattr(L, "fem_dev_set_xa"):
        L.fem_dev_set_xa.argtypes = [vp, C.c_int, C.c_int32]
        L.fem_dev_xa_count.argtypes = [vp, C.c_int, C.POINTER(u64)]
    for name, params, n_arrays in (("trim", _TrimParams, 2), ("adapter", _AdapterParams, 1), ("pair_overlap", _PairOverlapParams, 1)):
        if hasattr(L, "fem_dev_set_" + name):
            getattr(L, "fem_dev_set_" + name).argtypes = [vp, C.c_int, C.POINTER(params)]
            getattr(L, "fem_dev_fetch_" + name).argtypes = [vp, C.c_int] + [C.POINTER(vp)] * n_arrays + [C.POINTER(u64)]
            getattr(L, "fem_dev_%s_count" % name).argtypes = [vp, C.c_int, C.POINTER(u64), C.POINTER(u64)]
    if hasattr(L, "fem_dev_fetch_bam"):
        L.fem_dev_fetch_bam.argtypes = [vp, C.c_int, C.c_int, C.POINTER(_BatchBam)]
        L.fem_dev_fetch_bam_nowait.argtypes = [vp, C.c_int, C.c_int, C.POINTER(_BatchBam)]
        L.fem_dev_bam_wait.argtypes = [vp, C.c_int]
        L.fem_dev_bgzf_compress.argtypes = [vp, vp, u64, C.c_int, vp, u64, C.POINTER(u64)]
    if hasattr(L, "fem_dev_set_coverage"):
        L.fem_dev_set_coverage.argtypes = [vp, C.POINTER(_CoverageParams)]
        L.fem_dev_coverage_layout.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
        L.fem_dev_fetch_coverage.argtypes = [vp, C.POINTER(u64), u64]
        L.fem_dev_reset_coverage.argtypes = [vp]
        L.fem_dbg_stage_ms.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_float)]
    if hasattr(L, "fem_dbg_live_bytes"):
        L.fem_dbg_live_bytes.argtypes = [C.POINTER(u64), C.POINTER(u64)]
    L.fem_device_numa.argtypes = [C.c_int, C.POINTER(C.c_int32), C.c_char_p, u64]
    L.fem_bind_thread_near_device.argtypes = [C.c_int]
    _HIP = L
    return L


def device_numa(device=0):
    """(NUMA node of the host memory next to GPU `device` or -1, that node's CPUs as a cpulist string)."""
    node = C.c_int32(-1)
    buf = C.create_string_buffer(4096)
    rc = load_hip().fem_device_numa(int(device), C.byref(node), buf, 4096)
    if rc != 0:
        raise FemError("fem_device_numa: %d" % rc)
    return node.value, buf.value.decode()


def bind_near_device(device=0):
    """Restricts the calling thread (and the threads it starts later) to the CPUs next to GPU `device`; True if bound."""
    return load_hip().fem_bind_thread_near_device(int(device)) == 0


def live_bytes():
    """fem_dbg_live_bytes: (device bytes, pinned host bytes) the library's buffers hold now, over all handles of the process."""
    dev, pin = C.c_uint64(), C.c_uint64()
    rc = load_hip().fem_dbg_live_bytes(C.byref(dev), C.byref(pin))
    if rc != 0:
        raise FemError("fem_dbg_live_bytes: %d" % rc)
    return dev.value, pin.value


def packed_layout(n_reads, read_len):
    """(bytes per read, offset of the exception positions behind the codes, most exceptions a packed batch may carry)
    of fem_dev_commit_stage_packed's staging layout."""
    bpr, off, cap = C.c_uint32(), C.c_uint64(), C.c_uint64()
    rc = load_hip().fem_dev_packed_layout(int(n_reads), int(read_len), C.byref(bpr), C.byref(off), C.byref(cap))
    if rc != 0:
        raise FemError("fem_dev_packed_layout: %d" % rc)
    return bpr.value, off.value, cap.value


def pack_reads(bases, n_reads, read_len, out):
    """numpy restatement of the packed form (tests): characters of n_reads reads of read_len -> codes + exceptions
    written into `out` (a staging view); returns the number of exceptions."""
    bpr, exc_off, exc_cap = packed_layout(n_reads, read_len)
    b = np.asarray(bases[:n_reads * read_len], dtype=np.uint8).reshape(n_reads, read_len)
    ok = (b == 65) | (b == 67) | (b == 71) | (b == 84)
    code = np.where(ok, ((b >> 1) ^ (b >> 2)) & 3, 0).astype(np.uint8)
    pad = bpr * 4 - read_len
    if pad:
        code = np.concatenate([code, np.zeros((n_reads, pad), np.uint8)], axis=1)
    q = code.reshape(n_reads, bpr, 4)
    out[:n_reads * bpr] = (q[:, :, 0] | (q[:, :, 1] << 2) | (q[:, :, 2] << 4) | (q[:, :, 3] << 6)).reshape(-1)
    out[n_reads * bpr:exc_off] = 0
    pos = np.flatnonzero(~ok.reshape(-1)).astype(np.uint32)
    n_exc = len(pos)
    if n_exc > exc_cap:
        raise FemError("too many exceptions for a packed batch")
    out[exc_off:exc_off + 4 * n_exc] = pos.view(np.uint8)
    out[exc_off + 4 * n_exc:exc_off + 5 * n_exc] = b.reshape(-1)[pos]
    return n_exc


def _copy(ptr, n, dtype, copy=True):
    n = int(n)
    if n == 0 or not ptr:
        return np.zeros(0, dtype=dtype)
    buf = (C.c_char * (n * np.dtype(dtype).itemsize)).from_address(ptr)
    a = np.frombuffer(buf, dtype=dtype, count=n)
    return a.copy() if copy else a


class BatchResult:
    """fem_batch_result: host copies of the arrays, or (copy=False) views of the handle's pinned result buffers,
    valid until the slot is staged or mapped again."""

    def __init__(self, r, copy=True):
        n2 = 2 * int(r.n_reads)
        nc = int(r.n_candidates)
        self.n_reads = int(r.n_reads)
        self.n_candidates = nc
        self.cand_begin = _copy(r.cand_begin, n2, np.uint32, copy)
        self.cand_count = _copy(r.cand_count, n2, np.uint32, copy)
        self.cand = _copy(r.cand, nc, np.uint64, copy)
        self.ed = _copy(r.ed, nc, np.uint8, copy)
        self.end = _copy(r.end, nc, np.int16, copy)
        self.stats = np.array(list(r.stats), dtype=np.uint64)

    def per_strand(self):
        """Candidates regrouped in (read, strand) order: offsets[2n+1], cand, ed, end — the layout the oracle uses."""
        cnt = self.cand_count.astype(np.int64)
        off = np.zeros(len(cnt) + 1, dtype=np.uint64)
        off[1:] = np.cumsum(cnt)
        total = int(off[-1])
        idx = np.zeros(total, dtype=np.int64)
        if total:
            starts = np.repeat(self.cand_begin.astype(np.int64) - off[:-1].astype(np.int64), cnt)
            idx = np.arange(total, dtype=np.int64) + starts
        return off, self.cand[idx], self.ed[idx], self.end[idx]


class BatchPacked:
    """fem_batch_packed (include/fem_hip.h): the outcome in the form that crosses the link — one byte per strand, one offset
    per 256 strands, the candidates without padding.  copy=False: views of the handle's pinned buffers."""

    def __init__(self, r, copy=True):
        n2 = 2 * int(r.n_reads)
        nc = int(r.n_candidates)
        self.n_reads = int(r.n_reads)
        self.n_candidates = nc
        self.count = _copy(r.count, n2, np.uint8, copy)
        self.seg_begin = _copy(r.seg_begin, (n2 + 255) // 256, np.uint32, copy)
        self.cand = _copy(r.cand, nc, np.uint64, copy)
        self.ed = _copy(r.ed, nc, np.uint8, copy)
        self.end = _copy(r.end, nc, np.int16, copy)
        self.n_big = int(r.n_big)
        self.big = _copy(r.big, 2 * self.n_big, np.uint32, True).reshape(-1, 2)
        self.stats = np.array(list(r.stats), dtype=np.uint64)
        self.d2h_bytes = n2 + 4 * len(self.seg_begin) + 11 * nc + 8 * self.n_big

    def counts(self):
        """Candidates per strand, the strands listed in big[] with their real counts."""
        cnt = self.count.astype(np.int64)
        for s_, c_ in self.big:
            cnt[int(s_)] = int(c_)
        return cnt

    def per_strand(self):
        """Candidates regrouped in (read, strand) order: offsets[2n+1], cand, ed, end — the layout the oracle uses."""
        cnt = self.counts()
        off = np.zeros(len(cnt) + 1, dtype=np.uint64)
        off[1:] = np.cumsum(cnt)
        total = int(off[-1])
        idx = np.zeros(total, dtype=np.int64)
        if total:
            n_seg = len(self.seg_begin)
            pad = np.zeros(n_seg * 256, dtype=np.int64)
            pad[:len(cnt)] = cnt
            within = np.cumsum(pad.reshape(n_seg, 256), axis=1) - pad.reshape(n_seg, 256)  # exclusive prefix inside a segment
            begin = (self.seg_begin.astype(np.int64)[:, None] + within).reshape(-1)[:len(cnt)]
            idx = np.arange(total, dtype=np.int64) + np.repeat(begin - off[:-1].astype(np.int64), cnt)
        return off, self.cand[idx], self.ed[idx], self.end[idx]


class BatchRecords:
    """Host copy of fem_batch_records: the batch's output records in the reference's order."""

    def __init__(self, r):
        n, nr = int(r.n_reads), int(r.n_records)
        self.n_reads, self.n_records = n, nr
        self.rec_begin = _copy(r.rec_begin, n + 1, np.uint32)
        self.flag = _copy(r.flag, nr, np.uint16)
        self.tid = _copy(r.tid, nr, np.uint32)
        self.pos0 = _copy(r.pos0, nr, np.uint32)
        self.nm = _copy(r.nm, nr, np.uint8)
        self.cigar_off = _copy(r.cigar_off, nr + 1, np.uint32)
        self.cigar = _copy(r.cigar, int(self.cigar_off[-1]) if nr + 1 else 0, np.uint32)
        self.md_off = _copy(r.md_off, nr + 1, np.uint32)
        self.md = _copy(r.md, int(self.md_off[-1]) if nr + 1 else 0, np.uint8)
        self.stats = np.array(list(r.stats), dtype=np.uint64)


class BatchPairs:
    """Host copy of fem_batch_pairs: the batch's records in paired output order, with the mate columns.  rec_begin[2 i + m]:
    first record of mate m of pair i."""

    def __init__(self, r):
        n_pairs, nr = int(r.n_pairs), int(r.n_records)
        self.n_pairs, self.n_records, self.n_proper = n_pairs, nr, int(r.n_proper)
        self.rec_begin = _copy(r.rec_begin, 2 * n_pairs + 1, np.uint32)
        self.flag = _copy(r.flag, nr, np.uint16)
        self.tid = _copy(r.tid, nr, np.uint32)
        self.pos0 = _copy(r.pos0, nr, np.uint32)
        self.nm = _copy(r.nm, nr, np.uint8)
        self.cigar_off = _copy(r.cigar_off, nr + 1, np.uint32)
        self.cigar = _copy(r.cigar, int(self.cigar_off[-1]), np.uint32)
        self.md_off = _copy(r.md_off, nr + 1, np.uint32)
        self.md = _copy(r.md, int(self.md_off[-1]), np.uint8)
        self.mate_tid = _copy(r.mate_tid, nr, np.uint32)
        self.mate_pos0 = _copy(r.mate_pos0, nr, np.uint32)
        self.tlen = _copy(r.tlen, nr, np.int32)
        self.stats = np.array(list(r.stats), dtype=np.uint64)


class InsertEstimate:
    """fem_insert_estimate: what a batch of read pairs says about the library's insert sizes (include/fem_hip.h: the rule)."""
    FIELDS = ("n_pairs", "n_unique", "n_informative", "q25", "q50", "q75", "min_insert", "max_insert", "estimated")

    def __init__(self, r):
        for f in self.FIELDS:
            setattr(self, f, int(getattr(r, f)))

    def as_tuple(self):
        return tuple(getattr(self, f) for f in self.FIELDS)

    def __repr__(self):
        return "InsertEstimate(%s)" % ", ".join("%s=%d" % (f, getattr(self, f)) for f in self.FIELDS)


ORIENTATIONS = ("fr", "rf", "ff")  # FEM_ORIENT_FR, _RF, _FF


class LibraryEstimate:
    """fem_library_estimate: the insert estimate under each orientation (.by: three InsertEstimate, FR RF FF) and the chosen
    orientation (.orientation: 0, 1, 2, or -1 when no orientation has enough informative pairs)."""

    def __init__(self, r):
        self.by = tuple(InsertEstimate(r.by[o]) for o in range(3))
        self.orientation = int(r.orientation)

    def __repr__(self):
        return "LibraryEstimate(orientation=%d, by=%r)" % (self.orientation, self.by)


class Device:
    """One GPU: resident index + reference, batches mapped through slots."""

    def __init__(self, device=0):
        self._L = load_hip()
        h = C.c_void_p()
        rc = self._L.fem_dev_open(device, C.byref(h))
        if rc != 0:
            raise FemError("fem_dev_open(%d) failed: %s — the HIP path needs a GPU, there is no CPU fallback"
                           % (device, self._L.fem_strerror(rc).decode()))
        self._h = h
        self._keep = []

    def close(self):
        if self._h:
            self._L.fem_dev_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise FemError("%s: %s" % (self._L.fem_strerror(rc).decode(),
                                       self._L.fem_dev_last_error(self._h).decode()))

    def limits(self):
        m, s = C.c_uint32(), C.c_int32()
        self._check(self._L.fem_dev_limits(self._h, C.byref(m), C.byref(s)))
        return m.value, s.value

    def upload_index(self, k, step, lookup, occ, n_occ=None):
        lookup = np.ascontiguousarray(lookup, dtype=np.uint32)
        occ = np.ascontiguousarray(occ, dtype=np.uint64)
        n_occ = len(occ) if n_occ is None else n_occ
        self._check(self._L.fem_dev_upload_index(self._h, k, step, lookup.ctypes.data, len(lookup), occ.ctypes.data,
                                                 n_occ))

    def upload_reference(self, seqs):
        """seqs: list of bytes / uint8 arrays (raw FASTA characters)."""
        arrs = [np.frombuffer(s, dtype=np.uint8) if isinstance(s, (bytes, bytearray)) else np.ascontiguousarray(s, np.uint8)
                for s in seqs]
        ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
        lens = np.array([len(a) for a in arrs], dtype=np.uint32)
        self._check(self._L.fem_dev_upload_reference(self._h, len(arrs), ptrs, lens.ctypes.data))
        self._n_seq = len(arrs)  # (coverage_layout sizes bin_off by it)

    def build_index(self, k=12, step=3, fetch=True):
        n = C.c_uint64()
        self._check(self._L.fem_dev_build_index(self._h, k, step, None, None, 0, C.byref(n)))
        if not fetch:
            return int(n.value), None, None
        lookup, occ = self.fetch_index(k, int(n.value))
        return int(n.value), lookup, occ

    def fetch_index(self, k, n_occ):
        """fem_dev_fetch_index: (lookup, occ) of the resident index, built or uploaded, whose k and size the caller knows."""
        lookup = np.zeros((1 << (2 * k)) + 1, dtype=np.uint32)
        occ = np.zeros(max(int(n_occ), 1), dtype=np.uint64)
        self._check(self._L.fem_dev_fetch_index(self._h, lookup.ctypes.data, occ.ctypes.data, len(occ)))
        return lookup, occ[:int(n_occ)]

    @staticmethod
    def _batch(bases, offsets):
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        return _ReadBatch(bases.ctypes.data, offsets.ctypes.data, len(offsets) - 1), (bases, offsets)

    def stage_reads(self, bases, offsets, slot=0):
        b, keep = self._batch(bases, offsets)
        self._check(self._L.fem_dev_stage_reads(self._h, slot, C.byref(b)))

    def stage_info(self, slot=0):
        """(bytes the slot's last staging sent over the link, True if as 2-bit codes)."""
        nb, pk = C.c_uint64(0), C.c_int32(0)
        self._check(self._L.fem_dev_stage_info(self._h, slot, C.byref(nb), C.byref(pk)))
        return nb.value, bool(pk.value)

    def stage_front(self, slot=0):
        """(True if the slot's last dense mapping selected its seeds from the 2-bit codes, True if the slot's batch has its
        characters in device memory)."""
        sp, cr = C.c_int32(0), C.c_int32(0)
        self._check(self._L.fem_dev_stage_front(self._h, slot, C.byref(sp), C.byref(cr)))
        return bool(sp.value), bool(cr.value)

    def acquire_stage(self, n_reads_cap, n_bases_cap, slot=0):
        """The slot's pinned staging buffers as numpy views (bases uint8[n_bases_cap + 64], offsets uint64[n_reads_cap + 1]):
        a parser (or a generator) writes the batch straight into them; commit_stage() then starts the H2D copy."""
        pb, po = C.c_void_p(), C.c_void_p()
        self._check(self._L.fem_dev_acquire_stage(self._h, slot, n_reads_cap, n_bases_cap, C.byref(pb), C.byref(po)))
        bases = np.frombuffer((C.c_char * (int(n_bases_cap) + 64)).from_address(pb.value), dtype=np.uint8)
        offs = np.frombuffer((C.c_char * (8 * (int(n_reads_cap) + 1))).from_address(po.value), dtype=np.uint64)
        return bases, offs

    def commit_stage(self, n_reads, max_len, slot=0, uniform=False):
        """uniform=True: every read has exactly max_len characters; the offsets are generated on the device."""
        if uniform:
            self._check(self._L.fem_dev_commit_stage_uniform(self._h, slot, n_reads, max_len))
        else:
            self._check(self._L.fem_dev_commit_stage(self._h, slot, n_reads, max_len))

    def commit_stage_packed(self, n_reads, read_len, n_exc=0, slot=0):
        """The slot's staging holds the batch at two bits per base + n_exc exceptions (packed_layout)."""
        self._check(self._L.fem_dev_commit_stage_packed(self._h, slot, n_reads, read_len, n_exc))

    def map_staged(self, e=3, a=1, k=12, step=3, slot=0):
        p = Params(k, step, e, a)
        self._check(self._L.fem_dev_map_staged(self._h, slot, C.byref(p)))

    def sync(self, slot=0):
        self._check(self._L.fem_dev_sync(self._h, slot))

    def fetch_stats(self, slot=0):
        st = np.zeros(5, dtype=np.uint64)
        self._check(self._L.fem_dev_fetch_stats(self._h, slot, st.ctypes.data))
        return st

    def fetch(self, slot=0, copy=True):
        r = _BatchResult()
        self._check(self._L.fem_dev_fetch(self._h, slot, C.byref(r)))
        return BatchResult(r, copy)

    def fetch_packed(self, slot=0, copy=True):
        """fem_dev_fetch_packed: the same outcome at a third of the bytes over the link."""
        r = _BatchPacked()
        self._check(self._L.fem_dev_fetch_packed(self._h, slot, C.byref(r)))
        return BatchPacked(r, copy)

    def seed_kernel(self, e=3, a=1, k=12, step=3):
        p = Params(k, step, e, a)
        return self._L.fem_dev_seed_kernel(self._h, C.byref(p)).decode()

    def index_info(self):
        """fem_dev_index_info: which derived tables the resident index has."""
        buf = C.create_string_buffer(512)
        self._check(self._L.fem_dev_index_info(self._h, buf, 512))
        return buf.value.decode()

    def reserve_batch(self, n_reads, n_records, max_len, e=3, a=1, k=12, step=3, slot=0):
        """fem_dev_reserve_batch: the slot's allocations for batches of this shape, made now."""
        p = Params(k, step, e, a)
        self._check(self._L.fem_dev_reserve_batch(self._h, slot, n_reads, n_records, max_len, C.byref(p)))

    def fetch_records(self, slot=0):
        """The device mapping tail: sorted records with CIGAR and MD (fem_dev_fetch_records)."""
        r = _BatchRecords()
        self._check(self._L.fem_dev_fetch_records(self._h, slot, C.byref(r)))
        return BatchRecords(r)

    def upload_reference_names(self, names):
        """names: list of str / bytes, one per reference sequence (the @SQ names)."""
        raw = [n.encode() if isinstance(n, str) else bytes(n) for n in names]
        off = np.zeros(len(raw) + 1, np.uint64)
        off[1:] = np.cumsum([len(n) for n in raw])
        self._check(self._L.fem_dev_upload_reference_names(self._h, len(raw), b"".join(raw), off.ctypes.data))

    def stage_text(self, quals, names, slot=0, quals_on_host=False):
        """Qualities (uint8 array / bytes, same offsets as the staged bases) and read names (list) of the slot's batch.
        quals_on_host: fem_dev_commit_names_stage — only the names go to the device, fetch_sam(quals=, offsets=) puts the
        qualities into the text."""
        raw = [n.encode() if isinstance(n, str) else bytes(n) for n in names]
        q = np.frombuffer(bytes(quals), np.uint8) if not isinstance(quals, np.ndarray) else quals
        nn = sum(len(n) for n in raw)
        pq, pn, po = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._check(self._L.fem_dev_acquire_text_stage(self._h, slot, len(raw), len(q), nn, C.byref(pq), C.byref(pn), C.byref(po)))
        if len(q):
            C.memmove(pq.value, q.ctypes.data, len(q))
        if nn:
            C.memmove(pn.value, b"".join(raw), nn)
        off = np.zeros(len(raw) + 1, np.uint64)
        off[1:] = np.cumsum([len(n) for n in raw])
        C.memmove(po.value, off.ctypes.data, 8 * (len(raw) + 1))
        if quals_on_host:
            self._check(self._L.fem_dev_commit_names_stage(self._h, slot, len(raw), nn))
        else:
            self._check(self._L.fem_dev_commit_text_stage(self._h, slot, len(raw), nn))

    def fetch_sam(self, slot=0, nowait=False, quals=None, offsets=None):
        """(SAM text of the slot's batch as bytes, n_records, n_asserted, stats) — rendered on the device.
        nowait: through fem_dev_fetch_sam_nowait + fem_dev_sam_wait."""
        r = _BatchSam()
        if nowait:
            self._check(self._L.fem_dev_fetch_sam_nowait(self._h, slot, C.byref(r)))
            self._check(self._L.fem_dev_sam_wait(self._h, slot))
        else:
            self._check(self._L.fem_dev_fetch_sam(self._h, slot, C.byref(r)))
        if quals is not None and r.len:  # the batch went without its qualities: into the fields the device left open
            from fem_amd import host
            qa, nq = C.c_void_p(), C.c_uint64()
            self._check(self._L.fem_dev_sam_quals(self._h, slot, C.byref(qa), C.byref(nq)))
            q = np.ascontiguousarray(quals, dtype=np.uint8)
            o = np.ascontiguousarray(offsets, dtype=np.uint64)
            rc = host.lib().fem_sam_fill_quals(r.text, r.len, qa.value, nq.value, q.ctypes.data, o.ctypes.data, 0, 3)
            if rc:
                raise FemError("fem_sam_fill_quals failed (%d)" % rc)
        text = C.string_at(r.text, r.len) if r.len else b""
        return text, int(r.n_records), int(r.n_asserted), np.array(list(r.stats), dtype=np.uint64)

    def fetch_bam(self, slot=0, level=1, nowait=False):
        """(BGZF members of the slot's batch as BAM records (bytes), raw_len, n_blocks, n_records, n_asserted, stats) — the
        lines of fetch_sam, encoded and compressed on the device.  nowait: through fem_dev_fetch_bam_nowait + fem_dev_bam_wait."""
        r = _BatchBam()
        if nowait:
            self._check(self._L.fem_dev_fetch_bam_nowait(self._h, slot, int(level), C.byref(r)))
            self._check(self._L.fem_dev_bam_wait(self._h, slot))
        else:
            self._check(self._L.fem_dev_fetch_bam(self._h, slot, int(level), C.byref(r)))
        data = C.string_at(r.data, r.len) if r.len else b""
        return (data, int(r.raw_len), int(r.n_blocks), int(r.n_records), int(r.n_asserted),
                np.array(list(r.stats), dtype=np.uint64))

    def bgzf_compress(self, data, level=1):
        """fem_dev_bgzf_compress: BGZF members (bytes, no EOF block) of `data`, compressed on the device."""
        raw = bytes(data)
        cap = 65536 * (len(raw) // 65280 + 1)
        out = C.create_string_buffer(cap)
        n = C.c_uint64()
        self._check(self._L.fem_dev_bgzf_compress(self._h, raw, len(raw), int(level), out, cap, C.byref(n)))
        return out.raw[:n.value]

    def set_pairs(self, min_insert=0, max_insert=500, slot=0):
        """fem_dev_set_pairs: the slot's batches are read pairs (read i and read n/2 + i); min_insert=None: single-end again."""
        if min_insert is None:
            self._check(self._L.fem_dev_set_pairs(self._h, slot, None))
        else:
            pp = _PairParams(int(min_insert), int(max_insert))
            self._check(self._L.fem_dev_set_pairs(self._h, slot, C.byref(pp)))

    def fetch_pairs(self, slot=0):
        """fem_dev_fetch_pairs: the records paired on the device, in output order (BatchPairs)."""
        r = _BatchPairs()
        self._check(self._L.fem_dev_fetch_pairs(self._h, slot, C.byref(r)))
        return BatchPairs(r)

    def estimate_insert(self, slot=0):
        """fem_dev_estimate_insert: the insert size range the slot's batch of read pairs suggests (InsertEstimate), from its
        unique pairs, on the device; the slot's options and later fetches are untouched."""
        r = _InsertEstimate()
        self._check(self._L.fem_dev_estimate_insert(self._h, slot, C.byref(r)))
        return InsertEstimate(r)

    def set_orientation(self, orientation, slot=0):
        """fem_dev_set_orientation: the library's orientation in pair mode: 0 / "fr" (the default), 1 / "rf", 2 / "ff"."""
        if isinstance(orientation, str):
            if orientation.lower() not in ORIENTATIONS:
                raise FemError("fem_dev_set_orientation: not one of fr, rf, ff: %r" % orientation)
            orientation = ORIENTATIONS.index(orientation.lower())
        self._check(self._L.fem_dev_set_orientation(self._h, slot, int(orientation)))

    def estimate_library(self, slot=0):
        """fem_dev_estimate_library: estimate_insert under the three orientations in one pass over the slot's batch, and the
        orientation with the most informative pairs (LibraryEstimate); the slot's options and later fetches are untouched."""
        r = _LibraryEstimate()
        self._check(self._L.fem_dev_estimate_library(self._h, slot, C.byref(r)))
        return LibraryEstimate(r)

    def pair_count(self, slot=0):
        """fem_dev_pair_count: proper pairs of the slot's last paired text."""
        n = C.c_uint64()
        self._check(self._L.fem_dev_pair_count(self._h, slot, C.byref(n)))
        return int(n.value)

    def set_rescue(self, max_edits=None, slot=0):
        """fem_dev_set_rescue: rescue the mate without records of a read pair at max_edits (0..15) edits; None: off."""
        if max_edits is None:
            self._check(self._L.fem_dev_set_rescue(self._h, slot, None))
        else:
            rp = _RescueParams(int(max_edits))
            self._check(self._L.fem_dev_set_rescue(self._h, slot, C.byref(rp)))

    def set_rescue_discordant(self, on=True, slot=0):
        """fem_dev_set_rescue_discordant: with pair mode and set_rescue, also rescue a mate of a pair whose records do not pair
        (both mates have records, no combination is concordant); False: only the mate without records, as before."""
        self._check(self._L.fem_dev_set_rescue_discordant(self._h, slot, 1 if on else 0))

    def set_mapq(self, on=True, slot=0):
        """fem_dev_set_mapq: MAPQ from the hit strata in the slot's SAM text and BAM records (False: 255, as the reference)."""
        self._check(self._L.fem_dev_set_mapq(self._h, slot, 1 if on else 0))

    def set_unmapped(self, on=True, slot=0):
        """fem_dev_set_unmapped: a line for every read without a mapping in the slot's SAM text and BAM records (False: none,
        as the reference)."""
        self._check(self._L.fem_dev_set_unmapped(self._h, slot, 1 if on else 0))

    def unmapped_count(self, slot=0):
        """fem_dev_unmapped_count: lines for unmapped reads in the slot's last SAM text or BAM."""
        n = C.c_uint64()
        self._check(self._L.fem_dev_unmapped_count(self._h, slot, C.byref(n)))
        return int(n.value)

    def set_report(self, strata=None, max_hits=None, slot=0):
        """fem_dev_set_report: the line filter of the slot's SAM text and BAM records: a read's (a mate's) lines within `strata`
        (0..15) edits of its best one, at most `max_hits` (>= 1) of them; None: that part off, both None: every line again."""
        if strata is None and max_hits is None:
            self._check(self._L.fem_dev_set_report(self._h, slot, None))
            return
        for v in (strata, max_hits):
            if v is not None and not -2 ** 31 <= int(v) < 2 ** 31:
                raise FemError("fem_dev_set_report: parameter out of range")
        rp = _ReportParams(-1 if strata is None else int(strata), -1 if max_hits is None else int(max_hits))
        self._check(self._L.fem_dev_set_report(self._h, slot, C.byref(rp)))

    def set_tags(self, slot=0, read_group=None, hits=False):
        """fem_dev_set_tags: RG:Z:<read_group> on every line of the slot's SAM text and BAM records (None: no RG tag), NH:i and
        HI:i on every mapped line (hits); neither: the lines as they are without tags."""
        if read_group is None and not hits:
            self._check(self._L.fem_dev_set_tags(self._h, slot, None))
            return
        rg = None if read_group is None else (read_group if isinstance(read_group, bytes) else read_group.encode("latin-1"))
        tp = _TagParams(rg, 1 if hits else 0)
        self._check(self._L.fem_dev_set_tags(self._h, slot, C.byref(tp)))

    def set_mate_tags(self, on=True, slot=0):
        """fem_dev_set_mate_tags: MC:Z, MQ:i and ms:i (the other mate's CIGAR, MAPQ and quality score) on every line of the slot's
        paired SAM text and BAM records (False: none); the qualities must be on the device then."""
        self._check(self._L.fem_dev_set_mate_tags(self._h, slot, 1 if on else 0))

    def set_sam_seq(self, on=True, slot=0):
        """fem_dev_set_sam_seq: SEQ reverse-complemented and QUAL reversed on the lines and BAM records of the slot's output whose
        FLAG has 0x10 and that carry them, as the SAM specification orders them (False: every read as sequenced, the reference's
        output); the qualities must be on the device then."""
        self._check(self._L.fem_dev_set_sam_seq(self._h, slot, 1 if on else 0))

    XA_ALL = 2**31 - 1  # set_xa: no entry limit, the byte budget (FEM_XA_MAX_BYTES) alone bounds a slot's folding

    def set_xa(self, max_entries=XA_ALL, slot=0):
        """fem_dev_set_xa: the secondary lines of every slot of the slot's SAM text and BAM records folded into an XA:Z field on the
        slot's primary line, at most max_entries of them and FEM_XA_MAX_BYTES bytes per line (0: off, a line per mapping)."""
        self._check(self._L.fem_dev_set_xa(self._h, slot, max_entries))

    def xa_count(self, slot=0):
        """fem_dev_xa_count: lines folded into XA:Z entries in the slot's last SAM text or BAM."""
        n = C.c_uint64()
        self._check(self._L.fem_dev_xa_count(self._h, slot, C.byref(n)))
        return int(n.value)

    def set_coverage(self, window=1000, all_hits=False, min_mapq=0):
        """fem_dev_set_coverage: the handle keeps a coverage track of windows of `window` bases from now on, which the first text
        or BAM fetch of every mapped batch adds to; window=None: off.  Setting it again zeroes the track."""
        if window is None:
            return self._check(self._L.fem_dev_set_coverage(self._h, None))
        cp = _CoverageParams(int(window), int(all_hits), int(min_mapq))
        self._check(self._L.fem_dev_set_coverage(self._h, C.byref(cp)))

    def coverage_layout(self):
        """fem_dev_coverage_layout: (n_bins, bin_off with n_seq + 1 entries)."""
        n = C.c_uint64()
        self._check(self._L.fem_dev_coverage_layout(self._h, C.byref(n), None))
        off = np.zeros(self._n_seq + 1, np.uint64)
        self._check(self._L.fem_dev_coverage_layout(self._h, C.byref(n), off.ctypes.data_as(C.POINTER(C.c_uint64))))
        return int(n.value), off

    def fetch_coverage(self, cap=None):
        """fem_dev_fetch_coverage: the track's bins (uint64), after everything the slots have queued; cap: the room offered."""
        n = C.c_uint64()
        self._check(self._L.fem_dev_coverage_layout(self._h, C.byref(n), None))
        cap = int(n.value) if cap is None else int(cap)
        bins = np.zeros(max(cap, 1), np.uint64)
        self._check(self._L.fem_dev_fetch_coverage(self._h, bins.ctypes.data_as(C.POINTER(C.c_uint64)), cap))
        return bins[: int(n.value)]

    def reset_coverage(self):
        self._check(self._L.fem_dev_reset_coverage(self._h))

    def stage_ms(self, stage, slot=0):
        """fem_dbg_stage_ms: device time of one stage of the slot's last fetch (STAGE_TEXT, STAGE_COVERAGE); negative: it did not run."""
        ms = C.c_float()
        self._check(self._L.fem_dbg_stage_ms(self._h, slot, int(stage), C.byref(ms)))
        return float(ms.value)

    def _fetch_cuts(self, fn, slot, n_arrays=1):
        """A cut producer's fetch (fem_dev_fetch_trim, _adapter, _pair_overlap): its uint16 arrays, read for read."""
        ptrs, n = [C.c_void_p() for _ in range(n_arrays)], C.c_uint64()
        self._check(fn(self._h, slot, *[C.byref(p) for p in ptrs], C.byref(n)))
        return [_copy(p.value, n.value, np.uint16) for p in ptrs]

    def _cut_counts(self, fn, slot):
        """A cut producer's two counters (fem_dev_trim_count, _adapter_count, _pair_overlap_count)."""
        n_cut, n_bases = C.c_uint64(), C.c_uint64()
        self._check(fn(self._h, slot, C.byref(n_cut), C.byref(n_bases)))
        return int(n_cut.value), int(n_bases.value)

    def set_trim(self, trim5=0, trim3=0, qual=0, slot=0):
        """fem_dev_set_trim: the slot's batches are trimmed on the device from the next fem_dev_map_staged on: trim5 / trim3 bases
        (0..1024) off the reads' ends, the 3' end by quality at qual (1..93; 0: off); all 0: off.  The SAM text and BAM records
        print the clipped bases as soft clips."""
        tp = _TrimParams(int(trim5), int(trim3), int(qual))
        self._check(self._L.fem_dev_set_trim(self._h, slot, C.byref(tp)))

    def fetch_trim(self, slot=0):
        """fem_dev_fetch_trim: (clip5, clip3) of the slot's trimmed batch, read for read (uint16 arrays)."""
        return tuple(self._fetch_cuts(self._L.fem_dev_fetch_trim, slot, 2))

    def trim_count(self, slot=0):
        """fem_dev_trim_count: (reads the slot's batch had trimmed, bases trimmed off them)."""
        return self._cut_counts(self._L.fem_dev_trim_count, slot)

    def set_adapter(self, seq1=None, seq2=None, min_overlap=5, err_pct=10, slot=0):
        """fem_dev_set_adapter: the slot's batches have the 3' adapter seq1 (mate 2 in pair mode: seq2, default seq1; 4..64 letters
        of ACGT) matched and cut on the device from the next fem_dev_map_staged on, at an overlap of min_overlap bases at the least
        and err_pct (0..30) per cent of mismatches at the most; seq1 None: off.  The cut bases are printed as soft clips."""
        if seq1 is None:
            self._check(self._L.fem_dev_set_adapter(self._h, slot, None))
            return
        enc = lambda x: x.encode("latin-1") if isinstance(x, str) else x  # noqa: E731
        ap = _AdapterParams(enc(seq1), enc(seq2), int(min_overlap), int(err_pct))
        self._check(self._L.fem_dev_set_adapter(self._h, slot, C.byref(ap)))

    def fetch_adapter(self, slot=0):
        """fem_dev_fetch_adapter: the adapter cuts a3 of the slot's batch, read for read (a uint16 array)."""
        return self._fetch_cuts(self._L.fem_dev_fetch_adapter, slot)[0]

    def adapter_count(self, slot=0):
        """fem_dev_adapter_count: (reads of the slot's batch with an adapter cut, bases cut off them)."""
        return self._cut_counts(self._L.fem_dev_adapter_count, slot)

    def set_pair_overlap(self, min_overlap=20, err_pct=10, slot=0):
        """fem_dev_set_pair_overlap: in pair mode the slot's batches have the read-through of both mates found from their overlap
        and cut on the device from the next fem_dev_map_staged on: the largest fragment length at which mate 1 is the reverse
        complement of mate 2 over min_overlap (8..1024) bases at the least with err_pct (0..30) per cent of mismatches at the most;
        min_overlap None: off.  The cut bases are printed as soft clips."""
        if min_overlap is None:
            self._check(self._L.fem_dev_set_pair_overlap(self._h, slot, None))
            return
        vp = _PairOverlapParams(int(min_overlap), int(err_pct))
        self._check(self._L.fem_dev_set_pair_overlap(self._h, slot, C.byref(vp)))

    def fetch_pair_overlap(self, slot=0):
        """fem_dev_fetch_pair_overlap: the overlap cuts v3 of the slot's batch, read for read (a uint16 array)."""
        return self._fetch_cuts(self._L.fem_dev_fetch_pair_overlap, slot)[0]

    def pair_overlap_count(self, slot=0):
        """fem_dev_pair_overlap_count: (pairs of the slot's batch with an overlap cut, bases cut off both mates)."""
        return self._cut_counts(self._L.fem_dev_pair_overlap_count, slot)

    def filtered_count(self, slot=0):
        """fem_dev_filtered_count: lines the filter left out of the slot's last SAM text or BAM."""
        n = C.c_uint64()
        self._check(self._L.fem_dev_filtered_count(self._h, slot, C.byref(n)))
        return int(n.value)

    def rescue_count(self, slot=0):
        """fem_dev_rescue_count: rescued mates of the slot's last paired text (or fetch_pairs)."""
        n = C.c_uint64()
        self._check(self._L.fem_dev_rescue_count(self._h, slot, C.byref(n)))
        return int(n.value)

    def rescue_discordant_count(self, slot=0):
        """fem_dev_rescue_discordant_count: the rescued records of pairs whose records did not pair among rescue_count's."""
        n = C.c_uint64()
        self._check(self._L.fem_dev_rescue_discordant_count(self._h, slot, C.byref(n)))
        return int(n.value)

    def map_batch(self, bases, offsets, e=3, a=1, k=12, step=3, slot=0):
        b, keep = self._batch(bases, offsets)
        p = Params(k, step, e, a)
        self._check(self._L.fem_dev_map_batch_submit(self._h, slot, C.byref(p), C.byref(b)))
        r = _BatchResult()
        self._check(self._L.fem_dev_map_batch_wait(self._h, slot, C.byref(r)))
        return BatchResult(r)

    def set_timing(self, on=True):
        self._check(self._L.fem_dev_set_timing(self._h, int(on)))

    def reset_timing(self):
        self._check(self._L.fem_dev_reset_timing(self._h))

    def kernel_time(self, kernel):
        ms, n = C.c_double(), C.c_uint64()
        self._check(self._L.fem_dev_kernel_time(self._h, kernel, C.byref(ms), C.byref(n)))
        return ms.value, int(n.value)

    def h2d_bandwidth(self, nbytes=1 << 28, iters=8):
        g = C.c_double()
        self._check(self._L.fem_dev_h2d_bandwidth(self._h, nbytes, iters, C.byref(g)))
        return g.value

    def copy_bandwidth(self, nbytes=1 << 30, iters=10):
        g = C.c_double()
        self._check(self._L.fem_dev_copy_bandwidth(self._h, nbytes, iters, C.byref(g)))
        return g.value
