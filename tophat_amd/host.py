"""ctypes binding of the C ABI in include/thj.h (libthj_hip.so).

Host-side mirror used by bench.py, the tests and smoke(); the drop-in C++
binaries call the same ABI directly.  There is no fallback: if the HIP library
is missing or a call fails, an exception is raised.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .batch import Events, HIT_DTYPE, JUNC_DTYPE, SegBatch
from .params import CParams, Params

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "csrc", "libthj_hip.so")

INS_CODE = "ACGTN"

FUSION_DTYPE = np.dtype([("ref_id1", "<u4"), ("ref_id2", "<u4"), ("left", "<u4"), ("right", "<u4"), ("dir", "<u4"),
                         ("count", "<u4"), ("edit_dist", "<u4"), ("skip", "<u4")])


class ThjError(RuntimeError):
    pass


class CSegBatch(C.Structure):
    _fields_ = [("n_reads", C.c_int32), ("nseg", C.c_int32), ("words_per_plane", C.c_int32), ("reserved", C.c_int32),
                ("seg_off", C.c_void_p), ("hits", C.c_void_p), ("read_planes", C.c_void_p), ("read_len", C.c_void_p),
                ("mate_off", C.c_void_p), ("mate_hits", C.c_void_p), ("ordinal_base", C.c_uint32),
                ("reserved2", C.c_uint32)]


class CJunction(C.Structure):
    _fields_ = [("ref_id", C.c_uint32), ("left", C.c_uint32), ("right", C.c_uint32), ("antisense", C.c_uint32)]


class CInsertion(C.Structure):
    _fields_ = [("ref_id", C.c_uint32), ("left", C.c_uint32), ("seq", C.c_char * 8), ("prio", C.c_uint64)]


class CCounts(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("n_juncs", "n_deletions", "n_insertions", "n_windows", "n_indel_pairs",
                                         "n_rescue_pairs", "n_overflow_blocks", "n_hits_read")]


ABI_VERSION = 2
ABI_SYMBOLS = [
    "thj_params_default", "thj_last_error", "thj_version", "thj_abi_version", "thj_ctx_stream_info", "thj_ctx_probe_streams",
    "thj_device_count", "thj_ctx_create", "thj_ctx_destroy", "thj_ctx_sync", "thj_ctx_stream",
    "thj_genome_layout", "thj_genome_pack", "thj_genome_upload", "thj_genome_adopt",
    "thj_reads_pack",
    "thj_batch_upload", "thj_batch_free",
    "thj_segjuncs_configure", "thj_segjuncs_reset_async", "thj_segjuncs_run_async", "thj_segjuncs_run_pair_async",
    "thj_segjuncs_finish", "thj_segjuncs_download", "thj_segjuncs_device_keys",
    "thj_segjuncs_merge_keys_async", "thj_profile_segjuncs", "thj_profile_serial",
    "thj_segjuncs_device_insertions", "thj_segjuncs_merge_insertions_async",
    "thj_fusion_reset_async", "thj_fusion_set_ignored", "thj_fusion_run_async", "thj_genome_gather", "thj_fusion_finish", "thj_fusion_download",
    "thj_covsearch_reset_async", "thj_covsearch_add_hits_async", "thj_covsearch_add_reads", "thj_covsearch_run_async", "thj_covsearch_finish",
    "thj_covsearch_device_state", "thj_covsearch_merge_async", "thj_span_hit_heads_async",
    "thj_comm_unique_id", "thj_comm_create", "thj_comm_create_local", "thj_comm_destroy", "thj_comm_info",
    "thj_events_allgather_async", "thj_fusion_allgather", "thj_covsearch_allgather", "thj_span_fusions_upload", "thj_md_string2", "thj_ingest_span_batch", "thj_ingest_timing_report", "thj_pinned_alloc", "thj_pinned_free", "thj_pinned_drain", "thj_ctx_warm",
]

_lib = None


def load_lib(path: Optional[str] = None):
    """Loads libthj_hip.so; raises ThjError if it is not built (run __graft_entry__.build())."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise ThjError("HIP extension %s not built; run `python -c 'import __graft_entry__ as g; g.build()'`" % p)
    lib = C.CDLL(p)
    lib.thj_last_error.restype = C.c_char_p
    lib.thj_version.restype = C.c_char_p
    # the argument layouts this module was written against (include/thj.h: THJ_ABI_VERSION)
    if not hasattr(lib, "thj_abi_version") or lib.thj_abi_version() != ABI_VERSION:
        raise ThjError("%s has ABI revision %s, this module wants %d: rebuild (python -c 'import __graft_entry__ as g; g.build()')" % (
            p, lib.thj_abi_version() if hasattr(lib, "thj_abi_version") else "< 2", ABI_VERSION))
    if hasattr(lib, "thj_ctx_stream"):
        lib.thj_ctx_stream.restype = C.c_void_p
    if path is None:
        _lib = lib
    return lib


def _check(lib, rc: int, what: str):
    if rc != 0:
        raise ThjError("%s failed (%d): %s" % (what, rc, lib.thj_last_error().decode()))


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else C.c_void_p(a.ctypes.data)


class PackedGenome:
    def __init__(self, blocks: np.ndarray, contig_blk: np.ndarray, lens: np.ndarray):
        self.blocks, self.contig_blk, self.lens = blocks, contig_blk, lens

    @property
    def n_blocks(self) -> int:
        return self.blocks.shape[0] // 4

    @property
    def n_contigs(self) -> int:
        return self.lens.shape[0]

    def decode_gpos(self, gpos: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """global base coordinate -> (ref_id 1-based, pos)"""
        starts = self.contig_blk[:-1].astype(np.int64) * 64
        idx = np.searchsorted(starts, gpos, side="right") - 1
        return (idx + 1).astype(np.uint32), (gpos - starts[idx]).astype(np.int64)


def pack_genome(seqs: Sequence[Optional[str]], lib=None) -> PackedGenome:
    lib = lib or load_lib()
    n = len(seqs)
    lens = np.array([0 if s is None else len(s) for s in seqs], dtype=np.int64)
    contig_blk = np.zeros(n + 1, dtype=np.uint32)
    nb = C.c_int64()
    _check(lib, lib.thj_genome_layout(n, _ptr(lens), _ptr(contig_blk), C.byref(nb)), "thj_genome_layout")
    blocks = np.zeros(nb.value * 4, dtype=np.uint64)
    bufs = [None if s is None else s.encode() for s in seqs]
    arr = (C.c_char_p * n)(*bufs)
    _check(lib, lib.thj_genome_pack(n, arr, _ptr(lens), _ptr(contig_blk), _ptr(blocks), nb), "thj_genome_pack")
    pg = PackedGenome(blocks, contig_blk, lens)
    pg.seqs = list(seqs)            # the host keeps the bases: MD strings the device leaves to it are rebuilt from them
    return pg


def words_per_plane(max_len: int) -> int:
    return max(1, (int(max_len) + 63) // 64)


def pack_reads(b: SegBatch, W: Optional[int] = None, lib=None) -> Tuple[np.ndarray, np.ndarray, int]:
    lib = lib or load_lib()
    n = b.n_reads
    lens_ = np.diff(b.read_off) if n else np.zeros(0, dtype=np.int64)
    if W is None:
        W = words_per_plane(int(lens_.max()) if n else 1)
    planes = np.zeros(n * 3 * W, dtype=np.uint64)
    lens = np.zeros(n, dtype=np.uint16)
    bases = np.ascontiguousarray(b.bases, dtype=np.uint8)
    off = np.ascontiguousarray(b.read_off, dtype=np.int64)
    _check(lib, lib.thj_reads_pack(C.c_int64(n), _ptr(off), _ptr(bases), W, _ptr(planes), _ptr(lens)), "thj_reads_pack")
    return planes, lens, W


def host_cbatch(b: SegBatch, ordinal_base: int = 0, lib=None):
    """CSegBatch whose pointers are HOST numpy arrays (+ the arrays, to keep them alive)."""
    planes, lens, W = pack_reads(b, lib=lib)
    keep = [np.ascontiguousarray(b.seg_off, dtype=np.uint32), np.ascontiguousarray(b.hits), planes, lens]
    cb = CSegBatch()
    cb.n_reads, cb.nseg, cb.words_per_plane = b.n_reads, b.nseg, W
    cb.seg_off, cb.hits, cb.read_planes, cb.read_len = [a.ctypes.data for a in keep]
    if b.mate_off is not None:
        keep += [np.ascontiguousarray(b.mate_off, dtype=np.uint32), np.ascontiguousarray(b.mate_hits)]
        cb.mate_off = keep[-2].ctypes.data
        cb.mate_hits = keep[-1].ctypes.data if len(keep[-1]) else keep[-2].ctypes.data
    cb.ordinal_base = ordinal_base
    n_mate = 0 if b.mate_hits is None else len(b.mate_hits)
    return cb, keep, len(b.hits), n_mate


COMM_ID_BYTES = 128
COMM_TRANSPORT = {0: "self", 1: "rccl", 2: "loopback"}


def comm_unique_id(lib=None) -> bytes:
    """ncclGetUniqueId through the C ABI: made by one rank, handed to the others by the caller."""
    lib = lib or load_lib()
    buf = (C.c_uint8 * COMM_ID_BYTES)()
    _check(lib, lib.thj_comm_unique_id(buf), "thj_comm_unique_id")
    return bytes(buf)


class Comm:
    """One rank of the exchange step (thj_comm): bound to one Context."""

    def __init__(self, ctx: "Context", handle: C.c_void_p):
        self.ctx, self._h = ctx, handle

    @staticmethod
    def create(ctx: "Context", unique_id: Optional[bytes], n_ranks: int, rank: int) -> "Comm":
        h = C.c_void_p()
        idbuf = (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(unique_id) if unique_id is not None else None
        _check(ctx.lib, ctx.lib.thj_comm_create(ctx._ctx, idbuf, n_ranks, rank, C.byref(h)), "thj_comm_create")
        return Comm(ctx, h)

    @staticmethod
    def create_local(ctxs: Sequence["Context"]) -> List["Comm"]:
        n = len(ctxs)
        arr = (C.c_void_p * n)(*[c._ctx for c in ctxs])
        out = (C.c_void_p * n)()
        _check(ctxs[0].lib, ctxs[0].lib.thj_comm_create_local(arr, n, out), "thj_comm_create_local")
        return [Comm(ctxs[i], C.c_void_p(out[i])) for i in range(n)]

    def info(self):
        n, r, t = C.c_int32(), C.c_int32(), C.c_int32()
        st = (C.c_int64 * 4)()
        _check(self.ctx.lib, self.ctx.lib.thj_comm_info(self._h, C.byref(n), C.byref(r), C.byref(t), st), "thj_comm_info")
        return {"n_ranks": n.value, "rank": r.value, "transport": COMM_TRANSPORT[t.value], "steps": st[0], "repeats": st[1],
                "bytes_per_rank": st[2], "junction_capacity": st[3]}

    def events_allgather(self):
        _check(self.ctx.lib, self.ctx.lib.thj_events_allgather_async(self.ctx._ctx, self._h), "thj_events_allgather_async")

    def fusion_allgather(self) -> np.ndarray:
        """after Context.fusions(...) on every rank: the merged FusionSimpleSet (FUSION_DTYPE array), same on every rank"""
        n = C.c_int64()
        _check(self.ctx.lib, self.ctx.lib.thj_fusion_allgather(self.ctx._ctx, self._h, C.byref(n)), "thj_fusion_allgather")
        out = np.zeros(max(1, n.value), dtype=FUSION_DTYPE)
        _check(self.ctx.lib, self.ctx.lib.thj_fusion_download(self.ctx._ctx, _ptr(out)), "thj_fusion_download")
        return out[:n.value]

    def covsearch_allgather(self):
        _check(self.ctx.lib, self.ctx.lib.thj_covsearch_allgather(self.ctx._ctx, self._h), "thj_covsearch_allgather")

    def close(self):
        if self._h:
            self.ctx.lib.thj_comm_destroy(self._h)
            self._h = C.c_void_p()


def decode_ins_seq(code: int, length: int) -> str:
    return "".join(INS_CODE[(code >> (3 * k)) & 7] for k in range(length))


class Context:
    """One (host thread, device) context: resident genome, event tables, stream."""

    def __init__(self, device: int = 0, stream: Optional[int] = None):
        self.lib = load_lib()
        self._ctx = C.c_void_p()
        _check(self.lib, self.lib.thj_ctx_create(device, C.c_void_p(stream) if stream else None, C.byref(self._ctx)),
               "thj_ctx_create")
        self.genome: Optional[PackedGenome] = None
        self._batches: List[C.c_void_p] = []

    def close(self):
        if self._ctx:
            for b in self._batches:
                self.lib.thj_batch_free(self._ctx, b)
            self._batches = []
            self.lib.thj_ctx_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def sync(self):
        _check(self.lib, self.lib.thj_ctx_sync(self._ctx), "thj_ctx_sync")

    def upload_genome(self, g: PackedGenome):
        _check(self.lib, self.lib.thj_genome_upload(self._ctx, _ptr(g.blocks), C.c_int64(g.n_blocks), _ptr(g.contig_blk),
                                                    _ptr(g.lens), g.n_contigs), "thj_genome_upload")
        self.genome = g
        self.host_seqs = getattr(g, "seqs", None)

    def adopt_genome(self, d_blocks: int, g: PackedGenome):
        _check(self.lib, self.lib.thj_genome_adopt(self._ctx, C.c_void_p(d_blocks), C.c_int64(g.n_blocks),
                                                   _ptr(g.contig_blk), _ptr(g.lens), g.n_contigs), "thj_genome_adopt")
        self.genome = g

    def upload_batch(self, b: SegBatch, ordinal_base: int = 0) -> C.c_void_p:
        cb, keep, nh, nm = host_cbatch(b, ordinal_base, self.lib)
        out = C.c_void_p()
        _check(self.lib, self.lib.thj_batch_upload(self._ctx, C.byref(cb), C.c_int64(nh), C.c_int64(nm), C.byref(out)),
               "thj_batch_upload")
        self.sync()
        self._batches.append(out)
        return out

    def free_batch(self, h: C.c_void_p):
        self._batches = [b for b in self._batches if b.value != h.value]
        _check(self.lib, self.lib.thj_batch_free(self._ctx, h), "thj_batch_free")

    def configure(self, junc_capacity: int, indel_capacity: int):
        _check(self.lib, self.lib.thj_segjuncs_configure(self._ctx, C.c_int64(junc_capacity), C.c_int64(indel_capacity)),
               "thj_segjuncs_configure")

    def reset(self):
        _check(self.lib, self.lib.thj_segjuncs_reset_async(self._ctx), "thj_segjuncs_reset_async")

    def run(self, p: Params, batch):
        """batch: handle from upload_batch, or a CSegBatch of DEVICE pointers."""
        cp = p.as_ctypes()
        arg = C.byref(batch) if isinstance(batch, CSegBatch) else batch
        _check(self.lib, self.lib.thj_segjuncs_run_async(self._ctx, C.byref(cp), arg), "thj_segjuncs_run_async")

    def run_pair(self, p0: Params, batch0, p1: Params, batch1):
        """two batches (the two sides of a pass) as one call: see thj_segjuncs_run_pair_async"""
        c0, c1 = p0.as_ctypes(), p1.as_ctypes()
        a0 = C.byref(batch0) if isinstance(batch0, CSegBatch) else batch0
        a1 = C.byref(batch1) if isinstance(batch1, CSegBatch) else batch1
        _check(self.lib, self.lib.thj_segjuncs_run_pair_async(self._ctx, C.byref(c0), a0, C.byref(c1), a1), "thj_segjuncs_run_pair_async")

    def finish(self) -> CCounts:
        cnt = CCounts()
        _check(self.lib, self.lib.thj_segjuncs_finish(self._ctx, C.byref(cnt)), "thj_segjuncs_finish")
        return cnt

    def download(self, cnt: CCounts) -> Events:
        j = np.zeros(cnt.n_juncs, dtype=JUNC_DTYPE)
        d = np.zeros(cnt.n_deletions, dtype=JUNC_DTYPE)
        ins = (CInsertion * max(1, cnt.n_insertions))()
        _check(self.lib, self.lib.thj_segjuncs_download(self._ctx, _ptr(j), _ptr(d), ins), "thj_segjuncs_download")
        il = [(int(ins[k].ref_id), int(ins[k].left), ins[k].seq.decode()) for k in range(cnt.n_insertions)]
        stats = {"windows": cnt.n_windows, "indel_pairs": cnt.n_indel_pairs, "rescue_pairs": cnt.n_rescue_pairs,
                 "overflow_blocks": cnt.n_overflow_blocks, "hits_read": cnt.n_hits_read}
        return Events(j, d, il, stats)

    def segjuncs(self, runs: Sequence[Tuple[Params, object]]) -> Events:
        """reset; run every (params, batch); finish; download -- one segment_juncs pass."""
        self.reset()
        for p, b in runs:
            self.run(p, b)
        return self.download(self.finish())

    # ---- coverage search (thj_covsearch_*): call between reset() and finish() of a segment_juncs pass
    def covsearch_reset(self):
        _check(self.lib, self.lib.thj_covsearch_reset_async(self._ctx), "thj_covsearch_reset_async")

    def covsearch_add_hits(self, batch):
        arg = C.byref(batch) if isinstance(batch, CSegBatch) else batch
        _check(self.lib, self.lib.thj_covsearch_add_hits_async(self._ctx, arg), "thj_covsearch_add_hits_async")

    def covsearch_add_reads(self, ium_reads: Sequence[str]):
        n = len(ium_reads)
        if not n:
            return
        off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum([len(r) for r in ium_reads], out=off[1:])
        bases = np.frombuffer("".join(ium_reads).encode(), dtype=np.uint8)
        W = words_per_plane(max(len(r) for r in ium_reads))
        planes = np.zeros(n * 3 * W, dtype=np.uint64)
        lens = np.zeros(n, dtype=np.uint16)
        _check(self.lib, self.lib.thj_reads_pack(C.c_int64(n), _ptr(off), _ptr(bases), W, _ptr(planes), _ptr(lens)), "thj_reads_pack")
        _check(self.lib, self.lib.thj_covsearch_add_reads(self._ctx, C.c_int64(n), W, _ptr(planes), _ptr(lens), 0), "thj_covsearch_add_reads")

    def covsearch_add_reads_device(self, n: int, W: int, planes_ptr: int, lens_ptr: int):
        """planes / lengths already on the device (thj_reads_pack layout)"""
        _check(self.lib, self.lib.thj_covsearch_add_reads(self._ctx, C.c_int64(n), W, C.c_void_p(planes_ptr), C.c_void_p(lens_ptr), 1),
               "thj_covsearch_add_reads")

    def covsearch_device_state(self):
        """-> (coverage bits ptr, n_words, sizes ptr, ext keys ptr, ext vals ptr, n_ext): device pointers of this rank's state"""
        bits, sizes, keys, vals = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        nw, ne = C.c_int64(), C.c_int64()
        _check(self.lib, self.lib.thj_covsearch_device_state(self._ctx, C.byref(bits), C.byref(nw), C.byref(sizes), C.byref(keys), C.byref(vals),
                                                             C.byref(ne)), "thj_covsearch_device_state")
        return bits.value, nw.value, sizes.value, keys.value, vals.value, ne.value

    def covsearch_merge(self, bits_ptr: int, sizes_ptr: int, keys_ptr: int, vals_ptr: int, n_ext: int):
        _check(self.lib, self.lib.thj_covsearch_merge_async(self._ctx, C.c_void_p(bits_ptr), C.c_void_p(sizes_ptr), C.c_void_p(keys_ptr),
                                                            C.c_void_p(vals_ptr), C.c_int64(n_ext)), "thj_covsearch_merge_async")

    def covsearch_run(self, min_cov_length: int, min_intron: int = 50, max_intron: int = 20000):
        _check(self.lib, self.lib.thj_covsearch_run_async(self._ctx, min_cov_length, min_intron, max_intron), "thj_covsearch_run_async")

    def covsearch_finish(self, max_cov_juncs: int = 5000000) -> int:
        found = C.c_int64()
        _check(self.lib, self.lib.thj_covsearch_finish(self._ctx, C.c_int64(max_cov_juncs), C.byref(found)), "thj_covsearch_finish")
        return found.value

    def butterfly_run(self, min_intron: int = 50, max_intron: int = 20000, max_cov_juncs: int = 5000000) -> int:
        """--butterfly-search (segment_juncs.cpp:4178-4249, :1698-2049) from the coverage map and the extension table of the
        covsearch_add_* calls; after covsearch_finish when the coverage search runs too.  -> junctions added to the pass's set"""
        found = C.c_int64()
        _check(self.lib, self.lib.thj_butterfly_run(self._ctx, int(min_intron), int(max_intron), C.c_int64(max_cov_juncs), C.byref(found)), "thj_butterfly_run")
        return found.value

    # ---- microexon search (thj_microexon_*): candidates on the device, window merge on the host, per-window pairing on the device
    def microexon_reset(self):
        _check(self.lib, self.lib.thj_microexon_reset_async(self._ctx), "thj_microexon_reset_async")

    def microexon_collect(self, p: Params, batch, read_side: int):
        arg = C.byref(batch) if isinstance(batch, CSegBatch) else batch
        cp = p.as_ctypes()
        _check(self.lib, self.lib.thj_microexon_collect(self._ctx, C.byref(cp), arg, int(read_side)), "thj_microexon_collect")

    def microexon_candidates(self) -> np.ndarray:
        ptr, n = C.c_void_p(), C.c_int64()
        _check(self.lib, self.lib.thj_microexon_candidates(self._ctx, C.byref(ptr), C.byref(n)), "thj_microexon_candidates")
        a = np.zeros(0, dtype=MX_CAND_DTYPE)
        if n.value:
            a = np.frombuffer((C.c_char * (n.value * MX_CAND_DTYPE.itemsize)).from_address(ptr.value), dtype=MX_CAND_DTYPE).copy()
            C.CDLL(None).free(ptr)
        return a

    def microexon_run(self, windows: np.ndarray, strs: np.ndarray, str_len: np.ndarray, str_window: np.ndarray, min_intron: int = 50, library_type: int = 0,
                      max_juncs: int = 5000000) -> int:
        w = np.ascontiguousarray(windows, dtype=MX_WINDOW_DTYPE)
        a, b, c_ = np.ascontiguousarray(strs, dtype=np.uint64), np.ascontiguousarray(str_len, dtype=np.uint8), np.ascontiguousarray(str_window, dtype=np.uint32)
        found = C.c_int64()
        _check(self.lib, self.lib.thj_microexon_run(self._ctx, C.c_void_p(w.ctypes.data), C.c_int64(len(w)), C.c_void_p(a.ctypes.data), C.c_void_p(b.ctypes.data),
                                                    C.c_void_p(c_.ctypes.data), C.c_int64(len(a)), int(min_intron), int(library_type), C.c_int64(max_juncs), C.byref(found)),
               "thj_microexon_run")
        return found.value

    def segjuncs_with_coverage_search(self, runs: Sequence[Tuple[Params, object]], ium_reads: Sequence[str], min_cov_length: int,
                                      min_intron: int = 50, max_intron: int = 20000, max_cov_juncs: int = 5000000):
        """One segment_juncs pass with the coverage search (segment_juncs.cpp:4268-4543) on top of the segment search:
        runs = (params, uploaded batch) of both sides, ium_reads = the initially unmapped reads (--ium-reads).
        -> (Events, junctions the coverage search found, counted with those the segment search also found)"""
        self.reset()
        self.covsearch_reset()
        for p, b in runs:
            self.run(p, b)
            self.covsearch_add_hits(b)
        self.covsearch_add_reads(ium_reads)
        self.covsearch_run(min_cov_length, min_intron, max_intron)
        found = self.covsearch_finish(max_cov_juncs)
        return self.download(self.finish()), found

    SJ_KERNELS = ("thj_k_sj_flat", "thj_k_sj_general<8, 256, true>", "thj_k_sj_general<32, 256, false>", "thj_k_segjuncs_shared",
                  "thj_k_segjuncs_rescue + thj_k_segjuncs_rescue_shared", "thj_k_sj_tasks_list", "thj_k_sj_rescue_scan + thj_k_sj_rescue_flat",
                  "thj_k_sj_tasks")

    def profile_serial(self, on: bool = True):
        """every kernel of the stage calls on the context's stream, one after the other: the profiles then give each kernel's own duration"""
        _check(self.lib, self.lib.thj_profile_serial(self._ctx, 1 if on else 0), "thj_profile_serial")

    def profile(self, enable: bool = True):
        """(ms per launch of each entry of SJ_KERNELS, runs, {reads and tasks of the lists}) since the last call"""
        ms = (C.c_double * 8)()
        st = (C.c_double * 4)()
        n = C.c_int64()
        _check(self.lib, self.lib.thj_profile_segjuncs(self._ctx, 1 if enable else 0, ms, C.byref(n), st), "thj_profile_segjuncs")
        return tuple(ms), n.value, {"many_reads": st[0], "mid_reads": st[1], "list_tasks": st[2], "flat_rescue_pairs": st[3]}

    def device_keys(self, kind: int) -> Tuple[int, int]:
        p = C.c_void_p()
        n = C.c_int64()
        _check(self.lib, self.lib.thj_segjuncs_device_keys(self._ctx, kind, C.byref(p), C.byref(n)),
               "thj_segjuncs_device_keys")
        return (p.value or 0), n.value

    def _fusion_pass(self, runs, ignore_ref_ids) -> int:
        """reset; thj_fusion_run_async for every (params, batch); finish -> number of fusions.  THJ_ERETRY at the finish (a batch had more
        raw candidates than the buffer held; it has been enlarged) runs the pass again."""
        runs = list(runs)
        ign = np.ascontiguousarray(list(ignore_ref_ids), dtype=np.uint32)
        for attempt in range(3):
            _check(self.lib, self.lib.thj_fusion_reset_async(self._ctx), "thj_fusion_reset_async")
            _check(self.lib, self.lib.thj_fusion_set_ignored(self._ctx, _ptr(ign) if len(ign) else None, len(ign)), "thj_fusion_set_ignored")
            for p, b in runs:
                cp = p.as_ctypes()
                arg = C.byref(b) if isinstance(b, CSegBatch) else b
                _check(self.lib, self.lib.thj_fusion_run_async(self._ctx, C.byref(cp), arg), "thj_fusion_run_async")
            n = C.c_int64()
            rc = self.lib.thj_fusion_finish(self._ctx, C.byref(n))
            if rc != -7 or attempt == 2:
                _check(self.lib, rc, "thj_fusion_finish")
                return int(n.value)
        raise AssertionError("unreachable")

    def fusions(self, runs, ignore_ref_ids=()) -> np.ndarray:
        """reset; thj_fusion_run_async for every (params, batch); finish; download -> FUSION_DTYPE array"""
        n = C.c_int64(self._fusion_pass(runs, ignore_ref_ids))
        out = np.zeros(max(1, n.value), dtype=FUSION_DTYPE)
        _check(self.lib, self.lib.thj_fusion_download(self._ctx, _ptr(out)), "thj_fusion_download")
        return out[:n.value]

    def device_insertions(self) -> Tuple[int, int, int]:
        k, v, n = C.c_void_p(), C.c_void_p(), C.c_int64()
        _check(self.lib, self.lib.thj_segjuncs_device_insertions(self._ctx, C.byref(k), C.byref(v), C.byref(n)),
               "thj_segjuncs_device_insertions")
        return (k.value or 0), (v.value or 0), n.value

    def merge_insertions(self, d_keys: int, d_vals: int, n: int):
        _check(self.lib, self.lib.thj_segjuncs_merge_insertions_async(self._ctx, C.c_void_p(d_keys), C.c_void_p(d_vals), C.c_int64(n)),
               "thj_segjuncs_merge_insertions_async")

    def merge_keys(self, kind: int, d_keys: int, n: int):
        _check(self.lib, self.lib.thj_segjuncs_merge_keys_async(self._ctx, kind, C.c_void_p(d_keys), C.c_int64(n)),
               "thj_segjuncs_merge_keys_async")


# ------------------------------------------------------------------ long_spanning_reads

from .batch import Aln, SpanBatch  # noqa: E402

ALN_DTYPE = np.dtype([
    ("read_idx", "<u4"), ("ref_id", "<u4"), ("left", "<i4"),
    ("flags", "u1"), ("mismatches", "u1"), ("edit_dist", "u1"), ("n_cigar", "u1"),
    ("AS", "<i2"), ("XM", "u1"), ("XO", "u1"), ("XG", "u1"), ("md_len", "u1"), ("order", "<u2"),
    ("cigar", "<u4", (16,)), ("md", "S40"),
])
assert ALN_DTYPE.itemsize == 128


class CSpanBatch(C.Structure):
    _fields_ = [("n_reads", C.c_int32), ("nseg", C.c_int32), ("words_per_plane", C.c_int32), ("qual_stride", C.c_int32),
                ("seg_off", C.c_void_p), ("hits", C.c_void_p), ("read_planes", C.c_void_p), ("read_len", C.c_void_p),
                ("quals", C.c_void_p), ("hit_heads", C.c_void_p)]


def encode_ins_seq(seq: str) -> int:
    v = 0
    for k, ch in enumerate(seq):
        v |= (INS_CODE.index(ch) if ch in INS_CODE else 4) << (3 * k)
    return v


def pack_span_batch(b: SpanBatch, lib=None):
    """-> dict of contiguous HOST arrays in the thj_span_batch layout"""
    lib = lib or load_lib()
    n = b.n_reads
    lens_ = np.diff(b.read_off) if n else np.zeros(0, dtype=np.int64)
    mx = int(lens_.max()) if n else 1
    W = words_per_plane(mx)
    planes = np.zeros(n * 3 * W, dtype=np.uint64)
    lens = np.zeros(n, dtype=np.uint16)
    bases = np.ascontiguousarray(b.bases, dtype=np.uint8)
    off = np.ascontiguousarray(b.read_off, dtype=np.int64)
    _check(lib, lib.thj_reads_pack(C.c_int64(n), _ptr(off), _ptr(bases), W, _ptr(planes), _ptr(lens)), "thj_reads_pack")
    stride = (mx + 3) // 4 * 4
    quals = np.zeros(n * stride, dtype=np.uint8)
    for r in range(n):
        quals[r * stride:r * stride + lens_[r]] = b.quals[off[r]:off[r + 1]]
    return dict(n_reads=n, nseg=b.nseg, W=W, qual_stride=stride, seg_off=np.ascontiguousarray(b.seg_off, dtype=np.uint32),
                hits=np.ascontiguousarray(b.hits), planes=planes, read_len=lens, quals=quals)


MD_ON_HOST = 255
_RC = bytes.maketrans(b"ACGTNacgtn", b"TGCANtgcan")


def md_on_host(seq_of_contig, read_seq: str, antisense: bool, left: int, cigar, lib=None, seq_of_contig2=None) -> str:
    """thj_md_string / thj_md_string2: the MD:Z of an alignment whose string does not fit a device record.  seq_of_contig: the
    contig's bases (str / bytes), seq_of_contig2: the second contig of a fusion alignment; read_seq: the read as sequenced"""
    lib = lib or load_lib()
    ref = seq_of_contig if isinstance(seq_of_contig, bytes) else seq_of_contig.encode()
    s = read_seq.encode()
    if antisense:
        s = s.translate(_RC)[::-1]
    cig = (C.c_uint32 * max(1, len(cigar)))(*cigar)
    buf = C.create_string_buffer(4096)
    if seq_of_contig2 is not None:
        ref2 = seq_of_contig2 if isinstance(seq_of_contig2, bytes) else seq_of_contig2.encode()
        n = lib.thj_md_string2(ref, C.c_int64(len(ref)), ref2, C.c_int64(len(ref2)), s, len(s), int(left), cig, len(cigar), buf, 4096)
    else:
        n = lib.thj_md_string(ref, C.c_int64(len(ref)), s, len(s), int(left), cig, len(cigar), buf, 4096)
    if n < 0:
        raise ThjError("thj_md_string: %s" % lib.thj_last_error().decode())
    return buf.value.decode()


SPAN_FUSION_DTYPE = np.dtype([("ref_id1", "<u4"), ("ref_id2", "<u4"), ("left", "<u4"), ("right", "<u4"), ("dir", "<u4")])   # thj_span_fusion
_FUSION_OPS = (7, 8, 9, 10)


def alns_from_array(a: np.ndarray, md_resolver=None) -> List[Aln]:
    """md_resolver(read_idx, ref_id, antisense, left, cigar) -> MD string, for records flagged THJ_MD_ON_HOST"""
    out = []
    for x in a:
        n = int(x["n_cigar"])
        cig = tuple(int(c) for c in x["cigar"][:n])
        ref_id2 = int(x["cigar"][15]) if any((c >> 28) in _FUSION_OPS for c in cig) else 0     # fusion alignment: ref_id2 in the last slot
        if int(x["md_len"]) == MD_ON_HOST:
            if md_resolver is None:
                raise ThjError("a record's MD string is left to the host (THJ_MD_ON_HOST) and no resolver was given")
            if ref_id2:
                md = md_resolver(int(x["read_idx"]), int(x["ref_id"]), bool(x["flags"] & 1), int(x["left"]), cig, ref_id2)
            else:
                md = md_resolver(int(x["read_idx"]), int(x["ref_id"]), bool(x["flags"] & 1), int(x["left"]), cig)
        else:
            md = x["md"][:int(x["md_len"])].decode()
        out.append(Aln(int(x["read_idx"]), int(x["ref_id"]), int(x["left"]), bool(x["flags"] & 1), bool(x["flags"] & 4),
                       int(x["mismatches"]), int(x["edit_dist"]), cig, int(x["AS"]), int(x["XM"]), int(x["XO"]), int(x["XG"]), md, ref_id2))
    return out


def span_md_resolver(seqs, batches, lib=None):
    """resolver over the host copies of a pass: seqs[ref_id - 1] = contig bases, batches = the SpanBatch objects in run order
    (read_idx counts through them)"""
    starts = [0]
    for b in batches:
        starts.append(starts[-1] + b.n_reads)

    def resolve(read_idx, ref_id, antisense, left, cigar, ref_id2=0):
        k = max(i for i in range(len(batches)) if starts[i] <= read_idx)
        b = batches[k]
        r = read_idx - starts[k]
        return md_on_host(seqs[ref_id - 1], b.bases[b.read_off[r]:b.read_off[r + 1]].tobytes().decode(), antisense, left, cigar, lib,
                          seqs[ref_id2 - 1] if ref_id2 else None)
    return resolve


def _ins_table(insertions) -> np.ndarray:
    t = np.zeros((max(1, len(insertions)), 4), dtype=np.uint32)
    for k, (ref, left, seq) in enumerate(insertions):
        t[k] = (ref, left, len(seq), encode_ins_seq(seq))
    return t


def _span_methods():
    def upload_span_fusions(self, fusions: np.ndarray):
        """--fusion-search: the .fusions list (SPAN_FUSION_DTYPE, Fusion::operator< order) for runs with Params.fusion_search"""
        f = np.ascontiguousarray(fusions, dtype=SPAN_FUSION_DTYPE)
        _check(self.lib, self.lib.thj_span_fusions_upload(self._ctx, _ptr(f) if len(f) else None, C.c_int64(len(f))), "thj_span_fusions_upload")

    def upload_span_sets(self, juncs: np.ndarray, insertions):
        j = np.ascontiguousarray(juncs, dtype=JUNC_DTYPE)
        t = _ins_table(insertions)
        _check(self.lib, self.lib.thj_span_sets_upload(self._ctx, _ptr(j), C.c_int64(len(j)), _ptr(t), C.c_int64(len(insertions))),
               "thj_span_sets_upload")

    def span_sets_from_segjuncs(self):
        _check(self.lib, self.lib.thj_span_sets_from_segjuncs(self._ctx), "thj_span_sets_from_segjuncs")

    def span_fusions_from_segjuncs(self):
        """--fusion-search: the list of the last fusion_search() / fusions() of this context, handed over on the device"""
        _check(self.lib, self.lib.thj_span_fusions_from_segjuncs(self._ctx), "thj_span_fusions_from_segjuncs")

    def fusion_search(self, runs, ignore_ref_ids=()) -> int:
        """fusions() without the download: reset; thj_fusion_run_async for every (params, batch); finish -> number of fusions"""
        return self._fusion_pass(runs, ignore_ref_ids)

    def span_hit_heads(self, d_hits: int, n_hits: int, d_heads: int):
        """the dense 16-byte head array of device-resident hit records (CSpanBatch.hit_heads)"""
        _check(self.lib, self.lib.thj_span_hit_heads_async(self._ctx, C.c_void_p(d_hits), C.c_int64(n_hits), C.c_void_p(d_heads)),
               "thj_span_hit_heads_async")

    def upload_span_batch(self, b: SpanBatch):
        d = pack_span_batch(b, self.lib)
        cb = CSpanBatch()
        cb.n_reads, cb.nseg, cb.words_per_plane, cb.qual_stride = d["n_reads"], d["nseg"], d["W"], d["qual_stride"]
        cb.seg_off, cb.hits, cb.read_planes, cb.read_len, cb.quals = [d[k].ctypes.data for k in ("seg_off", "hits", "planes", "read_len", "quals")]
        out = C.c_void_p()
        _check(self.lib, self.lib.thj_span_batch_upload(self._ctx, C.byref(cb), C.c_int64(len(d["hits"])), C.byref(out)),
               "thj_span_batch_upload")
        self._span_batches = getattr(self, "_span_batches", []) + [out]
        if not hasattr(self, "_span_host"):
            self._span_host = {}
        self._span_host[out.value] = b
        return out

    def span_reset(self):
        _check(self.lib, self.lib.thj_span_reset_async(self._ctx), "thj_span_reset_async")

    def span_run(self, p: Params, batch):
        cp = p.as_ctypes()
        arg = C.byref(batch) if isinstance(batch, CSpanBatch) else batch
        _check(self.lib, self.lib.thj_span_run_async(self._ctx, C.byref(cp), arg), "thj_span_run_async")

    def span_finish(self) -> int:
        n = C.c_int64()
        _check(self.lib, self.lib.thj_span_finish(self._ctx, C.byref(n)), "thj_span_finish")
        return n.value

    def span_download(self, n: int) -> np.ndarray:
        a = np.zeros(max(1, n), dtype=ALN_DTYPE)
        _check(self.lib, self.lib.thj_span_download(self._ctx, _ptr(a)), "thj_span_download")
        return a[:n]

    def spanning(self, p: Params, batches, md_resolver=None) -> List[Aln]:
        """md_resolver: see alns_from_array; built automatically when the genome was uploaded from strings kept by the caller
        (Context.host_seqs) and the batches came from upload_span_batch"""
        for attempt in range(4):
            self.span_reset()
            for b in batches:
                self.span_run(p, b)
            n = C.c_int64()
            rc = self.lib.thj_span_finish(self._ctx, C.byref(n))
            if rc != -7:                       # THJ_ERETRY: the extra-record pool was enlarged, the pass runs again
                break
        _check(self.lib, rc, "thj_span_finish")
        a = self.span_download(n.value)
        if md_resolver is None and getattr(self, "host_seqs", None) is not None:
            hb = [self._span_host.get(getattr(b, "value", None)) for b in batches]
            if all(x is not None for x in hb):
                md_resolver = span_md_resolver(self.host_seqs, hb, self.lib)
        return alns_from_array(a, md_resolver)

    def span_run_pair(self, p: Params, batch0, batch1):
        """two batches (the two sides of a pass) beside each other: thj_span_run_pair_async"""
        cp = p.as_ctypes()
        a0 = C.byref(batch0) if isinstance(batch0, CSpanBatch) else batch0
        a1 = C.byref(batch1) if isinstance(batch1, CSpanBatch) else batch1
        _check(self.lib, self.lib.thj_span_run_pair_async(self._ctx, C.byref(cp), a0, a1), "thj_span_run_pair_async")

    def span_tier0_pair(self, p: Params, batch0, batch1):
        """the pair's tier 0 ahead of span_run_pair on the same batches (needs no junction set): thj_span_tier0_pair_async"""
        cp = p.as_ctypes()
        a0 = C.byref(batch0) if isinstance(batch0, CSpanBatch) else batch0
        a1 = C.byref(batch1) if isinstance(batch1, CSpanBatch) else batch1
        _check(self.lib, self.lib.thj_span_tier0_pair_async(self._ctx, C.byref(cp), a0, a1), "thj_span_tier0_pair_async")

    def span_tier_counts(self):
        """of the batch launched last: reads to the closure kernels, to the multihit kernel, on to the general kernel"""
        c = (C.c_int64 * 5)()
        _check(self.lib, self.lib.thj_span_tier_counts(self._ctx, c), "thj_span_tier_counts")
        return int(c[0]), int(c[1]), int(c[2])

    def span_chain_count(self):
        """of the batch launched last: the reads that travelled as chain entries (tier 0 -> thj_k_join_finish -> thj_k_finish)"""
        c = (C.c_int64 * 5)()
        _check(self.lib, self.lib.thj_span_tier_counts(self._ctx, c), "thj_span_tier_counts")
        return int(c[3])

    def stream_info(self):
        """thj_ctx_stream_info: {"n_side", "independent": [..], "ratio": [..]} of the side streams made so far"""
        n = C.c_int32()
        ind = (C.c_int32 * 3)()
        ratio = (C.c_double * 3)()
        _check(self.lib, self.lib.thj_ctx_stream_info(self._ctx, C.byref(n), ind, ratio), "thj_ctx_stream_info")
        return {"n_side": int(n.value), "independent": [bool(ind[k]) for k in range(n.value)], "ratio": [float(ratio[k]) for k in range(n.value)]}

    def probe_streams(self, need=2):
        _check(self.lib, self.lib.thj_ctx_probe_streams(self._ctx, int(need)), "thj_ctx_probe_streams")
        return self.stream_info()

    def span_chain_groups(self):
        """of the batch launched last: the multihit reads whose chains travelled as chain entries (thj_k_chains)"""
        c = (C.c_int64 * 5)()
        _check(self.lib, self.lib.thj_span_tier_counts(self._ctx, c), "thj_span_tier_counts")
        return int(c[4])

    Context.SPAN_KERNELS = ("thj_k_stitch_contig", "thj_k_chains", "thj_k_join", "thj_k_join_closure", "thj_k_finish", "thj_k_stitch", "thj_k_stitch_pack", "thj_k_stitch_generic")

    def profile_span(self, enable: bool = True):
        """-> ([ms per launch of each entry of SPAN_KERNELS], launches)"""
        ms = (C.c_double * 8)()
        n = C.c_int64()
        _check(self.lib, self.lib.thj_profile_span(self._ctx, 1 if enable else 0, ms, C.byref(n)), "thj_profile_span")
        return list(ms), n.value

    for f in (upload_span_fusions, upload_span_sets, span_sets_from_segjuncs, span_fusions_from_segjuncs, fusion_search, upload_span_batch, span_reset, span_run, span_finish,
              span_download, spanning, profile_span, span_tier_counts, span_hit_heads, span_run_pair, span_tier0_pair, span_chain_count, span_chain_groups, stream_info, probe_streams):
        setattr(Context, f.__name__, f)


_span_methods()

ABI_SYMBOLS += ["thj_bgzf_inflate", "thj_ingest_seg_batch", "thj_ingest_span_hits", "thj_span_batch_attach_reads"]
ABI_SYMBOLS += ["thj_juncbed_configure", "thj_juncbed_reset_async", "thj_juncbed_add_span_async", "thj_juncbed_add_records",
                "thj_juncbed_finish", "thj_juncbed_download", "thj_juncbed_collect_indels", "thj_juncbed_add_records_seq",
                "thj_juncbed_add_span_seq_async", "thj_juncbed_indel_counts", "thj_juncbed_indel_download",
                "thj_juncbed_collect_fusions", "thj_juncbed_fusion_count", "thj_juncbed_fusion_download",
                "thj_juncbed_known_junctions", "thj_juncbed_read_filter", "thj_juncbed_best_alignments", "thj_juncbed_best_counts",
                "thj_juncbed_pair_alignments", "thj_juncbed_add_pairs", "thj_juncbed_add_pairs_seq", "thj_juncbed_pair_counts"]
ABI_SYMBOLS += ["thj_md_string"]
ABI_SYMBOLS += ["thj_microexon_reset_async", "thj_microexon_collect", "thj_microexon_candidates", "thj_microexon_run"]
ABI_SYMBOLS += ["thj_butterfly_run", "thj_covsearch_add_reads_bam", "thj_covsearch_reserve_reads"]
ABI_SYMBOLS += ["thj_span_sets_upload", "thj_span_sets_from_segjuncs", "thj_span_fusions_from_segjuncs", "thj_span_batch_upload", "thj_span_batch_free",
                "thj_span_reset_async", "thj_span_run_async", "thj_span_run_pair_async", "thj_span_tier0_pair_async", "thj_span_finish", "thj_span_download", "thj_profile_span",
                "thj_span_tier_counts", "thj_span_device_records"]


# ------------------------------------------------------------------ junction consensus (thj_juncbed_*)

JUNCSTAT_DTYPE = np.dtype([("ref_id", "<u4"), ("left", "<u4"), ("right", "<u4"), ("antisense", "<u4"), ("left_extent", "<u4"),
                           ("right_extent", "<u4"), ("support", "<u4"), ("reserved", "<u4")])


def junctions_bed_text(js: np.ndarray, names: Sequence[str]) -> str:
    """print_junctions / print_junction (junctions.cpp:100-120, :330-350)"""
    out = ['track name=junctions description="TopHat junctions"\n']
    for k, j in enumerate(js):
        start = int(j["left"]) + 1 - int(j["left_extent"])
        end = int(j["right"]) + int(j["right_extent"])
        out.append("%s\t%d\t%d\tJUNC%08d\t%d\t%s\t%d\t%d\t255,0,0\t2\t%d,%d\t0,%d\n" % (
            names[int(j["ref_id"]) - 1], start, end, k + 1, int(j["support"]), "-" if j["antisense"] else "+", start, end,
            int(j["left_extent"]), int(j["right_extent"]), int(j["right"]) - start))
    return "".join(out)


INSSTAT_DTYPE = np.dtype([("ref_id", "<u4"), ("left", "<u4"), ("len", "<u4"), ("support", "<u4"), ("left_extent", "<u4"),
                          ("right_extent", "<u4"), ("bases", "S16")])
assert INSSTAT_DTYPE.itemsize == 40


def insertions_bed_text(ins: np.ndarray, names: Sequence[str]) -> str:
    """print_insertions (insertions.cpp:87-101): the support is capped at 1000 here, where the text is written; left is printed
    with %d (an INS at position 0 has left = -1)"""
    out = ['track name=insertions description="TopHat insertions"\n']
    for i in ins:
        left = int(np.int32(np.uint32(i["left"])))
        out.append("%s\t%d\t%d\t%s\t%d\n" % (names[int(i["ref_id"]) - 1], left, left, bytes(i["bases"])[:int(i["len"])].decode(), min(int(i["support"]), 1000)))
    return "".join(out)


def deletions_bed_text(dels: np.ndarray, names: Sequence[str]) -> str:
    """print_deletions (deletions.cpp:36-45): left + 1, right, "-", the support uncapped"""
    out = ['track name=deletions description="TopHat deletions"\n']
    for d in dels:
        out.append("%s\t%d\t%d\t-\t%d\n" % (names[int(d["ref_id"]) - 1], int(np.int32(np.uint32(d["left"]) + np.uint32(1))), int(np.int32(np.uint32(d["right"]))),
                                             int(d["support"])))
    return "".join(out)


FUSSTAT_DTYPE = np.dtype([("ref_id1", "<u4"), ("ref_id2", "<u4"), ("left", "<u4"), ("right", "<u4"), ("dir", "<u4"), ("count", "<u4"), ("unsupport", "<u4"),
                          ("left_ext", "<u4"), ("right_ext", "<u4"), ("n_diffs", "<u4"), ("diffs", "<u4", (5,)), ("left_bases", "<u4", (50,)),
                          ("right_bases", "<u4", (50,)), ("seq1", "S100"), ("seq2", "S100")])
assert FUSSTAT_DTYPE.itemsize == 660


def fusions_out_text(stats: np.ndarray, names: Sequence[str]) -> str:
    """print_fusions (fusions.cpp:347-433).  symm is accumulated in float term by term as there; the two pair columns are 0 and the
    pair list is empty (pair_support is not reproduced: what the reference prints for single-end input)"""
    out = []
    for f in stats:
        count = int(f["count"])
        if count <= 0:
            continue
        lb, rb = [int(x) for x in f["left_bases"]], [int(x) for x in f["right_bases"]]
        symm = np.float32(0.0)
        for a, b in zip(lb, rb):
            term = np.float32(a - b) / np.float32(count)
            symm = np.float32(symm + np.float32(term * term))
        s1, s2 = bytes(f["seq1"]).decode(), bytes(f["seq2"]).decode()
        h1, h2 = len(s1) // 2, len(s2) // 2
        out.append("%s-%s\t%d\t%d\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%.6f\t@\t%s\t@\t%s %s\t@\t%s %s\t@\t%s\t@\t%s\t@\t\n" % (
            names[int(f["ref_id1"]) - 1], names[int(f["ref_id2"]) - 1], int(np.int32(np.uint32(f["left"]))), int(np.int32(np.uint32(f["right"]))),
            {7: "ff", 8: "fr", 9: "rf"}.get(int(f["dir"]), "rr"), count, 0, 0, int(f["unsupport"]), int(f["left_ext"]), int(f["right_ext"]), float(symm),
            "".join("%d " % int(x) for x in f["diffs"][:int(f["n_diffs"])]), s1[:h1], s1[h1:], s2[:h2], s2[h2:],
            "".join("%d " % x for x in lb), "".join("%d " % x for x in rb)))
    return "".join(out)


def _juncbed_methods():
    def juncbed_configure(self, capacity: int):
        _check(self.lib, self.lib.thj_juncbed_configure(self._ctx, C.c_int64(capacity)), "thj_juncbed_configure")

    def juncbed_reset(self):
        _check(self.lib, self.lib.thj_juncbed_reset_async(self._ctx), "thj_juncbed_reset_async")

    def juncbed_add_span(self):
        """folds the records of the last spanning pass (still on the device) in"""
        _check(self.lib, self.lib.thj_juncbed_add_span_async(self._ctx), "thj_juncbed_add_span_async")

    def juncbed_add_records(self, recs: np.ndarray):
        """recs: ALN_DTYPE array (ref_id, left, flags & 4 = antisense splice, n_cigar, cigar are read; with juncbed_read_filter also mismatches)"""
        a = np.ascontiguousarray(recs, dtype=ALN_DTYPE)
        _check(self.lib, self.lib.thj_juncbed_add_records(self._ctx, _ptr(a) if len(a) else None, C.c_int64(len(a)), 0), "thj_juncbed_add_records")

    def juncbed_finish(self, min_anchor_len: int = 8) -> np.ndarray:
        n = C.c_int64()
        _check(self.lib, self.lib.thj_juncbed_finish(self._ctx, min_anchor_len, C.byref(n)), "thj_juncbed_finish")
        out = np.zeros(max(1, n.value), dtype=JUNCSTAT_DTYPE)
        _check(self.lib, self.lib.thj_juncbed_download(self._ctx, _ptr(out)), "thj_juncbed_download")
        return out[:n.value]

    def juncbed_collect_indels(self, on: bool = True):
        """between juncbed_reset and the first add: the insertion and deletion sets are reduced beside the junctions"""
        _check(self.lib, self.lib.thj_juncbed_collect_indels(self._ctx, 1 if on else 0), "thj_juncbed_collect_indels")

    def juncbed_add_records_seq(self, recs: np.ndarray, ins_seqs: Sequence[str]):
        """recs as for juncbed_add_records; ins_seqs[i] = the letters of record i's I / i ops, one after the other in cigar order"""
        a = np.ascontiguousarray(recs, dtype=ALN_DTYPE)
        off = np.zeros(len(a) + 1, dtype=np.int64)
        np.cumsum([len(x) for x in ins_seqs], out=off[1:])
        bases = "".join(ins_seqs).encode()
        _check(self.lib, self.lib.thj_juncbed_add_records_seq(self._ctx, _ptr(a) if len(a) else None, C.c_int64(len(a)), _ptr(off), C.c_char_p(bases)),
               "thj_juncbed_add_records_seq")

    def juncbed_add_span_seq(self, batch):
        """juncbed_add_span with the pass's batch (from upload_span_batch): the inserted bases come from its reads on the device"""
        arg = C.byref(batch) if isinstance(batch, CSpanBatch) else batch
        _check(self.lib, self.lib.thj_juncbed_add_span_seq_async(self._ctx, arg), "thj_juncbed_add_span_seq_async")

    def juncbed_indels(self):
        """after juncbed_finish -> (INSSTAT_DTYPE array, JUNCSTAT_DTYPE array of the deletions), each in its set's order"""
        ni, nd = C.c_int64(), C.c_int64()
        _check(self.lib, self.lib.thj_juncbed_indel_counts(self._ctx, C.byref(ni), C.byref(nd)), "thj_juncbed_indel_counts")
        ins = np.zeros(max(1, ni.value), dtype=INSSTAT_DTYPE)
        dels = np.zeros(max(1, nd.value), dtype=JUNCSTAT_DTYPE)
        _check(self.lib, self.lib.thj_juncbed_indel_download(self._ctx, _ptr(ins), _ptr(dels)), "thj_juncbed_indel_download")
        return ins[:ni.value], dels[:nd.value]

    def juncbed_collect_fusions(self, on: bool = True, anchor_len: int = 20, read_mismatches: int = 2, multireads: int = 2):
        """between juncbed_reset and the first add: the fusion set (fusions.out) is reduced beside the junctions; the add calls then
        read read_idx (the reads of one call, numbered from 0) and edit_dist of every record"""
        _check(self.lib, self.lib.thj_juncbed_collect_fusions(self._ctx, 1 if on else 0, anchor_len, read_mismatches, multireads), "thj_juncbed_collect_fusions")

    def juncbed_fusions(self):
        """after juncbed_finish -> FUSSTAT_DTYPE array, the rows of fusions.out in their order"""
        n = C.c_int64()
        _check(self.lib, self.lib.thj_juncbed_fusion_count(self._ctx, C.byref(n)), "thj_juncbed_fusion_count")
        out = np.zeros(max(1, n.value), dtype=FUSSTAT_DTYPE)
        _check(self.lib, self.lib.thj_juncbed_fusion_download(self._ctx, _ptr(out)), "thj_juncbed_fusion_download")
        return out[:n.value]

    def juncbed_known_junctions(self, juncs):
        """between juncbed_reset and the first add: the annotated junctions (tophat_reports --gtf-juncs), a JUNC_DTYPE array or a list of
        (ref_id, left, right, antisense) in any order; they are accepted whatever their extents, length and support, and no neighbour
        on the other strand knocks them out.  An empty list turns it off."""
        if isinstance(juncs, np.ndarray) and juncs.dtype.names:
            j = np.ascontiguousarray(juncs, dtype=JUNC_DTYPE)
        else:
            j = np.zeros(len(juncs), dtype=JUNC_DTYPE)
            for k, (ref, left, right, anti) in enumerate(juncs):
                j[k] = (int(ref) & 0xFFFFFFFF, int(left) & 0xFFFFFFFF, int(right) & 0xFFFFFFFF, 1 if anti else 0)
        _check(self.lib, self.lib.thj_juncbed_known_junctions(self._ctx, _ptr(j) if len(j) else None, C.c_int64(len(j))), "thj_juncbed_known_junctions")

    def juncbed_read_filter(self, on: bool = True, read_mismatches: int = 2, read_gap_length: int = 2, read_edit_dist: int = 2):
        """between juncbed_reset and the first add: a record with more mismatches (its `mismatches` field), gap bases (the I, i, D, d of
        its cigar) or (uint8)(mismatches + gap bases) than the three limits is passed over by every set in both passes"""
        _check(self.lib, self.lib.thj_juncbed_read_filter(self._ctx, 1 if on else 0, read_mismatches, read_gap_length, read_edit_dist), "thj_juncbed_read_filter")

    def juncbed_best_alignments(self, on: bool = True, max_multihits: int = 20, suppress_hits: bool = False, bowtie2_max_penalty: int = 6):
        """between juncbed_reset and the first add: only each read's best alignments count (read_best_alignments in both modes, the
        AlignStatus score, the --max-multihits cap with the reference's generator; single-end).  A read = the records of one add call
        that follow each other under one read_idx; the add calls then read read_idx (below the call's size, never falling) and AS."""
        _check(self.lib, self.lib.thj_juncbed_best_alignments(self._ctx, 1 if on else 0, max_multihits, 1 if suppress_hits else 0, bowtie2_max_penalty),
               "thj_juncbed_best_alignments")

    def juncbed_best_counts(self):
        """after juncbed_finish -> (reads, reads that lost records to the choice, reads over the cap, first-pass duplicate records)"""
        out = (C.c_int64 * 4)()
        _check(self.lib, self.lib.thj_juncbed_best_counts(self._ctx, out), "thj_juncbed_best_counts")
        return tuple(int(x) for x in out)

    def juncbed_pair_alignments(self, on: bool = True, inner_dist_mean: int = 200, inner_dist_std_dev: int = 20, fusion_min_dist: int = 10000000,
                                report_mixed: bool = False, report_discordant: bool = False):
        """between juncbed_reset and the first add, after juncbed_best_alignments: inserts are graded (pair_best_alignments in both modes, the
        InsertAlignmentGrade score with its too_far rescue, the cap over pairs); the records then come through juncbed_add_pairs"""
        _check(self.lib, self.lib.thj_juncbed_pair_alignments(self._ctx, 1 if on else 0, inner_dist_mean, inner_dist_std_dev, fusion_min_dist, 1 if report_mixed else 0,
                                                              1 if report_discordant else 0), "thj_juncbed_pair_alignments")

    def juncbed_add_pairs(self, left: np.ndarray, right: np.ndarray):
        """left, right: ALN_DTYPE arrays; read_idx = the insert's number inside the call (it does not fall within a side and stays below
        len(left) + len(right)); an insert on one side only is a singleton.  Several calls continue the visit order."""
        a, b = np.ascontiguousarray(left, dtype=ALN_DTYPE), np.ascontiguousarray(right, dtype=ALN_DTYPE)
        _check(self.lib, self.lib.thj_juncbed_add_pairs(self._ctx, _ptr(a) if len(a) else None, C.c_int64(len(a)), _ptr(b) if len(b) else None, C.c_int64(len(b))),
               "thj_juncbed_add_pairs")

    def juncbed_add_pairs_seq(self, left: np.ndarray, left_ins_seqs: Sequence[str], right: np.ndarray, right_ins_seqs: Sequence[str]):
        """juncbed_add_pairs plus, per side, ins_seqs[i] = the letters of record i's I / i ops, one after the other in cigar order"""
        a, b = np.ascontiguousarray(left, dtype=ALN_DTYPE), np.ascontiguousarray(right, dtype=ALN_DTYPE)
        offs, text = [], []
        for seqs, n in ((left_ins_seqs, len(a)), (right_ins_seqs, len(b))):
            off = np.zeros(n + 1, dtype=np.int64)
            np.cumsum([len(x) for x in seqs], out=off[1:])
            offs.append(off); text.append("".join(seqs).encode())
        _check(self.lib, self.lib.thj_juncbed_add_pairs_seq(self._ctx, _ptr(a) if len(a) else None, C.c_int64(len(a)), _ptr(offs[0]), C.c_char_p(text[0]),
                                                            _ptr(b) if len(b) else None, C.c_int64(len(b)), _ptr(offs[1]), C.c_char_p(text[1])), "thj_juncbed_add_pairs_seq")

    def juncbed_pair_counts(self):
        """after juncbed_finish -> (inserts with both sides, inserts of which a pair is reported, inserts over the cap, singletons, reads that
        contribute nothing because their mate has no alignment left and mixed alignments are not reported)"""
        out = (C.c_int64 * 5)()
        _check(self.lib, self.lib.thj_juncbed_pair_counts(self._ctx, out), "thj_juncbed_pair_counts")
        return tuple(int(x) for x in out)

    for f in (juncbed_configure, juncbed_reset, juncbed_add_span, juncbed_add_records, juncbed_finish, juncbed_collect_indels, juncbed_add_records_seq,
              juncbed_add_span_seq, juncbed_indels, juncbed_collect_fusions, juncbed_fusions, juncbed_known_junctions, juncbed_read_filter,
              juncbed_best_alignments, juncbed_best_counts, juncbed_pair_alignments, juncbed_add_pairs, juncbed_add_pairs_seq, juncbed_pair_counts):
        setattr(Context, f.__name__, f)


_juncbed_methods()


MX_CAND_DTYPE = np.dtype([("ordinal", "<u4"), ("rank", "<u2"), ("side", "u1"), ("len", "u1"), ("ref_id", "<u4"), ("left", "<i4"), ("right", "<i4"),
                          ("reserved", "<u4"), ("str", "<u8")])
MX_WINDOW_DTYPE = np.dtype([("ref_id", "<u4"), ("left", "<i4"), ("right", "<i4"), ("side", "<i4")])
assert MX_CAND_DTYPE.itemsize == 32 and MX_WINDOW_DTYPE.itemsize == 16


def microexon_merge_windows(cands: np.ndarray):
    """add_to_microexon_windows (segment_juncs.cpp:3675-3735) over the candidates in visiting order -- the Python mirror of
    csrc/host/thj_mx_host.h (the executables use that one) -> (windows, strs, str_len, str_window) for Context.microexon_run"""
    import bisect
    order = np.lexsort((cands["rank"], cands["ordinal"], cands["side"]))
    keys, vals = [], []                                   # sorted (ref, left, right) -> (side, [candidate indices])

    def overlap(ll, lr, rl, rr):
        return (rl <= ll < rr) or (rl < lr < rr) or (ll <= rl < lr) or (ll < rr < lr)
    for ci in order:
        c = cands[ci]
        ref, lbd, rbd, side = int(c["ref_id"]), int(c["left"]), int(c["right"]), int(c["side"])
        key = (ref, lbd, rbd)
        lb = bisect.bisect_left(keys, key)
        ub = bisect.bisect_left(keys, (ref, rbd, rbd + 1))
        if lb == len(keys):
            keys.append(key); vals.append((side, [int(ci)]))
            continue
        first, last, new_vec, have = None, ub, [], False
        for k in range(lb, ub):
            if overlap(keys[k][1], keys[k][2], lbd, rbd):
                have = True
                if first is None:
                    first = k
                key = (ref, min(keys[k][1], lbd), max(keys[k][2], rbd))
                new_vec += vals[k][1]
            elif first is not None:
                last = k
        if first is not None:
            del keys[first:last]; del vals[first:last]
        new_vec = new_vec + [int(ci)] if have else [int(ci)]
        at = bisect.bisect_left(keys, key)
        if at < len(keys) and keys[at] == key:
            continue                                       # map::insert leaves an existing key alone
        keys.insert(at, key); vals.insert(at, (side, new_vec))
    windows = np.zeros(len(keys), dtype=MX_WINDOW_DTYPE)
    strs, lens, wins = [], [], []
    for w, (k, (side, idx)) in enumerate(zip(keys, vals)):
        windows[w] = (k[0], k[1], k[2], side)
        for ci in idx:
            strs.append(int(cands[ci]["str"])); lens.append(int(cands[ci]["len"])); wins.append(w)
    return windows, np.array(strs, dtype=np.uint64), np.array(lens, dtype=np.uint8), np.array(wins, dtype=np.uint32)


def aln_array_from_tuples(recs) -> np.ndarray:
    """[(ref_id, left, antisense_splice, [(op, len) ...][, ref_id2])] -> ALN_DTYPE array (the fields the junction consensus reads; a fusion
    alignment has at most 15 ops and its second contig in cigar[15])"""
    a = np.zeros(len(recs), dtype=ALN_DTYPE)
    for k, rec in enumerate(recs):
        ref, left, anti, cig = rec[:4]
        a[k]["ref_id"], a[k]["left"], a[k]["flags"], a[k]["n_cigar"] = ref, left, 4 if anti else 0, len(cig)
        for i, (op, ln) in enumerate(cig):
            a[k]["cigar"][i] = (op << 28) | ln
        if len(rec) > 4 and rec[4]:
            a[k]["cigar"][15] = rec[4]
        if len(rec) > 5:                                      # (..., ref_id2 or 0, read_idx, edit_dist): what the fusion set reads besides
            a[k]["read_idx"], a[k]["edit_dist"] = rec[5], rec[6] if len(rec) > 6 else 0
    return a


# ------------------------------------------------------------------ the BAM writer's device side (thj_bamout.hip)

ABI_SYMBOLS += ["thj_span_bam_encode", "thj_bgzf_deflate", "thj_bam_stream_upload", "thj_bam_stream_download", "thj_span_batch_reads_host"]
ABI_SYMBOLS += ["thj_span_juncdb_upload", "thj_span_juncdb_fusion_contigs", "thj_ingest_span_batch_spliced"]       # junction-db segment maps on the device
ABI_SYMBOLS += ["thj_bam_contig_names_upload", "thj_span_bam_encode_records"]      # fusion alignments' two records on the device


def bgzf_plan_cuts(sizes: Sequence[int], block: int = 0x10000) -> List[int]:
    """where BGZF members end in a stream of records that starts a member: bam_write1 calls bgzf_flush_try(4 + block_len) -- a record
    that does not fit what is left of the 64 KiB block starts a new one (bam.c:225, bgzf.c:587-592) -- and bgzf_write flushes a full
    block (bgzf.c:594-623).  The last member is closed at the end of the stream.  The Python mirror of BamWriter::plan_cuts."""
    cuts, off, pos = [], 0, 0
    for s in sizes:
        if off + s > block and off > 0:
            cuts.append(pos); off = 0
        while s > 0:
            c = min(block - off, s)
            off += c; pos += c; s -= c
            if off == block:
                cuts.append(pos); off = 0
    if off:
        cuts.append(pos)
    return cuts


def _bamout_methods():
    def bam_stream_upload(self, data: bytes):
        buf = np.frombuffer(data, dtype=np.uint8)
        _check(self.lib, self.lib.thj_bam_stream_upload(self._ctx, _ptr(buf) if len(data) else None, C.c_int64(len(data))), "thj_bam_stream_upload")
        self._bam_bytes = len(data)

    def bam_stream_download(self, n: int) -> bytes:
        buf = np.zeros(max(1, n), dtype=np.uint8)
        _check(self.lib, self.lib.thj_bam_stream_download(self._ctx, _ptr(buf)), "thj_bam_stream_download")
        return buf[:n].tobytes()

    def bgzf_deflate(self, member_end: Sequence[int]):
        """the context's stream cut at member_end -> ([raw DEFLATE stream per member], [CRC-32 per member])"""
        ends = np.asarray(member_end, dtype=np.int64)
        n = len(ends)
        comp = np.zeros(max(1, n) * 65536, dtype=np.uint8)
        clen = np.zeros(max(1, n), dtype=np.uint32); crc = np.zeros(max(1, n), dtype=np.uint32)
        total = C.c_int64()
        _check(self.lib, self.lib.thj_bgzf_deflate(self._ctx, C.c_int64(n), _ptr(ends), _ptr(comp), C.c_int64(comp.size), _ptr(clen), _ptr(crc), C.byref(total)),
               "thj_bgzf_deflate")
        out, at = [], 0
        for k in range(n):
            out.append(comp[at:at + int(clen[k])].tobytes()); at += int(clen[k])
        assert at == total.value
        return out, [int(x) for x in crc[:n]]

    for f in (bam_stream_upload, bam_stream_download, bgzf_deflate):
        setattr(Context, f.__name__, f)


_bamout_methods()


# ------------------------------------------------------------------ the stream in `samtools sort` order (thj_bamsort.hip)

ABI_SYMBOLS += ["thj_bam_stream_sort"]
SAMTOOLS_SORT_MAX_MEM = 500_000_000                       # bam_sort's max_mem when -m is not given (tophat.py gives none)


def _bamsort_methods():
    def bam_stream_sort(self, sizes: Sequence[int], max_mem: int = SAMTOOLS_SORT_MAX_MEM):
        """the context's stream (records of these sizes, block_size fields included, back to back) put into the order samtools 0.1.18's
        `sort` gives them with -m max_mem -> (the sizes in the new order, how many blocks the reference would have written; 1 = no merge)"""
        s = np.ascontiguousarray(np.asarray(sizes, dtype=np.uint32))
        nb = C.c_int64()
        _check(self.lib, self.lib.thj_bam_stream_sort(self._ctx, _ptr(s) if len(s) else None, C.c_int64(len(s)), C.c_int64(max_mem), C.byref(nb)), "thj_bam_stream_sort")
        return [int(x) for x in s], int(nb.value)

    setattr(Context, bam_stream_sort.__name__, bam_stream_sort)


_bamsort_methods()


# ------------------------------------------------------------------ reported alignments straight from BAM bytes (thj_juncbed_add_bam)

ABI_SYMBOLS += ["thj_juncbed_add_bam"]
ABI_SYMBOLS += ["thj_juncbed_collect_accepted", "thj_juncbed_report_bam", "thj_juncbed_collect_accepted_pairs", "thj_juncbed_report_pairs_bam"]      # accepted_hits.bam's records on the device
JUNCBED_PIECE_MEMBERS = 4096                              # BGZF members per add call, as thj_junctions cuts its inputs


class CBamPiece(C.Structure):                             # thj_bam_piece
    _fields_ = [("comp", C.c_void_p), ("comp_bytes", C.c_int64), ("first_skip", C.c_uint32), ("n_tid", C.c_int32), ("tid2ref", C.c_void_p)]


def bam_layout(data: bytes):
    """-> (member offsets with the end of the data as the last entry, index of the member the first record lies in, its offset inside
    that member, the header's target names).  Empty members count; the data must be whole BGZF members."""
    import struct
    import zlib
    offs, off = [], 0
    while off < len(data):
        if len(data) - off < 28 or data[off:off + 4] != b"\x1f\x8b\x08\x04":
            raise ThjError("not a run of whole BGZF members (offset %d)" % off)
        xlen = struct.unpack_from("<H", data, off + 10)[0]
        x, bsize = off + 12, 0
        while x + 4 <= off + 12 + xlen:
            slen = struct.unpack_from("<H", data, x + 2)[0]
            if data[x:x + 2] == b"BC" and slen == 2:
                bsize = struct.unpack_from("<H", data, x + 4)[0] + 1
            x += 4 + slen
        if not bsize or off + bsize > len(data):
            raise ThjError("not a run of whole BGZF members (offset %d)" % off)
        offs.append(off)
        off += bsize
    offs.append(len(data))
    # the header: magic, text, targets -- inflated member by member until it is all there
    h, ends = b"", []

    def have(n):
        nonlocal h
        while len(h) < n and len(ends) < len(offs) - 1:
            a, b = offs[len(ends)], offs[len(ends) + 1]
            xl = struct.unpack_from("<H", data, a + 10)[0]
            h += zlib.decompress(data[a + 12 + xl:b - 8], -15)
            ends.append(len(h))
        return len(h) >= n
    if not have(12) or h[:4] != b"BAM\x01":
        raise ThjError("not a BAM file")
    l_text = struct.unpack_from("<i", h, 4)[0]
    if not have(12 + l_text):
        raise ThjError("truncated BAM header")
    n_ref = struct.unpack_from("<i", h, 8 + l_text)[0]
    p, targets = 12 + l_text, []
    for _ in range(n_ref):
        if not have(p + 4):
            raise ThjError("truncated BAM header")
        l_name = struct.unpack_from("<i", h, p)[0]
        if not have(p + 8 + l_name):
            raise ThjError("truncated BAM header")
        targets.append(h[p + 4:p + 4 + l_name].split(b"\0")[0].decode("latin-1"))
        p += 8 + l_name
    m, begin = len(ends), 0                                # right after the members read, unless the first record lies inside one
    for k, e in enumerate(ends):
        if p < e:
            m, begin = k, p - (ends[k - 1] if k else 0)
            break
    return offs, m, begin, targets


def _walk_pieces(self, path_or_bytes, tid2ref, piece_members, call, who):
    """the loop thj_junctions runs over one file: pieces of piece_members BGZF members, each beginning where the one before says it
    stopped; call(piece, more_follows, n, resume_member, resume_skip, the piece's inflated size) -> the ABI call's return code"""
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
        data = bytes(path_or_bytes)
    else:
        with open(path_or_bytes, "rb") as f:
            data = f.read()
    offs, m, skip, _targets = bam_layout(data)
    n_members = len(offs) - 1
    while n_members > m and data[offs[n_members] - 4:offs[n_members]] == bytes(4):
        n_members -= 1                                 # empty members at the end (the EOF marker) hold no records: nothing follows them
    per = piece_members if piece_members else JUNCBED_PIECE_MEMBERS
    if per < 1:
        raise ValueError("piece_members must be at least 1")
    buf = np.frombuffer(data + bytes(64), dtype=np.uint8)
    t2r = np.ascontiguousarray(tid2ref, dtype=np.uint32)
    seen = m
    while m < n_members:
        # every piece covers piece_members members of new ground; what the piece before left out (a read's last run) rides in front
        end, fresh = seen, 0
        while end < n_members and fresh < per:         # (an empty member in the middle of a file is no new ground)
            fresh += data[offs[end + 1] - 4:offs[end + 1]] != bytes(4)
            end += 1
        more = 1 if end < n_members else 0
        piece = CBamPiece(buf.ctypes.data + offs[m], offs[end] - offs[m], skip, len(t2r), t2r.ctypes.data if len(t2r) else None)
        n, rm, rs = C.c_int64(), C.c_uint32(), C.c_uint32()
        inflated = sum(int.from_bytes(data[offs[k + 1] - 4:offs[k + 1]], "little") for k in range(m, end))
        rc = call(piece, more, n, rm, rs, inflated)
        if rc:
            e = ThjError("%s failed (%d): %s" % (who, rc, self.lib.thj_last_error().decode()))
            e.code = rc
            raise e
        if not more:
            break
        m, skip, seen = m + rm.value, rs.value, end


def _reported_methods():
    def bam_contig_names_upload(self, names: Sequence[str]):
        """the run's contig names, names[ref_id - 1]: what a fusion alignment's record names its contigs with"""
        arr = (C.c_char_p * max(1, len(names)))(*[n.encode() for n in names])
        _check(self.lib, self.lib.thj_bam_contig_names_upload(self._ctx, arr, C.c_int32(len(names))), "thj_bam_contig_names_upload")

    def juncbed_add_bam(self, path_or_bytes, tid2ref: Sequence[int], max_report_intron: int, piece_members: Optional[int] = None) -> int:
        """A BAM file of reported alignments (a path, or its bytes) into the consensus, parsed on the device: cut into pieces of
        piece_members BGZF members (default JUNCBED_PIECE_MEMBERS) and handed to thj_juncbed_add_bam piece after piece, each piece
        beginning where the one before says it stopped -- the loop thj_junctions runs.  tid2ref[tid] = contig number of the file's
        target tid, 0 = unknown.  -> records counted.  A ThjError carries the call's return code as .code (-6, THJ_EFALLBACK: the file
        wants the host readers; what earlier pieces added stays added -- reset before reading it another way)."""
        total = [0]

        def call(piece, more, n, rm, rs, _inflated):
            rc = self.lib.thj_juncbed_add_bam(self._ctx, C.byref(piece), C.c_int32(max_report_intron), C.c_int32(more), C.byref(n), C.byref(rm), C.byref(rs))
            if not rc:
                total[0] += n.value
            return rc
        _walk_pieces(self, path_or_bytes, tid2ref, piece_members, call, "thj_juncbed_add_bam")
        return total[0]

    def juncbed_collect_accepted(self, on: bool = True, library_type: int = 1, rg_id: str = "", tid_of_ref: Sequence[int] = (), pairs: bool = False):
        """between juncbed_reset and the first add, after juncbed_best_alignments: the chosen alignments will be written out afterwards
        (juncbed_report_bam).  library_type: Params.library_type's numbers (2 fr-firststrand, 3 fr-secondstrand); tid_of_ref[ref_id - 1] =
        the contig's index in the output header.  pairs: thj_juncbed_collect_accepted_pairs -- the same beside juncbed_pair_alignments
        (either first), for juncbed_report_pairs_bam."""
        t = np.ascontiguousarray(tid_of_ref, dtype=np.int32)
        name = "thj_juncbed_collect_accepted_pairs" if pairs else "thj_juncbed_collect_accepted"
        _check(self.lib, getattr(self.lib, name)(self._ctx, 1 if on else 0, C.c_int32(library_type), C.c_char_p(rg_id.encode()) if rg_id else None,
                                                                C.c_void_p(t.ctypes.data) if len(t) else None, C.c_int32(len(t))), name)

    def juncbed_report_bam(self, path_or_bytes, tid2ref: Sequence[int], max_report_intron: int, piece_members: Optional[int] = None):
        """after juncbed_finish: replays the file exactly as juncbed_add_bam cut it (the same piece_members) and appends the rewritten
        records of its reported alignments to the context's BAM stream -> (their sizes in output order, the stream's length).  Several
        files: one call each, in the order they were added."""
        sizes, total = [], [0]

        def call(piece, more, n, rm, rs, inflated):
            cap = inflated // 36 + 1                        # a record takes its block_size and 32 fixed bytes at least
            buf = np.zeros(cap, dtype=np.uint32)
            tot = C.c_int64()
            rc = self.lib.thj_juncbed_report_bam(self._ctx, C.byref(piece), C.c_int32(max_report_intron), C.c_int32(more), C.byref(n), C.byref(rm), C.byref(rs),
                                                 _ptr(buf), C.c_int64(cap), C.byref(tot))
            if not rc:
                sizes.extend(int(x) for x in buf[:n.value])
                total[0] = tot.value
            return rc
        _walk_pieces(self, path_or_bytes, tid2ref, piece_members, call, "thj_juncbed_report_bam")
        return sizes, total[0]

    def juncbed_report_pairs_bam(self, left_records: Sequence[bytes], right_records: Sequence[bytes], count_only: bool = False):
        """after juncbed_finish of a consensus with juncbed_pair_alignments and juncbed_collect_accepted(pairs=True) both on: once per juncbed_add_pairs[_seq]
        call, in the same order, with the raw BAM records (each behind its block_size field) of exactly the records that call was given, a
        side each.  The rewritten records of the inserts' reported alignments are appended to the context's BAM stream (the first call empties
        it) -> (the stream so far, the sizes of this call's records in output order).  count_only: nothing is appended -> (records, their
        bytes)."""
        def packed(recs):
            off = np.zeros(len(recs) + 1, dtype=np.int64)
            if len(recs):
                off[1:] = np.cumsum([len(r) for r in recs])
            return b"".join(recs), off
        (lb, lo), (rb, ro) = packed(left_records), packed(right_records)
        n, tot = C.c_int64(), C.c_int64()
        args = (self._ctx, C.c_char_p(lb) if lb else None, _ptr(lo), C.c_int64(len(left_records)), C.c_char_p(rb) if rb else None, _ptr(ro), C.c_int64(len(right_records)))
        _check(self.lib, self.lib.thj_juncbed_report_pairs_bam(*args, None, C.c_int64(0), C.byref(n), C.byref(tot)), "thj_juncbed_report_pairs_bam")
        if count_only:
            return n.value, tot.value
        buf = np.zeros(n.value + 1, dtype=np.uint32)
        _check(self.lib, self.lib.thj_juncbed_report_pairs_bam(*args, _ptr(buf), C.c_int64(n.value), C.byref(n), C.byref(tot)), "thj_juncbed_report_pairs_bam")
        return self.bam_stream_download(tot.value), [int(x) for x in buf[:n.value]]

    for f in (bam_contig_names_upload, juncbed_add_bam, juncbed_collect_accepted, juncbed_report_bam, juncbed_report_pairs_bam):
        setattr(Context, f.__name__, f)


_reported_methods()


# ------------------------------------------------------------------ the unmapped-read files and the align-summary counters (thj_unmapped.hip)

ABI_SYMBOLS += ["thj_juncbed_collect_unmapped", "thj_juncbed_read_numbers", "thj_juncbed_report_unmapped_bam", "thj_juncbed_align_stats"]
ALIGN_STATS = ("num_aligned_left", "num_unmapped_left", "num_aligned_left_multi", "num_aligned_left_xmulti",
               "num_aligned_right", "num_unmapped_right", "num_aligned_right_multi", "num_aligned_right_xmulti",
               "num_aligned_pairs", "num_aligned_pairs_multi", "num_aligned_pairs_disc",
               "num_aligned_unpaired", "num_unmapped_unpaired", "num_aligned_unpaired_multi", "num_aligned_unpaired_xmulti")      # SAlignStats' field order


def _unmapped_methods():
    def juncbed_collect_unmapped(self, on: bool = True, max_report_intron: int = 500000):
        """between juncbed_reset and the first add, after juncbed_best_alignments: the reads files will be walked afterwards
        (juncbed_report_unmapped_bam, juncbed_align_stats).  max_report_intron: what concordant() compares an insert's inner distance with."""
        _check(self.lib, self.lib.thj_juncbed_collect_unmapped(self._ctx, 1 if on else 0, C.c_int32(max_report_intron)), "thj_juncbed_collect_unmapped")

    def juncbed_read_numbers(self, numbers: Sequence[int]):
        """right after juncbed_add_records[_seq] / juncbed_add_pairs[_seq] while the unmapped reads are collected: the numbers of that
        call's reads (or inserts) in visit order; they rise strictly across all add calls"""
        a = np.ascontiguousarray(numbers, dtype=np.uint64)
        _check(self.lib, self.lib.thj_juncbed_read_numbers(self._ctx, _ptr(a) if len(a) else None, C.c_int64(len(a))), "thj_juncbed_read_numbers")

    def juncbed_report_unmapped_bam(self, side: int, path_or_bytes, piece_members: Optional[int] = None, count_only: bool = False):
        """after juncbed_finish: one side's reads file (unaligned BAM: a path, or its bytes; side 0 left or only, 1 right), cut into pieces
        of piece_members BGZF members as juncbed_add_bam cuts its input.  The unmapped reads' records are appended to the context's BAM
        stream (a side's first piece empties it) -> (the stream's bytes, the records' sizes).  count_only: nothing is appended or counted
        -> (records, their bytes)."""
        sizes, total, counted = [], [0], [0, 0]

        def call(piece, more, n, rm, rs, inflated):
            cap = inflated // 36 + 1
            buf = None if count_only else np.zeros(cap, dtype=np.uint32)
            tot = C.c_int64()
            rc = self.lib.thj_juncbed_report_unmapped_bam(self._ctx, C.c_int32(side), C.byref(piece), C.c_int32(more), C.byref(n), C.byref(rm), C.byref(rs),
                                                          _ptr(buf), C.c_int64(0 if count_only else cap), C.byref(tot))
            if not rc:
                if count_only:
                    counted[0] += n.value; counted[1] += tot.value
                else:
                    sizes.extend(int(x) for x in buf[:n.value]); total[0] = tot.value
            return rc
        calls = [0]

        def counted_call(*args):
            calls[0] += 1
            return call(*args)
        _walk_pieces(self, path_or_bytes, (), piece_members, counted_call, "thj_juncbed_report_unmapped_bam")
        if not calls[0]:                                    # a reads file without a record: the side ends all the same
            n, rm, rs = C.c_int64(), C.c_uint32(), C.c_uint32()
            rc = call(CBamPiece(None, 0, 0, 0, None), 0, n, rm, rs, 0)
            if rc:
                raise ThjError("thj_juncbed_report_unmapped_bam failed (%d): %s" % (rc, self.lib.thj_last_error().decode()))
        if count_only:
            return counted[0], counted[1]
        return self.bam_stream_download(total[0]), sizes

    def juncbed_align_stats(self) -> List[int]:
        """after every side's reads file has been reported: SAlignStats' fifteen counters in their order (ALIGN_STATS)"""
        a = np.zeros(15, dtype=np.int64)
        _check(self.lib, self.lib.thj_juncbed_align_stats(self._ctx, _ptr(a)), "thj_juncbed_align_stats")
        return [int(x) for x in a]

    for f in (juncbed_collect_unmapped, juncbed_read_numbers, juncbed_report_unmapped_bam, juncbed_align_stats):
        setattr(Context, f.__name__, f)


_unmapped_methods()
