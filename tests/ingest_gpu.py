"""Test-only: ctypes wrappers for the three ingest entry points of libthj_hip.so (thj_ingest_seg_batch, thj_ingest_span_hits,
thj_ingest_span_batch), which the executables call and host.py does not wrap.  Device arrays of a batch come back as numpy arrays
through the HIP runtime's own hipMemcpy, reached in the library this process has already loaded."""
import ctypes as C

import numpy as np

from tophat_amd import host
from tophat_amd.batch import HIT_DTYPE, SPAN_HIT_DTYPE

THJ_OK, THJ_EINVAL, THJ_EFALLBACK = 0, -1, -6
CODES = {"OK": THJ_OK, "EINVAL": THJ_EINVAL, "EFALLBACK": THJ_EFALLBACK}


class Piece(C.Structure):                              # thj_bam_piece
    _fields_ = [("comp", C.c_void_p), ("comp_bytes", C.c_int64), ("first_skip", C.c_uint32), ("n_tid", C.c_int32), ("tid2ref", C.c_void_p)]


def _hip_runtime():
    """the HIP runtime libthj_hip.so brought in: found in this process's own map, so that no second copy is loaded"""
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64" in line:
                return C.CDLL(line.split()[-1])
    raise RuntimeError("libthj_hip.so is loaded but no HIP runtime is mapped")


class Ingest:
    def __init__(self, ctx, params):
        self.ctx, self.lib = ctx, ctx.lib
        self.cp = params.as_ctypes()
        self.hip = _hip_runtime()
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.libc = C.CDLL(None)
        self.libc.free.argtypes = [C.c_void_p]
        self.lib.thj_pinned_free.argtypes = [C.c_void_p]
        self.lib.thj_batch_free.argtypes = [C.c_void_p, C.c_void_p]
        self.lib.thj_span_batch_free.argtypes = [C.c_void_p, C.c_void_p]
        self._keep = []

    def error(self):
        return self.lib.thj_last_error().decode()

    def piece(self, data_skip, tid2ref):
        data, skip = data_skip
        buf = np.frombuffer(bytes(data) + bytes(64), dtype=np.uint8)
        t = np.asarray(tid2ref, dtype=np.uint32)
        self._keep += [buf, t]
        return Piece(buf.ctypes.data, len(data), skip, len(t), t.ctypes.data)

    def pieces(self, list_of_data_skip, tid2ref):
        arr = (Piece * len(list_of_data_skip))(*[self.piece(p, tid2ref) for p in list_of_data_skip])
        self._keep.append(arr)
        return arr

    def d2h(self, ptr, dtype, n):
        out = np.zeros(n, dtype=dtype)
        if n:
            assert ptr
            rc = self.hip.hipMemcpy(out.ctypes.data, ptr, out.nbytes, 2)       # hipMemcpyDeviceToHost
            assert rc == 0, "hipMemcpy: %d" % rc
        return out

    def _host_array(self, ptr, dtype, n, free):
        a = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(n * np.dtype(dtype).itemsize,)).copy().view(dtype) if n else np.zeros(0, dtype)
        if ptr:
            free(ptr)
        return a

    def seg_batch(self, segs, mate_full, mate_last, reads, begin_id, end_id, include_top0, tid2ref):
        """-> (return code, None | dict of the batch's arrays)"""
        nseg = len(segs)
        out, n_reads = C.c_void_p(), C.c_int64()
        rc = self.lib.thj_ingest_seg_batch(self.ctx._ctx, C.byref(self.cp), C.c_int32(nseg), self.pieces(segs, tid2ref),
                                           C.byref(self.piece(mate_full, tid2ref)) if mate_full else None,
                                           C.byref(self.piece(mate_last, tid2ref)) if mate_last else None,
                                           C.byref(self.piece(reads, ())), C.c_uint32(begin_id), C.c_uint32(end_id), C.c_int32(include_top0),
                                           C.c_uint32(0), C.byref(out), C.byref(n_reads))
        self._keep = []
        if rc or not out.value:
            return rc, None
        self.ctx.sync()
        b = host.CSegBatch.from_address(out.value)
        n, W = b.n_reads, b.words_per_plane
        assert n == n_reads.value and b.nseg == nseg
        r = dict(n_reads=n, W=W, seg_off=self.d2h(b.seg_off, np.uint32, n * nseg + 1))
        r["hits"] = self.d2h(b.hits, HIT_DTYPE, int(r["seg_off"][-1]))
        r["planes"] = self.d2h(b.read_planes, np.uint64, n * 3 * W)
        r["read_len"] = self.d2h(b.read_len, np.uint16, n)
        if b.mate_off:
            r["mate_off"] = self.d2h(b.mate_off, np.uint32, n + 1)
            r["mate_hits"] = self.d2h(b.mate_hits, HIT_DTYPE, int(r["mate_off"][-1]))
        assert self.lib.thj_batch_free(self.ctx._ctx, out) == 0
        return rc, r

    def _span(self, segs, reads, begin_id, end_id, tid2ref):
        nseg = len(segs)
        out, row_ids, n_rows = C.c_void_p(), C.c_void_p(), C.c_int64()
        infl, infl_bytes, row_loc = C.c_void_p(), C.c_int64(), C.c_void_p()
        if reads is None:
            rc = self.lib.thj_ingest_span_hits(self.ctx._ctx, C.byref(self.cp), C.c_int32(nseg), self.pieces(segs, tid2ref), C.c_uint32(begin_id),
                                               C.c_uint32(end_id), C.byref(out), C.byref(row_ids), C.byref(n_rows))
        else:
            rc = self.lib.thj_ingest_span_batch(self.ctx._ctx, C.byref(self.cp), C.c_int32(nseg), self.pieces(segs, tid2ref),
                                                C.byref(self.piece(reads, ())), C.c_uint32(begin_id), C.c_uint32(end_id), C.byref(out),
                                                C.byref(row_ids), C.byref(n_rows), C.byref(infl), C.byref(infl_bytes), C.byref(row_loc))
        self._keep = []
        if rc or not out.value:
            return rc, None
        self.ctx.sync()
        b = host.CSpanBatch.from_address(out.value)
        n = b.n_reads
        assert n == n_rows.value and b.nseg == nseg
        r = dict(n_reads=n, read_id=self._host_array(row_ids.value, np.uint32, n, self.libc.free), seg_off=self.d2h(b.seg_off, np.uint32, n * nseg + 1))
        nh = int(r["seg_off"][-1])
        r["hits"] = self.d2h(b.hits, SPAN_HIT_DTYPE, nh)
        r["hit_heads"] = self.d2h(b.hit_heads, np.uint32, nh * 4).reshape(nh, 4)
        if reads is not None:
            W, qs = b.words_per_plane, b.qual_stride
            r.update(W=W, qual_stride=qs, planes=self.d2h(b.read_planes, np.uint64, n * 3 * W), read_len=self.d2h(b.read_len, np.uint16, n),
                     quals=self.d2h(b.quals, np.uint8, n * qs).reshape(n, qs),
                     reads_infl=self._host_array(infl.value, np.uint8, infl_bytes.value, self.lib.thj_pinned_free),
                     row_loc=self._host_array(row_loc.value, np.uint32, n, self.libc.free))
        assert self.lib.thj_span_batch_free(self.ctx._ctx, out) == 0
        return rc, r

    def span_hits(self, segs, begin_id, end_id, tid2ref):
        return self._span(segs, None, begin_id, end_id, tid2ref)

    def span_batch(self, segs, reads, begin_id, end_id, tid2ref):
        return self._span(segs, reads, begin_id, end_id, tid2ref)


def pack_letters(lib, seqs, W):
    """thj_reads_pack on decoded letters, each cut at W * 64 -> the planes (lengths are the caller's: the ingest keeps the full one)"""
    cut = [s[:W * 64] for s in seqs]
    off = np.zeros(len(cut) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(s) for s in cut])
    bases = np.frombuffer(("".join(cut) + "\0").encode(), dtype=np.uint8).copy()
    planes = np.zeros(len(cut) * 3 * W, dtype=np.uint64)
    lens = np.zeros(len(cut), dtype=np.uint16)
    rc = lib.thj_reads_pack(C.c_int64(len(cut)), C.c_void_p(off.ctypes.data), C.c_void_p(bases.ctypes.data), C.c_int32(W),
                            C.c_void_p(planes.ctypes.data), C.c_void_p(lens.ctypes.data))
    assert rc == 0
    return planes
