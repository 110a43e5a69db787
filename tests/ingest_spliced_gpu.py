"""Test-only: ctypes wrappers for the junction-db side of the device ingest (thj_span_juncdb_upload, thj_ingest_span_batch_spliced),
beside ingest_gpu.py's for the three older entry points.  The target table is built in Python from the map's header, field by field
as the executables' juncdb_target_from_name builds it (tests/test_splice_core_cpu.py holds that function to the same expectations)."""
import ctypes as C

import numpy as np

from ingest_gpu import Ingest
from tophat_amd import host
from tophat_amd.batch import SPAN_HIT_DTYPE

THJ_ESTATE = -5
TARGET_DTYPE = np.dtype([("ref_id", "<u4"), ("ref_id2", "<u4"), ("left", "<i4"), ("lsp", "<i4"), ("second", "<i4"), ("type", "u1"), ("strand", "u1"),
                         ("reserved", "<u2")])
assert TARGET_DTYPE.itemsize == 24
JUNC, DEL, INS, FUS, INVALID = range(5)
STRANDS = {"fwd": 0, "rev": 1, "ff": 2, "fr": 3, "rf": 4, "rr": 5}


def target_table(names, ref_ids):
    """thj_juncdb_target per target name; ref_ids: contig name -> id (a contig that is not in it is id 0)"""
    out = np.zeros(len(names), dtype=TARGET_DTYPE)
    for k, name in enumerate(names):
        out[k]["type"], out[k]["strand"] = INVALID, 6
        toks = name.lstrip("|").split("|")
        ne = len(toks) - 6
        if ne < 0:
            continue
        lr = [x for x in toks[ne + 2].split("-") if x]
        if len(lr) != 2:
            continue
        ty, strand = toks[ne + 4], STRANDS.get(toks[ne + 5], 6)
        if ty != "ins" and strand == 6:
            continue
        contig = "|".join(toks[:ne + 1])
        t = INS if ty == "ins" else DEL if ty == "del" else FUS if ty == "fus" else JUNC
        out[k]["strand"], out[k]["left"], out[k]["lsp"] = strand, int(toks[ne + 1]), int(lr[0])
        out[k]["second"] = len(lr[1]) if t == INS else int(lr[1])
        if t == FUS:
            cs = [x for x in contig.split("-") if x]
            if len(cs) != 2:
                continue
            out[k]["ref_id"], out[k]["ref_id2"] = ref_ids.get(cs[0], 0), ref_ids.get(cs[1], 0)
        else:
            out[k]["ref_id"] = ref_ids.get(contig, 0)
        out[k]["type"] = t
    return out


class SplicedIngest(Ingest):
    def upload_targets(self, table):
        table = np.ascontiguousarray(table, dtype=TARGET_DTYPE)
        return self.lib.thj_span_juncdb_upload(self.ctx._ctx, C.c_void_p(table.ctypes.data if len(table) else None), C.c_int64(len(table)))

    def span_batch_spliced(self, segs, spliced, reads, begin_id, end_id, tid2ref, spliced_n_tid=0):
        """-> (return code, None | dict of the batch's arrays); spliced: [(bytes, first_skip)], map s beside segment map s.
        spliced_n_tid: what the spliced pieces claim as n_tid, with a null tid2ref behind it (the call must look at neither)"""
        nseg = len(segs)
        sp = self.pieces(spliced, ()) if spliced else None
        for k in range(len(spliced)):
            sp[k].n_tid, sp[k].tid2ref = spliced_n_tid, None
        out, row_ids, n_rows = C.c_void_p(), C.c_void_p(), C.c_int64()
        rc = self.lib.thj_ingest_span_batch_spliced(self.ctx._ctx, C.byref(self.cp), C.c_int32(nseg), self.pieces(segs, tid2ref), C.c_int32(len(spliced)),
                                                    sp,
                                                    C.byref(self.piece(reads, ())) if reads is not None else None, C.c_uint32(begin_id), C.c_uint32(end_id),
                                                    C.byref(out), C.byref(row_ids), C.byref(n_rows), None, None, None)
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
                     quals=self.d2h(b.quals, np.uint8, n * qs).reshape(n, qs))
        assert self.lib.thj_span_batch_free(self.ctx._ctx, out) == 0
        return rc, r
