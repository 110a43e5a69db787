"""Test-only: SplicedIngest (ingest_spliced_gpu.py) with the switch that lets the device ingest splice fusion contigs
(thj_span_juncdb_fusion_contigs), and what the fusion-contig tests share: a planted map as one piece, the host driver's row / CSR
layout restated, the comparison of a batch with it."""
import ctypes as C
import gzip

import numpy as np

import splice_cases as sc
from ingest_spliced_gpu import SplicedIngest


class FusedIngest(SplicedIngest):
    def fusion_contigs(self, on):
        return self.lib.thj_span_juncdb_fusion_contigs(self.ctx._ctx, C.c_int32(1 if on else 0))


def whole(bam):
    """(bytes, first_skip) of a whole BAM file made by write_bam_from_sam: one member holds the header and the records"""
    data = open(bam, "rb").read()
    infl = gzip.decompress(data)
    l_text = int.from_bytes(infl[4:8], "little")
    n_ref = int.from_bytes(infl[8 + l_text:12 + l_text], "little")
    p = 12 + l_text
    for _ in range(n_ref):
        p += 4 + int.from_bytes(infl[p:p + 4], "little") + 4
    assert len(infl) <= 0xFF00, "the planted maps fit one BGZF member"
    return data, p


def layout(contig_hits, spliced_hits, begin_id, end_id):
    """the host driver's loop: rows = ids with a first-segment group in either stream, in id order; per segment the contig group, then
    the spliced group, each in file order.  *_hits[s] = [HitRec] in file order -> (row ids, seg_off, hits)"""
    def groups(hs):
        g = {}
        for h in hs:
            if h[0] and begin_id <= h[0] < end_id:
                g.setdefault(h[0], []).append(h)
        return g
    cg, sg = [groups(h) for h in contig_hits], [groups(h) for h in spliced_hits]
    ids = sorted(set(cg[0]) | (set(sg[0]) if sg else set()))
    seg_off, hits = [0], []
    for rid in ids:
        for s in range(len(cg)):
            hits += cg[s].get(rid, []) + (sg[s].get(rid, []) if s < len(sg) else [])
            seg_off.append(len(hits))
    return np.array(ids, dtype=np.uint32), np.array(seg_off, dtype=np.uint32), sc.hits_array(hits)


def same_batch(got, want, what):
    ids, seg_off, hits = want
    if len(ids) == 0:
        assert got is None, what
        return
    assert got is not None and got["n_reads"] == len(ids), what
    assert got["read_id"].tolist() == ids.tolist(), what
    assert got["seg_off"].tolist() == seg_off.tolist(), what
    for k in range(len(hits)):                         # record-wise: the first difference with its fields
        assert got["hits"][k].tobytes() == hits[k].tobytes(), "%s: hit %d is %r, the restatement gives %r" % (what, k, got["hits"][k], hits[k])
    assert len(got["hits"]) == len(hits)
    assert got["hit_heads"].tobytes() == np.ascontiguousarray(hits.view(np.uint32).reshape(-1, 8)[:, :4]).tobytes(), what + ": hit heads"
