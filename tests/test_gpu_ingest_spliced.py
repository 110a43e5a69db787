"""GPU: junction-db ("spliced") segment maps through the device-side ingest (thj_k_parse's third file kind over
thj_splice_core.h, the merge by read id with a contig map and a spliced map per segment) by way of thj_ingest_span_batch_spliced:
the planted records of splice_cases.py against the Python restatement of the spliced hit factory, hit by hit, and a merge table
against the row / CSR layout of the host driver's loop (long_spanning_reads.cpp:2706-2765, :125-147), restated here."""
import numpy as np
import pytest

import ingest_cases as ic
import splice_cases as sc
from tophat_amd import host
from tophat_amd.bamio import read_bam
from tophat_amd.params import Params
from tophat_amd.samtext import parse_sam_hits

pytestmark = pytest.mark.gpu
NSEG = 4
T2R_MERGE = (1, 2)                                     # the merge table's contig maps name chr1, chr2


@pytest.fixture(scope="module")
def ing():
    from ingest_spliced_gpu import SplicedIngest
    with host.Context(0) as ctx:
        yield SplicedIngest(ctx, Params(max_report_intron=ic.MAX_INTRON, segment_length=25))


def whole(bam):
    """(bytes, first_skip) of a whole BAM file made by write_bam_from_sam: one member holds the header and the records"""
    data = open(bam, "rb").read()
    import gzip
    infl = gzip.decompress(data)
    l_text = int.from_bytes(infl[4:8], "little")
    n_ref = int.from_bytes(infl[8 + l_text:12 + l_text], "little")
    p = 12 + l_text
    for _ in range(n_ref):
        p += 4 + int.from_bytes(infl[p:p + 4], "little") + 4
    assert len(infl) <= 0xFF00, "the planted maps fit one BGZF member"
    return data, p


def empty_map():
    return ic.write_bam(None, [([], 6)], targets=(("chr1", 1000000), ("chr2", 1000000))).piece()


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


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("planted"))
    cs = sc.cases()
    quiet = [c for c in cs if c[1] in (sc.KEPT, sc.DROPPED)]
    return dict(cases=cs, quiet=sc.write_map(d, "quiet", [c[3] for c in quiet]),
                six=sc.write_map(d, "six", [c[3] for c in cs if c[1] in (sc.KEPT, sc.SIX_OPS)][-3:]),
                fus=sc.write_map(d, "fus", [c[3] for c in cs if c[1] in (sc.KEPT, sc.FALLBACK)][-3:]))


def test_without_the_target_table(ing, planted):
    """THJ_ESTATE: spliced maps and no thj_span_juncdb_upload before them"""
    assert ing.upload_targets(np.zeros(0, dtype=np.uint8)) == 0
    rc, got = ing.span_batch_spliced([empty_map()] * NSEG, [whole(planted["quiet"][1])], None, sc.BEGIN_ID, sc.END_ID, T2R_MERGE)
    from ingest_spliced_gpu import THJ_ESTATE
    assert rc == THJ_ESTATE and got is None and "thj_span_juncdb_upload" in ing.error()


def test_planted_records(ing, planted):
    from ingest_spliced_gpu import target_table
    assert ing.upload_targets(target_table(sc.TARGETS, sc.REF_IDS)) == 0
    sam, bam = planted["quiet"]
    rc, got = ing.span_batch_spliced([empty_map()] * NSEG, [whole(bam)], None, sc.BEGIN_ID, sc.END_ID, T2R_MERGE)
    assert rc == 0, ing.error()
    want = sc.restated(sam)
    kept = {c[2] for c in planted["cases"] if c[1] == sc.KEPT}
    assert {h[0] for h in want} == kept, "the restatement keeps exactly the records planted as kept"
    same_batch(got, layout([[]] * NSEG, [want], sc.BEGIN_ID, sc.END_ID), "planted records")
    assert got["hits"]["n_cigar"].max() == 5 and (got["hits"]["flags"] & 4).any()


def test_spliced_pieces_tid2ref_is_not_looked_at(ing, planted):
    """a junction database has millions of targets: the table lives on the context, and a spliced piece's own n_tid / tid2ref are
    neither read nor sent up -- here a piece that claims 200 million targets behind a null pointer gives the same batch"""
    from ingest_spliced_gpu import target_table
    assert ing.upload_targets(target_table(sc.TARGETS, sc.REF_IDS)) == 0
    bam = planted["quiet"][1]
    rc1, a = ing.span_batch_spliced([empty_map()] * NSEG, [whole(bam)], None, sc.BEGIN_ID, sc.END_ID, T2R_MERGE)
    rc2, b = ing.span_batch_spliced([empty_map()] * NSEG, [whole(bam)], None, sc.BEGIN_ID, sc.END_ID, T2R_MERGE, spliced_n_tid=200 * 1000 * 1000)
    assert rc1 == 0 and rc2 == 0, ing.error()
    for k in ("read_id", "seg_off", "hits", "hit_heads"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert len(b["hits"]) > 30


def test_loud_outcomes(ing, planted):
    from ingest_spliced_gpu import target_table
    assert ing.upload_targets(target_table(sc.TARGETS, sc.REF_IDS)) == 0
    rc, got = ing.span_batch_spliced([empty_map()] * NSEG, [whole(planted["fus"][1])], None, sc.BEGIN_ID, sc.END_ID, T2R_MERGE)
    assert rc == -6 and got is None                    # THJ_EFALLBACK: the host factory takes the shard
    assert "fusion contigs" in ing.error()
    rc, got = ing.span_batch_spliced([empty_map()] * NSEG, [whole(planted["six"][1])], None, sc.BEGIN_ID, sc.END_ID, T2R_MERGE)
    assert rc == -1 and got is None and "more than 5 CIGAR" in ing.error()           # THJ_EINVAL, the contig path's message (ingest_cases.loud_cases)
    # ... and the context takes the next shard
    rc, got = ing.span_batch_spliced([empty_map()] * NSEG, [whole(planted["quiet"][1])], None, sc.BEGIN_ID, sc.END_ID, T2R_MERGE)
    assert rc == 0 and got is not None


@pytest.fixture(scope="module")
def merge(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("merge"))
    contig, spliced = sc.merge_maps(d)
    ids = sorted(set(sc.MERGE_CONTIG) | set(sc.MERGE_SPLICED))
    reads = ic.write_bam(None, [([ic.merge_read(i) for i in ids], 6)])
    return contig, spliced, reads


@pytest.mark.parametrize("with_reads", [False, True], ids=["hits", "with_reads"])
def test_merge_table(ing, merge, with_reads):
    from ingest_spliced_gpu import target_table
    contig, spliced, reads = merge
    assert ing.upload_targets(target_table(sc.TARGETS, sc.REF_IDS)) == 0
    chits = [list(parse_sam_hits(sam, {"chr1": 1, "chr2": 2})) for sam, _ in contig]
    # the contig factory's hits in thj_span_hit form: plain 25M
    chits = [[(h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7], h[8]) for h in hs] for hs in chits]
    rows_seen = set()
    for begin_id, end_id in sc.MERGE_WINDOWS:
        shits = [sc.restated(sam, begin_id, end_id) for sam, _ in spliced]
        want = layout(chits, shits, begin_id, end_id)
        rc, got = ing.span_batch_spliced([whole(b) for _, b in contig], [whole(b) for _, b in spliced], reads.piece() if with_reads else None,
                                         begin_id, end_id, T2R_MERGE)
        assert rc == 0, ing.error()
        same_batch(got, want, "window [%d, %d)" % (begin_id, end_id))
        rows_seen |= set(want[0].tolist())
        if with_reads and got is not None:
            assert got["read_len"].tolist() == [30 + i % 40 for i in want[0].tolist()]
    # the table's own claims: spliced-only rows, no row without a first-segment hit, the ends of the id range from the spliced map
    assert {18, 22, 32, 40} <= rows_seen and not rows_seen & {24, 26, 28, 29, 36}


def test_no_spliced_maps_equals_span_batch(ing, tmp_path):
    """n_spliced = 0: what thj_ingest_span_batch returns on ingest_cases.merge_table"""
    t = ic.merge_table()
    segs = [t.segs[s].piece(t.seg_start[s]) for s in range(3)]
    for begin_id, end_id in ((100, 500122), (95, 500200), (1, 104)):
        rc1, a = ing.span_batch(segs, t.reads.piece(), begin_id, end_id, ic.TID2REF)
        rc2, b = ing.span_batch_spliced(segs, [], t.reads.piece(), begin_id, end_id, ic.TID2REF)
        assert rc1 == 0 and rc2 == 0, ing.error()
        assert (a is None) == (b is None)
        if a is None:
            continue
        for k in ("read_id", "seg_off", "hits", "hit_heads", "planes", "read_len", "quals"):
            assert a[k].tobytes() == b[k].tobytes(), k
        assert a["n_reads"] == b["n_reads"] and a["n_reads"] > 0
