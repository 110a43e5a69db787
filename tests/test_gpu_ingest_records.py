"""GPU: the device-side ingest (thj_ingest.hip: thj_k_walk, thj_k_parse / parse_hit, thj_k_compact, the merge by read id,
thj_k_read_planes) through its three C entry points, on hand-made BAM files (ingest_cases.py), against the reference's reading
of the same bytes (ingest_ref.py) merged by the project's model of look_for_hit_group (batch.build_seg_batch / build_span_batch).
Every comparison is exact equality of integer arrays."""
import numpy as np
import pytest

import ingest_cases as ic
import ingest_ref as ir
from tophat_amd import host
from tophat_amd.batch import build_seg_batch, build_span_batch
from tophat_amd.params import Params

pytestmark = pytest.mark.gpu
T2R = ic.TID2REF
N_LETTER = {c: (c if c in "ACGT" else "N") for c in ir.SEQ_LETTERS}          # anything but A, C, G, T is N to the planes


@pytest.fixture(scope="module")
def ing():
    from ingest_gpu import Ingest
    with host.Context(0) as ctx:
        yield Ingest(ctx, Params(max_report_intron=ic.MAX_INTRON))


def same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, "%s: %s %s against %s %s" % (what, got.dtype, got.shape, want.dtype, want.shape)
    if got.tobytes() != want.tobytes():
        g, w = got.reshape(len(got), -1).view(np.uint8).reshape(len(got), -1), want.reshape(len(want), -1).view(np.uint8).reshape(len(want), -1)
        k = int(np.flatnonzero((g != w).any(axis=1))[0])
        raise AssertionError("%s: entry %d is %r, the reference reading gives %r" % (what, k, got[k], want[k]))


def hits_of(recs, begin_id, end_id):
    return ir.kept_hits(recs, T2R, ic.MAX_INTRON, begin_id, end_id)


def letters(seq):
    return "".join(N_LETTER[c] for c in seq)


def check_seg(ing, got, seg_recs, reads, begin_id, end_id, include_top0, mate_full=None, mate_last=None):
    """the device batch against the model over the reference reading; returns the model"""
    from ingest_gpu import pack_letters
    want = build_seg_batch([hits_of(r, begin_id, end_id) for r in seg_recs], {i: letters(s) for i, (s, _q) in reads.items()},
                           None if mate_full is None else hits_of(mate_full, begin_id, end_id),
                           None if mate_last is None else hits_of(mate_last, begin_id, end_id), include_top0=bool(include_top0))
    if want.n_reads == 0:
        assert got is None
        return want
    assert got is not None and got["n_reads"] == want.n_reads
    same(got["seg_off"], want.seg_off, "seg_off")
    same(got["hits"], want.hits, "hits")
    seqs = [want.read_seq(r) for r in range(want.n_reads)]
    same(got["planes"], pack_letters(ing.lib, seqs, got["W"]), "read planes")
    same(got["read_len"], np.array([len(s) for s in seqs], dtype=np.uint16), "read lengths")
    if mate_full is not None or mate_last is not None:
        same(got["mate_off"], want.mate_off, "mate_off")
        same(got["mate_hits"], want.mate_hits, "mate hits")
    return want


def check_span(got, seg_recs, reads, begin_id, end_id):
    want = build_span_batch([hits_of(r, begin_id, end_id) for r in seg_recs], {i: "" for i in reads}, {i: "" for i in reads})
    if want.n_reads == 0:
        assert got is None
        return want
    assert got is not None and got["n_reads"] == want.n_reads
    same(got["read_id"], want.read_id, "row ids")
    same(got["seg_off"], want.seg_off, "seg_off")
    same(got["hits"], want.hits, "span hits")
    same(got["hit_heads"], want.hits.view(np.uint32).reshape(-1, 8)[:, :4], "hit heads")
    return want


def check_span_reads(ing, got, want, reads_w, reads):
    """planes, lengths, quality strings and the rows' own records of a thj_ingest_span_batch"""
    from ingest_gpu import pack_letters
    ids = [int(i) for i in want.read_id]
    W, qs = got["W"], got["qual_stride"]
    same(got["planes"], pack_letters(ing.lib, [letters(reads[i][0]) for i in ids], W), "read planes")
    same(got["read_len"], np.array([len(reads[i][0]) for i in ids], dtype=np.uint16), "read lengths")
    q = np.zeros((len(ids), qs), dtype=np.uint8)
    for r, i in enumerate(ids):
        qual = reads[i][1][:qs]
        q[r, :len(qual)] = np.frombuffer(qual, dtype=np.uint8)
    same(got["quals"], q, "quality strings")
    # row_loc: member << 16 | offset of the block_size field of the record that IS the read (the first of its id that is no QC failure)
    where = {}
    for m, off, c in reads_w.chunks:
        rid, _s, _q, qc = ir.read_from_record(c[4:])
        if not qc and rid not in where:
            where[rid] = ((m << 16) | off, c)
    same(got["row_loc"], np.array([where[i][0] for i in ids], dtype=np.uint32), "row_loc")
    infl = got["reads_infl"].tobytes()
    for i in ids:
        loc, c = where[i]
        assert infl[loc:loc + len(c)] == c, "reads_infl at the record of read %d" % i


# ---------------------------------------------------------------------------------------------------------------- parser table
@pytest.fixture(scope="module")
def parser():
    recs = [r for _, r in ic.parser_records()]
    top = ic.FIRST_RUNNING_ID + len(recs)
    table = ic.write_bam(None, [(recs[:60], 6), (recs[60:], 0)])
    plain = ic.write_bam(None, [([ic.plain_hit(7, 50), ic.plain_hit(12, 60), ic.plain_hit(12, 61, flag=16), ic.plain_hit(top + 5, 70)], 6)])
    ids = [7] + list(range(ic.FIRST_RUNNING_ID, top + 6))
    reads = ic.write_bam(None, [([ic.plain_read(i, seq=("ACGTN" * 5)[i % 5:] + "ACGT"[:i % 4]) for i in ids], 6)])
    return table, plain, reads


@pytest.mark.parametrize("include_top0", [0, 1])
def test_parser_table_seg_batch(ing, parser, include_top0):
    table, plain, reads = parser
    rc, got = ing.seg_batch([plain.piece(), table.piece()], None, None, reads.piece(), 1, 0xFFFFFFFF, include_top0, T2R)
    assert rc == 0, ing.error()
    want = check_seg(ing, got, [plain.records_from(0), table.records_from(0)], ir.reads_of(reads.records_from(0)), 1, 0xFFFFFFFF, include_top0)
    assert want.n_reads > 100 and len(want.seg_hits(0, 1)) == 8          # the group of id 7: nine names, one of them id 0


def test_parser_table_span_hits(ing, parser):
    table, plain, reads = parser
    rc, got = ing.span_hits([table.piece(), plain.piece()], 1, 0xFFFFFFFF, T2R)
    assert rc == 0, ing.error()
    want = check_span(got, [table.records_from(0), plain.records_from(0)], ir.reads_of(reads.records_from(0)), 1, 0xFFFFFFFF)
    flags = want.hits["flags"]
    assert (flags & 4).sum() >= 4 and want.hits["n_cigar"].max() == 5     # antisense-splice hits and five-op records are in it


# ---------------------------------------------------------------------------------------------------------------- layout table
@pytest.fixture(scope="module")
def layout():
    return ic.layout_table()


def test_layout_whole_and_in_three_shards(ing, layout):
    hits, reads = layout.hits, layout.reads
    rd = ir.reads_of(reads.records_from(0))
    rc, whole = ing.seg_batch([hits.piece()], None, None, reads.piece(), 1, 0xFFFFFFFF, 1, T2R)
    assert rc == 0, ing.error()
    want = check_seg(ing, whole, [hits.records_from(0)], rd, 1, 0xFFFFFFFF, 1)
    assert want.n_reads == len(set(layout.hit_ids)) and len(want.hits) == len(layout.hit_ids)        # every planted record is a hit
    parts = []
    for chunk, b, e in layout.shards:
        rc, got = ing.seg_batch([hits.piece(chunk)], None, None, reads.piece(), b, e, 1, T2R)
        assert rc == 0, ing.error()
        check_seg(ing, got, [hits.records_from(chunk or 0)], rd, b, e, 1)
        parts.append(got)
    assert sum(p["n_reads"] for p in parts) == whole["n_reads"]
    base = np.cumsum([0] + [len(p["hits"]) for p in parts])
    same(np.concatenate([parts[0]["seg_off"]] + [p["seg_off"][1:] + np.uint32(base[k + 1]) for k, p in enumerate(parts[1:])]), whole["seg_off"], "seg_off of the shards")
    for key in ("hits", "planes", "read_len"):
        same(np.concatenate([p[key] for p in parts]), whole[key], key + " of the shards")


def test_layout_span_hits(ing, layout):
    rc, got = ing.span_hits([layout.hits.piece()], 1, 0xFFFFFFFF, T2R)
    assert rc == 0, ing.error()
    check_span(got, [layout.hits.records_from(0)], {i: ("", b"") for i in set(layout.hit_ids)}, 1, 0xFFFFFFFF)


def test_a_record_across_two_members_is_handed_back(ing, layout):
    from ingest_gpu import THJ_EFALLBACK
    rc, got = ing.seg_batch([layout.straddle.piece()], None, None, layout.reads.piece(), 1, 0xFFFFFFFF, 1, T2R)
    assert rc == THJ_EFALLBACK and got is None and "straddle" in ing.error()


# ---------------------------------------------------------------------------------------------------------------- merge table
@pytest.fixture(scope="module")
def merge():
    return ic.merge_table()


def _merge_inputs(m):
    pieces = [m.segs[s].piece(m.seg_start[s] or None) for s in range(3)]
    recs = [m.segs[s].records_from(m.seg_start[s]) for s in range(3)]
    return pieces, recs


@pytest.mark.parametrize("begin_id,end_id,include_top0", ic.MERGE_CALLS)
def test_merge_seg_batch(ing, merge, begin_id, end_id, include_top0):
    pieces, recs = _merge_inputs(merge)
    rc, got = ing.seg_batch(pieces, merge.mate_full.piece(), merge.mate_last.piece(), merge.reads.piece(), begin_id, end_id, include_top0, T2R)
    assert rc == 0, ing.error()
    want = check_seg(ing, got, recs, ir.reads_of(merge.reads.records_from(0)), begin_id, end_id, include_top0,
                     merge.mate_full.records_from(0), merge.mate_last.records_from(0))
    ids = [int(i) for i in want.read_id]
    assert 0 not in ids and all(begin_id <= i < end_id for i in ids)
    if (begin_id, end_id) == (100, 500122):
        assert ids[0] == 100 and ids[-1] == 500121 and (101 in ids) == bool(include_top0) and 102 in ids
        assert [len(want.seg_hits(ids.index(i), 1)) for i in (110, 111, 112, 113, 114, 115)] == [1, 2, 63, 64, 65, 300]
        mate = dict(zip(ids, np.diff(want.mate_off)))
        assert (mate[100], mate[112], mate[113], mate[103], mate[102], mate[500120]) == (2, 3, 65, 1, 0, 1)    # whole-read map first, else last segment


@pytest.mark.parametrize("one_mate_map", ["full", "last"])
def test_merge_seg_batch_with_one_mate_map(ing, merge, one_mate_map):
    pieces, recs = _merge_inputs(merge)
    mf = merge.mate_full if one_mate_map == "full" else None
    ml = merge.mate_last if one_mate_map == "last" else None
    rc, got = ing.seg_batch(pieces, mf and mf.piece(), ml and ml.piece(), merge.reads.piece(), 100, 500122, 0, T2R)
    assert rc == 0, ing.error()
    check_seg(ing, got, recs, ir.reads_of(merge.reads.records_from(0)), 100, 500122, 0, mf and mf.records_from(0), ml and ml.records_from(0))


@pytest.mark.parametrize("begin_id,end_id", [(100, 500122), (0, 104)])
def test_merge_span_batch(ing, merge, begin_id, end_id):
    pieces, recs = _merge_inputs(merge)
    reads = ir.reads_of(merge.reads.records_from(0))
    rc, got = ing.span_batch(pieces, merge.reads.piece(), begin_id, end_id, T2R)
    assert rc == 0, ing.error()
    want = check_span(got, recs, reads, begin_id, end_id)
    ids = [int(i) for i in want.read_id]
    assert 102 not in ids and 0 not in ids and 101 in ids               # hits in segments 1 and 2 only: no row on the spanning side
    check_span_reads(ing, got, want, merge.reads, reads)
    rc, got = ing.span_hits(pieces, begin_id, end_id, T2R)
    assert rc == 0, ing.error()
    check_span(got, recs, reads, begin_id, end_id)


def test_a_missing_read_is_an_error(ing, merge):
    from ingest_gpu import THJ_EINVAL
    pieces, _ = _merge_inputs(merge)
    rc, got = ing.seg_batch(pieces, None, None, merge.reads_missing.piece(), 100, 500122, 0, T2R)
    assert rc == THJ_EINVAL and got is None and "could not get a read" in ing.error()
    rc, got = ing.span_batch(pieces, merge.reads_missing.piece(), 100, 500122, T2R)
    assert rc == THJ_EINVAL and got is None and "could not get a read" in ing.error()


# ---------------------------------------------------------------------------------------------------------------- reads table
def test_reads_table(ing):
    p = Params()
    W = max(1, (p.segment_length * (ic.READS_NSEG + 1) - 1 + 63) // 64)
    t = ic.reads_table(W=W)
    reads = ir.reads_of(t.reads.records_from(0))
    lens = sorted(len(s) for s, _q in reads.values())
    assert lens[0] == 0 and lens[-1] > W * 64 and W * 64 in lens
    assert {c for s, _q in reads.values() for c in s} == set(ir.SEQ_LETTERS)
    recs = [w.records_from(0) for w in t.segs]
    rc, got = ing.seg_batch([w.piece() for w in t.segs], None, None, t.reads.piece(), 1, 0xFFFFFFFF, 0, T2R)
    assert rc == 0, ing.error()
    assert got["W"] == W
    want = check_seg(ing, got, recs, reads, 1, 0xFFFFFFFF, 0)
    assert want.n_reads == len(t.ids)
    rc, got = ing.span_batch([w.piece() for w in t.segs], t.reads.piece(), 1, 0xFFFFFFFF, T2R)
    assert rc == 0, ing.error()
    assert got["W"] == W and got["qual_stride"] == (p.segment_length * (ic.READS_NSEG + 1) + 3) // 4 * 4
    check_span_reads(ing, got, check_span(got, recs, reads, 1, 0xFFFFFFFF), t.reads, reads)


# ---------------------------------------------------------------------------------------------------------------- loud failures
@pytest.mark.parametrize("case", ic.loud_cases(), ids=lambda c: c[0])
def test_loud_failures(ing, case):
    from ingest_gpu import CODES
    label, rec, code, piece_of_message = case
    w = ic.write_bam(None, ic.loud_members(rec))
    rc, got = ing.span_hits([w.piece()], 1, 0xFFFFFFFF, T2R)
    assert rc == CODES[code] and got is None and piece_of_message in ing.error(), (label, rc, ing.error())
    rc, got = ing.seg_batch([w.piece()], None, None, ic.write_bam(None, [([ic.plain_read(i) for i in (19, 20, 21)], 6)]).piece(), 1, 0xFFFFFFFF, 1, T2R)
    assert rc == CODES[code] and got is None and piece_of_message in ing.error(), (label, rc, ing.error())


def test_more_than_eight_segments_go_to_the_host_readers(ing):
    from ingest_gpu import THJ_EFALLBACK
    w = ic.write_bam(None, [([ic.plain_hit(5, 100)], 6)])
    rc, got = ing.seg_batch([w.piece()] * 9, None, None, w.piece(), 1, 0xFFFFFFFF, 1, T2R)
    assert rc == THJ_EFALLBACK and got is None and "more than eight segments" in ing.error()
