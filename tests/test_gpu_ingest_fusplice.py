"""GPU: fusion-contig records of junction-db ("spliced") segment maps through the device-side ingest (thj_k_parse's instantiation
with the fusion branch of thj_splice_core.h, switched on per target table by thj_span_juncdb_fusion_contigs): the planted records
of fusplice_cases.py against the Python restatement of the spliced hit factory, hit by hit and hit head by hit head; the switch's
life; the loud outcome; and a merge table whose spliced maps alternate between junction and fusion targets, against the row / CSR
layout of the host driver's loop -- compaction, the merge by read id and the scatter carry a fused hit's 32 bytes as they are."""
import numpy as np
import pytest

import fusplice_cases as fc
import ingest_cases as ic
import splice_cases as sc
from tophat_amd import host
from tophat_amd.params import Params
from tophat_amd.samtext import parse_sam_hits

pytestmark = pytest.mark.gpu
NSEG = 4
T2R_MERGE = (1, 2)                                     # the merge table's contig maps name chr1, chr2
THJ_EINVAL, THJ_ESTATE, THJ_EFALLBACK = -1, -5, -6


@pytest.fixture(scope="module")
def ing():
    from ingest_fusplice_gpu import FusedIngest
    with host.Context(0) as ctx:
        yield FusedIngest(ctx, Params(max_report_intron=ic.MAX_INTRON, segment_length=25))


def empty_map():
    return ic.write_bam(None, [([], 6)], targets=(("chr1", 1000000), ("chr2", 1000000))).piece()


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("fusplanted"))
    cs = fc.cases()
    quiet = [c for c in cs if c[1] != fc.LOUD]
    kept = [c[3] for c in cs if c[1] == fc.KEPT]
    loud = {c[0]: fc.write_map(d, "loud_" + c[0], kept[:2] + [c[3]] + kept[2:4], fc.TARGETS) for c in cs if c[1] == fc.LOUD}
    return dict(cases=cs, quiet=fc.write_map(d, "quiet", [c[3] for c in quiet], fc.TARGETS), loud=loud)


def table(names=fc.TARGETS):
    from ingest_spliced_gpu import target_table
    return target_table(names, fc.REF_IDS)


def run_map(ing, bam):
    from ingest_fusplice_gpu import whole
    return ing.span_batch_spliced([empty_map()] * NSEG, [whole(bam)], None, fc.BEGIN_ID, fc.END_ID, T2R_MERGE)


def test_without_a_table(ing):
    assert ing.upload_targets(np.zeros(0, dtype=np.uint8)) == 0
    assert ing.fusion_contigs(True) == THJ_ESTATE and "thj_span_juncdb_upload" in ing.error()
    assert ing.fusion_contigs(False) == THJ_ESTATE


def test_planted_quiet_records(ing, planted):
    from ingest_fusplice_gpu import layout, same_batch
    assert ing.upload_targets(table()) == 0 and ing.fusion_contigs(True) == 0
    sam, bam = planted["quiet"]
    rc, got = run_map(ing, bam)
    assert rc == 0, ing.error()
    want = fc.restated(sam)
    assert {h[0] for h in want} == {c[2] for c in planted["cases"] if c[1] == fc.KEPT}, "the restatement keeps exactly the records planted as kept"
    same_batch(got, layout([[]] * NSEG, [want], fc.BEGIN_ID, fc.END_ID), "planted fusion-contig records")
    fused = got["hits"][(got["hits"]["flags"] & fc.FUSED) != 0]
    assert len(fused) == len(want) - 1 and (fused["cigar"][:, 4] == 2).all() and (fused["n_cigar"] == 3).all()
    assert set((fused["cigar"][:, 1] >> 28).tolist()) == {7, 8, 9, 10}, "a hit of each direction"
    assert not (fused["flags"] & 4).any()
    plain = got["hits"][(got["hits"]["flags"] & fc.FUSED) == 0]
    assert len(plain) == 1 and plain["cigar"][0, 4] == 0


def test_switch_off_hands_the_shard_back(ing, planted):
    assert ing.upload_targets(table()) == 0
    rc, got = run_map(ing, planted["quiet"][1])                  # a fresh table: off
    assert rc == THJ_EFALLBACK and got is None and "fusion contigs" in ing.error()
    assert ing.fusion_contigs(True) == 0 and ing.fusion_contigs(False) == 0
    rc, got = run_map(ing, planted["quiet"][1])
    assert rc == THJ_EFALLBACK and got is None and "fusion contigs" in ing.error()


def test_a_new_upload_turns_the_switch_off(ing, planted):
    assert ing.upload_targets(table()) == 0 and ing.fusion_contigs(True) == 0
    rc, got = run_map(ing, planted["quiet"][1])
    assert rc == 0 and got is not None
    assert ing.upload_targets(table()) == 0
    rc, got = run_map(ing, planted["quiet"][1])
    assert rc == THJ_EFALLBACK and got is None and "fusion contigs" in ing.error()


def test_loud_records(ing, planted):
    """a fused hit's fifth operation: THJ_EINVAL with the contig path's message, as the host factory ends the run there; the record on a
    target whose second contig is unknown is dropped before its operations are counted (it is in the quiet map)"""
    assert ing.upload_targets(table()) == 0 and ing.fusion_contigs(True) == 0
    assert len(planted["loud"]) == 13
    for label, (_sam, bam) in planted["loud"].items():
        rc, got = run_map(ing, bam)
        assert rc == THJ_EINVAL and got is None and "more than 5 CIGAR" in ing.error(), label
    # ... and the context takes the next shard
    rc, got = run_map(ing, planted["quiet"][1])
    assert rc == 0 and got is not None


def test_table_without_fusion_targets_runs_what_it_ran_before(ing, tmp_path):
    """the switch on a table that has no THJ_JUNCDB_FUS target changes nothing: splice_cases' quiet map, byte for byte"""
    names = tuple(t for t in sc.TARGETS if t != sc.FUS)
    assert names == sc.TARGETS[:-1], "the other targets keep their numbers"
    quiet = [c[3] for c in sc.cases() if c[1] in (sc.KEPT, sc.DROPPED)]
    _sam, bam = sc.write_map(str(tmp_path), "quiet", quiet, names)
    got = []
    for on in (False, True):
        assert ing.upload_targets(table(names)) == 0 and ing.fusion_contigs(on) == 0
        rc, b = run_map(ing, bam)
        assert rc == 0, ing.error()
        got.append(b)
    for k in ("read_id", "seg_off", "hits", "hit_heads"):
        assert got[0][k].tobytes() == got[1][k].tobytes(), k
    assert len(got[0]["hits"]) > 30 and got[0]["n_reads"] == got[1]["n_reads"]


@pytest.fixture(scope="module")
def merge(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("fusmerge"))
    contig, spliced = fc.merge_maps(d)
    ids = sorted(set(sc.MERGE_CONTIG) | set(sc.MERGE_SPLICED))
    reads = ic.write_bam(None, [([ic.merge_read(i) for i in ids], 6)])
    return contig, spliced, reads


@pytest.mark.parametrize("with_reads", [False, True], ids=["hits", "with_reads"])
def test_merge_table(ing, merge, with_reads):
    from ingest_fusplice_gpu import layout, same_batch, whole
    contig, spliced, reads = merge
    assert ing.upload_targets(table()) == 0 and ing.fusion_contigs(True) == 0
    chits = [[tuple(h[:9]) for h in parse_sam_hits(sam, {"chr1": 1, "chr2": 2})] for sam, _ in contig]       # the contig factory's hits: plain 25M
    rows_seen, ops_seen = set(), set()
    for begin_id, end_id in sc.MERGE_WINDOWS:
        shits = [fc.restated(sam, begin_id, end_id) for sam, _ in spliced]
        want = layout(chits, shits, begin_id, end_id)
        rc, got = ing.span_batch_spliced([whole(b) for _, b in contig], [whole(b) for _, b in spliced], reads.piece() if with_reads else None,
                                         begin_id, end_id, T2R_MERGE)
        assert rc == 0, ing.error()
        same_batch(got, want, "window [%d, %d)" % (begin_id, end_id))
        rows_seen |= set(want[0].tolist())
        if got is not None:
            ops_seen |= set((got["hits"]["cigar"][:, 1] >> 28).tolist())
            if with_reads:
                assert got["read_len"].tolist() == [30 + i % 40 for i in want[0].tolist()]
    # the table's own claims (splice_cases): spliced-only rows, no row without a first-segment hit, the id range's ends from the spliced map
    assert {18, 22, 32, 40} <= rows_seen and not rows_seen & {24, 26, 28, 29, 36}
    assert {7, 8, 9, 10, 11} <= ops_seen, "junction hits and fused hits of all four directions went through the merge"
