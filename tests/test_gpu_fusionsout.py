"""GPU: fusions.out from the junction consensus pass (thj_juncbed_collect_fusions, _fusion_count, _fusion_download; thj_junctions
--fusions-out) against the Python restatement of the reference (tests/fusionsout_ref.py, itself pinned by hand-written lines in
tests/test_fusionsout_cpu.py)."""
import copy
import os
import subprocess

import numpy as np
import pytest

import fusionsout_cases as fc
import fusionsout_ref as fr
import indelbed_ref as ir
import orc
from tophat_amd import host

pytestmark = pytest.mark.gpu
M, N, FF = fc.M, fc.N, fc.FF


def _run(ctx, recs, pieces=1, anchor=20, mism=2, multi=2, collect=True):
    """reset, collect, add (in `pieces` calls, cut between reads, every call's read_idx numbered from 0), finish -> (junctions, fusion stats)"""
    ctx.juncbed_reset()
    if collect:
        ctx.juncbed_collect_fusions(True, anchor, mism, multi)
    cuts = [0]
    for k in range(1, pieces):
        at = len(recs) * k // pieces
        while 0 < at < len(recs) and recs[at][5] == recs[at - 1][5]:
            at += 1
        cuts.append(max(at, cuts[-1]))
    cuts.append(len(recs))
    for k in range(len(cuts) - 1):
        part = fc.renumber(recs[cuts[k]:cuts[k + 1]])
        if part:
            ctx.juncbed_add_records(host.aln_array_from_tuples(part))
    js = ctx.juncbed_finish(8)
    return js, ctx.juncbed_fusions()


def _check(ctx, recs, pieces=1, **kw):
    want = fr.fusions(recs, fc.GENOME, **kw)
    js, st = _run(ctx, recs, pieces, **kw)
    assert fr.stat_rows(st) == want
    assert host.fusions_out_text(st, fc.NAMES) == fr.fusions_out(want, fc.NAMES)
    assert ir.junc_rows(js) == ir.consensus([r[:5] for r in recs])[0]                   # the junction rows are what they were
    return want


@pytest.fixture(scope="module")
def ctx():
    with host.Context(0) as c:
        c.upload_genome(host.pack_genome(fc.GENOME))
        yield c


@pytest.mark.parametrize("pieces", [1, 2, 3])
def test_case_lists(ctx, pieces):
    want = _check(ctx, fc.renumber(fc.directions()), pieces)
    assert {r[0][4] for r in want} == {7, 8, 9, 10} and any(r[2] > 0 for r in want) and any(not r[7] for r in want)
    _check(ctx, fc.renumber(fc.walker_cases()), pieces, anchor=0)
    want = _check(ctx, fc.crowd(), pieces)
    assert len(want) >= 5 and sum(r[2] for r in want) > 20
    _check(ctx, fc.crowd(seed=10), pieces, anchor=25, multi=1, mism=3)


@pytest.mark.parametrize("n", [63, 64, 65, 129])
def test_wave_wide_reservations(ctx, n):
    kinds = [[(1, 1000, False, [(M, 60), (FF, 500), (M, 40)], 2)], [(1, 1020, False, [(M, 100)], 0)], [(2, 450, False, [(M, 100)], 0)],
             [(1, 900, False, [(M, 25), (N, 80), (M, 55), (FF, 500), (M, 40)], 2)] * 3, [(1, 380, False, [(M, 30), (N, 100), (M, 30)], 0)]]
    recs, read = [], 0
    while len(recs) < n:
        for r in kinds[(read * 7 + read // 5) % 5]:
            recs.append(r + (read, read % 3))
        read += 1
    want = _check(ctx, recs[:n])
    assert len(want) >= 1 and want[0][2] > 0


def test_finishing_twice_changes_nothing_and_collection_off(ctx):
    recs = fc.crowd()
    js, st = _run(ctx, recs)
    js2, st2 = ctx.juncbed_finish(8), ctx.juncbed_fusions()
    assert js.tolist() == js2.tolist() and st.tobytes() == st2.tobytes() and len(st) >= 5
    js3, st3 = _run(ctx, recs, collect=False)                                            # off: zero rows, today's outputs
    ins, dels = ctx.juncbed_indels()
    assert len(st3) == 0 and js3.tolist() == js.tolist() and len(ins) == 0 and len(dels) == 0
    assert ir.junc_rows(js3) == ir.junc_rows(orc.junction_consensus(orc.jrecs_from_tuples([r[:5] for r in recs])))


def test_read_idx_outside_the_call(ctx):
    recs = fc.renumber(fc.directions())
    a = host.aln_array_from_tuples(recs)
    a["read_idx"][3] = len(a)
    ctx.juncbed_reset()
    ctx.juncbed_collect_fusions(True)
    with pytest.raises(host.ThjError, match=r"\(-1\).*read_idx"):
        ctx.juncbed_add_records(a)
    ctx.juncbed_finish(8)
    assert len(ctx.juncbed_fusions()) == 0                                               # nothing was counted


def test_fusion_table_overflow_is_loud_and_recoverable():
    # more distinct fusions than the minimum table (2^16 slots, three quarters usable) holds
    n = 50000
    a = np.zeros(n, dtype=host.ALN_DTYPE)
    k = np.arange(n)
    a["read_idx"], a["ref_id"], a["left"], a["n_cigar"] = k, 1, 100 + (k % 250) * 4, 3
    a["cigar"][:, 0], a["cigar"][:, 1], a["cigar"][:, 2], a["cigar"][:, 15] = (M << 28) | 30, (FF << 28) | (100 + (k // 250) * 8), (M << 28) | 30, 2
    with host.Context(0) as c:
        c.upload_genome(host.pack_genome(fc.GENOME))
        c.juncbed_configure(1)                                 # rounds up to the minimum table
        c.juncbed_reset()
        c.juncbed_collect_fusions(True)
        c.juncbed_add_records(a)
        with pytest.raises(host.ThjError, match=r"\(-4\).*fusion table full"):
            c.juncbed_finish(8)
        c.juncbed_configure(1 << 17)
        c.juncbed_reset()
        c.juncbed_collect_fusions(True)
        c.juncbed_add_records(a)
        c.juncbed_finish(8)
        st = c.juncbed_fusions()
    assert len(st) == n and int(st["count"].sum()) == n and int(st["left_ext"].min()) == 30
    got = np.stack([st["left"].astype(np.int64), st["right"].astype(np.int64)], axis=1)
    want = np.unique(np.stack([a["left"].astype(np.int64) + 29, 100 + (k // 250) * 8], axis=1), axis=0)
    assert (got == want).all()


# ---------------------------------------------------------------------------------------------- resident path
from golden_util import FUSION_SPAN_CASES, load  # noqa: E402


def test_resident_fusion_spanning_records_give_the_restatements_rows():
    """juncbed_add_span after a --fusion-search spanning pass: the rows the restatement computes from the oracle's alignments"""
    from test_golden_cpu import fusion_span_inputs
    n_rows = 0
    for name in FUSION_SPAN_CASES:
        c = load(name)
        juncs, ins, fus = fusion_span_inputs(c)
        p = copy.copy(c["p"])
        p.fusion_search = 1
        with host.Context(0) as ctx:
            ctx.upload_genome(host.pack_genome(c["seqs"]))
            ctx.upload_span_sets(juncs, ins)
            ctx.upload_span_fusions(fus)
            for sd, sb in c["span_batches"].items():
                want_alns = orc.spanning_fusion(p, orc.Genome(c["seqs"]), sb, juncs, ins, fus, True)
                recs = [(a.ref_id, a.left, a.antisense_splice, [(x >> 28, x & 0x0FFFFFFF) for x in a.cigar], a.ref_id2, a.read_idx, a.edit_dist) for a in want_alns]
                want = fr.fusions(recs, c["seqs"])
                assert ctx.spanning(p, [ctx.upload_span_batch(sb)]) == want_alns
                ctx.juncbed_reset()
                ctx.juncbed_collect_fusions(True)
                ctx.juncbed_add_span()                         # straight from the slots the stitch kernels wrote
                js = ctx.juncbed_finish(8)
                st = ctx.juncbed_fusions()
                assert fr.stat_rows(st) == want
                assert ir.junc_rows(js) == ir.consensus([r[:5] for r in recs])[0]
                n_rows += len(want)
    assert n_rows >= 1


# ---------------------------------------------------------------------------------------------- the executable
def test_thj_junctions_writes_fusions_out(tmp_path):
    from locked_make import locked_make
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    locked_make(os.path.join(here, "hostio"))
    names, seqs = fc.NAMES, fc.GENOME
    open(tmp_path / "ref.fa", "w").write("".join(">%s\n%s\n" % (n_, s_) for n_, s_ in zip(names, seqs)))
    open(tmp_path / "hdr.sam", "w").write("@HD\tVN:1.0\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % (n_, len(s_)) for n_, s_ in zip(names, seqs)))
    letters = {1: "M", 2: "m", 11: "N", 12: "n"}
    # QNAME runs of 1, 2 and 3 records (the crowd has up to four alignments a read), NM:i from 0 to 4, XF:Z pairs for the fusion records
    recs = [r for r in fc.crowd(seed=12, n_reads=150)]
    assert {sum(1 for r in recs if r[5] == k) for k in range(150)} >= {1, 2, 3}
    lines = []                                                # hostio_check's trimmed SAM form: QNAME FLAG RNAME POS MAPQ CIGAR SEQ QUAL tags
    for rec in recs:
        ref, left, anti, cig, ref2, read, ed = rec
        xs = "XS:A:%s" % ("-" if anti else "+")
        n_seq = sum(ln for op, ln in cig if op in (1, 2))
        sq = "ACGT" * (n_seq // 4) + "ACGT"[:n_seq % 4]
        if ref2:                                              # the two-record XF:Z form (bwt_map.cpp:2047-2083)
            cg = "".join("%d%s" % ((ln + 1, "F") if op in (7, 8, 9, 10) else (ln, letters[op])) for op, ln in cig)
            xf = "%s-%s %d %s %s %s" % (names[ref - 1], names[ref2 - 1], left + 1, cg, sq, "I" * len(sq))
            lines.append("%d\t0\t%s\t%d\t255\t10M\t%s\t%s\tNM:i:%d\t%s\tXF:Z:1 %s" % (read, names[ref - 1], left + 1, "A" * 10, "I" * 10, ed, xs, xf))
            lines.append("%d\t0\t%s\t%d\t255\t10M\t%s\t%s\tNM:i:%d\t%s\tXF:Z:2 %s" % (read, names[ref2 - 1], 7, "A" * 10, "I" * 10, ed, xs, xf))
        else:
            cg = "".join("%d%s" % (ln, letters[op]) for op, ln in cig)
            lines.append("%d\t0\t%s\t%d\t255\t%s\t%s\t%s\tNM:i:%d\t%s" % (read, names[ref - 1], left + 1, cg, sq, "I" * len(sq), ed, xs))
    open(tmp_path / "recs.sam", "w").write("\n".join(lines) + "\n")
    subprocess.check_call([os.path.join(here, "hostio", "hostio_check"), "sam2bam", str(tmp_path / "hdr.sam"), str(tmp_path / "recs.sam"), str(tmp_path / "in.bam")])
    exe = os.path.join(root, "tophat_amd", "bin", "thj_junctions")

    def run(d, *opts):
        (tmp_path / d).mkdir()
        subprocess.check_call([exe, "--sam-header", str(tmp_path / "hdr.sam")] + list(opts) + [str(tmp_path / "ref.fa"), str(tmp_path / d / "junctions.bed"), str(tmp_path / "in.bam")],
                              stderr=subprocess.DEVNULL)
        return tmp_path / d
    d1 = run("with", "--fusions-out", str(tmp_path / "with" / "fusions.out"))
    want = fr.fusions_out(fr.fusions(recs, seqs), names)
    assert open(d1 / "fusions.out").read() == want and want.count("\n") >= 4
    d2 = run("other", "--fusions-out", str(tmp_path / "other" / "fusions.out"), "--fusion-anchor-length", "25", "--fusion-multireads", "1")
    want2 = fr.fusions_out(fr.fusions(recs, seqs, anchor=25, multi=1), names)
    assert open(d2 / "fusions.out").read() == want2 and want2 != want and want2.count("\n") >= 2
    d3 = run("without")
    assert open(d3 / "junctions.bed").read() == open(d1 / "junctions.bed").read() == ir.junctions_bed(ir.consensus([r[:5] for r in recs])[0], names)
    assert sorted(os.listdir(d3)) == ["junctions.bed"]
