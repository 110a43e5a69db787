"""GPU: the junction consensus through the C ABI -- thj_juncbed_* -- against the recorded
junctions.bed of the reference's nine regression cases, against the oracle on seeded long_spanning_reads results left
resident on the device, and on hand-made filter cases."""
import os

import numpy as np
import pytest

import fusionsout_ref as fr
import indelbed_cases as ic
import indelbed_ref as ir
import orc
import ref_regression as rr
from test_hostsim_spanning import SPAN_CASES, span_inputs
from tophat_amd import host

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", rr.CASES)
def test_recorded_alignments_give_the_recorded_junctions_bed(case):
    recs = rr.recorded_alignment_records(case)
    genome = "".join(l.strip() for l in open(os.path.join(rr.GOLD, case, "genome.fa")) if not l.startswith(">")).upper()
    with host.Context(0) as ctx:
        ctx.upload_genome(host.pack_genome([orc.fold_genome_char(genome)]))
        ctx.juncbed_reset()
        a = host.aln_array_from_tuples(recs)
        half = len(a) // 2
        ctx.juncbed_add_records(a[:half])              # in two pieces: the reduce does not care how records arrive
        ctx.juncbed_add_records(a[half:])
        js = ctx.juncbed_finish(8)
    assert host.junctions_bed_text(js, ["fake"]) == open(os.path.join(rr.GOLD, case, "junctions.bed")).read()


@pytest.mark.parametrize("cfg", SPAN_CASES, ids=lambda c: "seed%d_rl%d_L%d" % (c["seed"], c["read_len"], c["seg_len"]))
def test_resident_spanning_records_reduce_like_the_oracle(cfg):
    case, p, seqs, g, sb, juncs, ins = span_inputs(cfg, cfg.get("n_reads", 400))
    want_alns = orc.spanning(p, g, sb, juncs, ins)
    want = orc.junction_consensus(orc.jrecs_from_alns(want_alns))
    with host.Context(0) as ctx:
        ctx.upload_genome(host.pack_genome(seqs))
        ctx.upload_span_sets(juncs, ins)
        got_alns = ctx.spanning(p, [ctx.upload_span_batch(sb)])
        assert got_alns == want_alns
        ctx.juncbed_reset()
        ctx.juncbed_add_span()                          # straight from the slots the stitch kernels wrote
        js = ctx.juncbed_finish(8)
        js2 = ctx.juncbed_finish(8)                     # finishing twice changes nothing
    assert js.tolist() == js2.tolist()
    assert [tuple(int(x) for x in r) for r in js.tolist()] == [tuple(int(x) for x in r) for r in want.tolist()]
    assert len(want) > 3
    assert host.junctions_bed_text(js, case.names) == orc.junctions_bed(want, case.names)


def test_filters_on_the_device():
    from test_juncbed_cpu import test_filters as _unused      # noqa: F401  (the same cases, see there for what each one shows)
    M, N = 1, 11

    def rec(left, a, gap, b, anti=False, ref=1):
        return (ref, left, anti, [(M, a), (N, gap), (M, b)])
    cases = [
        [rec(100, 20, 500, 7)],
        [rec(100, 20, 500, 7), rec(90, 30, 500, 12)],
        [rec(100, 20, 60000, 20)], [rec(100, 20, 60000, 20)] * 2, [rec(100, 20, 60000, 12)] * 2,
        [rec(100, 20, 500, 20, anti=False)] * 3 + [rec(103, 20, 497, 20, anti=True)],
        [rec(100, 20, 500, 20, anti=False)] * 2 + [rec(103, 20, 497, 20, anti=True)] * 2,       # equal support: both stay
        [(1, 100, False, [(M, 20), (N, 300), (M, 30), (N, 400), (M, 25)])],
        [(1, 100, False, [(M, 20), (N, 300), (M, 30), (N, 400), (M, 5)])],
        [(2, 1000, True, [(M, 10), (5, 3), (M, 10), (N, 100), (M, 15), (3, 2), (M, 9)])],
        [rec(3, 9, 100, 30), rec(5, 9, 98, 30, anti=True), rec(5, 9, 98, 30, anti=True)],       # left < anchor: no shadow test at all
        [],
    ]
    rng = np.random.default_rng(3)
    many = []
    for _ in range(3000):                                # a crowd of near-coincident junctions on both strands
        l0 = int(rng.integers(50, 400))
        many.append(rec(l0, int(rng.integers(5, 40)), int(rng.integers(60, 90)), int(rng.integers(5, 40)), anti=bool(rng.integers(0, 2)), ref=int(rng.integers(1, 3))))
    cases.append(many)
    with host.Context(0) as ctx:
        ctx.upload_genome(host.pack_genome(["ACGT" * 5000, "TTGCA" * 4000]))
        for recs in cases:
            ctx.juncbed_reset()
            ctx.juncbed_add_records(host.aln_array_from_tuples(recs))
            got = ctx.juncbed_finish(8)
            want = orc.junction_consensus(orc.jrecs_from_tuples(recs))
            assert [tuple(int(x) for x in r) for r in got.tolist()] == [tuple(int(x) for x in r) for r in want.tolist()], recs[:3]
    assert len(want) > 50


def test_table_overflow_is_loud_and_recoverable():
    M, N = 1, 11
    recs = [(1, 100 + 3 * k, False, [(M, 20), (N, 200), (M, 20)]) for k in range(3000)]
    a = host.aln_array_from_tuples(recs)
    with host.Context(0) as ctx:
        ctx.upload_genome(host.pack_genome(["ACGT" * 5000]))
        ctx.juncbed_configure(1)                         # rounds up to the minimum table
        ctx.juncbed_reset()
        ctx.juncbed_add_records(np.concatenate([a] * 30) if False else a)
        js = ctx.juncbed_finish(8)
        assert len(js) == 3000


def _fusion_cases():
    """fusion alignments that also hold splices: pieces running up (M, N, D) and down (m, n, d) the genome on either side of the fusion
    op, every direction, junctions before and behind the fusion (the ones behind belong to the second contig -- except after an RR
    fusion, which junctions_from_spliced_hit has no case for, junctions.cpp:77-85); plain spliced records among them"""
    M, m, I, D, d, N, n = 1, 2, 3, 5, 6, 11, 12
    FF, FR, RF, RR = 7, 8, 9, 10
    return [
        (1, 1000, False, [(M, 30), (N, 200), (M, 20), (FF, 5000), (M, 50)], 2),
        (1, 1000, False, [(M, 30), (N, 200), (M, 20), (FF, 5000), (M, 25), (N, 300), (M, 25)], 2),
        (1, 1000, True, [(M, 30), (N, 200), (M, 20), (FR, 9000), (m, 25), (n, 300), (m, 25)], 2),
        (2, 4000, False, [(m, 20), (n, 150), (m, 30), (RF, 700), (M, 30), (N, 90), (M, 20)], 1),
        (2, 4000, False, [(m, 20), (n, 150), (m, 30), (RR, 700), (m, 30), (n, 90), (m, 20)], 1),
        (1, 2000, False, [(M, 12), (D, 2), (M, 10), (N, 500), (M, 28), (FF, 3000), (M, 20), (I, 1), (M, 29)], 2),
        (1, 1000, False, [(M, 30), (N, 200), (M, 70)]), (1, 1000, False, [(M, 30), (N, 200), (M, 70)]),
        (2, 5025, False, [(M, 25), (N, 300), (M, 25)]),
        (2, 8675, True, [(M, 25), (N, 300), (M, 25)]),
    ]


def test_fusion_alignments_on_the_device():
    recs = _fusion_cases() * 3
    with host.Context(0) as ctx:
        ctx.upload_genome(host.pack_genome(["ACGT" * 5000, "TTGCA" * 4000]))
        ctx.juncbed_reset()
        ctx.juncbed_add_records(host.aln_array_from_tuples(recs))
        got = ctx.juncbed_finish(8)
    want = orc.junction_consensus(orc.jrecs_from_tuples(recs))
    assert [tuple(int(x) for x in r) for r in got.tolist()] == [tuple(int(x) for x in r) for r in want.tolist()]
    assert len(want) >= 8 and {int(r["ref_id"]) for r in want} == {1, 2}


def test_thj_junctions_reads_fusion_bams(tmp_path):
    """the executable on a BAM that holds fusion alignments in their two-record XF:Z form (bwt_map.cpp:2047-2083): the XF re-parse of
    BAMHitFactory (bwt_map.cpp:1208-1318) -> the same junctions.bed as the oracle's consensus of the alignments themselves"""
    import subprocess
    from locked_make import locked_make
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    locked_make(os.path.join(here, "hostio"))
    names, lens = ["chrA", "chrB"], [20000, 20000]
    seqs = ["ACGT" * 5000, "TTGCA" * 4000]
    open(tmp_path / "ref.fa", "w").write("".join(">%s\n%s\n" % (n_, s_) for n_, s_ in zip(names, seqs)))
    open(tmp_path / "hdr.sam", "w").write("@HD\tVN:1.0\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % (n_, l_) for n_, l_ in zip(names, lens)))
    letters = {1: "M", 2: "m", 3: "I", 4: "i", 5: "D", 6: "d", 11: "N", 12: "n"}
    recs = _fusion_cases() * 2
    lines = []
    for k, rec in enumerate(recs):
        ref, left, anti, cig = rec[:4]
        xs = "XS:A:%s" % ("-" if anti else "+")
        if len(rec) > 4:
            # F carries the position on the second contig + 1; the two records' own columns are the two pieces (their exact CIGARs do not matter here)
            cg = "".join("%d%s" % ((ln + 1, "F") if op in (7, 8, 9, 10) else (ln, letters[op])) for op, ln in cig)
            rl = sum(ln for op, ln in cig if op in (1, 2, 3, 4))
            xf = "%s-%s %d %s %s %s" % (names[ref - 1], names[rec[4] - 1], left + 1, cg, "A" * rl, "I" * rl)
            lines.append("%d\t0\t%s\t%d\t255\t%dM\t%s\t%s\tNM:i:0\t%s\tXF:Z:1 %s" % (k + 1, names[ref - 1], left + 1, 10, "A" * 10, "I" * 10, xs, xf))
            lines.append("%d\t0\t%s\t%d\t255\t%dM\t%s\t%s\tNM:i:0\t%s\tXF:Z:2 %s" % (k + 1, names[rec[4] - 1], 7, 10, "A" * 10, "I" * 10, xs, xf))
        else:
            cg = "".join("%d%s" % (ln, letters[op]) for op, ln in cig)
            rl = sum(ln for op, ln in cig if op in (1, 3))
            lines.append("%d\t0\t%s\t%d\t255\t%s\t%s\t%s\tNM:i:0\t%s" % (k + 1, names[ref - 1], left + 1, cg, "A" * rl, "I" * rl, xs))
    open(tmp_path / "recs.sam", "w").write("\n".join(lines) + "\n")
    subprocess.check_call([os.path.join(here, "hostio", "hostio_check"), "sam2bam", str(tmp_path / "hdr.sam"), str(tmp_path / "recs.sam"), str(tmp_path / "in.bam")])
    subprocess.check_call([os.path.join(root, "tophat_amd", "bin", "thj_junctions"), "--sam-header", str(tmp_path / "hdr.sam"), str(tmp_path / "ref.fa"),
                           str(tmp_path / "junctions.bed"), str(tmp_path / "in.bam")], stderr=subprocess.DEVNULL)
    want = orc.junctions_bed(orc.junction_consensus(orc.jrecs_from_tuples(recs)), names)
    assert open(tmp_path / "junctions.bed").read() == want
    assert want.count("\n") >= 8


def test_all_three_tables_overflow_and_recover():
    """more distinct junctions (50 000) than the minimum table lets in (2^16 slots, three quarters usable = 49 152) but fewer than it
    has slots, so no insert ever walks a full table; with the indel sets and the fusion set collected, so that the larger capacity
    afterwards moves all three tables"""
    M, N = 1, 11
    n = 50000
    recs = [(1, 100 + 3 * k, False, [(M, 20), (N, 200), (M, 20)], 0, k, 0) for k in range(n)]
    a = host.aln_array_from_tuples(recs)
    want = orc.junction_consensus(orc.jrecs_from_tuples(recs))
    assert len(want) == n
    with host.Context(0) as ctx:
        ctx.upload_genome(host.pack_genome(["ACGTG" * 40000]))
        ctx.juncbed_configure(1)                         # rounds up to the minimum table
        ctx.juncbed_reset()
        ctx.juncbed_collect_indels(True)
        ctx.juncbed_collect_fusions(True)
        ctx.juncbed_add_records(a)
        with pytest.raises(host.ThjError, match=r"\(-4\).*junction table full \(50000 distinct junctions, capacity 65536\): call thj_juncbed_configure with a larger capacity and add the records again"):
            ctx.juncbed_finish(8)
        ctx.juncbed_configure(1 << 18)
        ctx.juncbed_reset()
        ctx.juncbed_collect_indels(True)
        ctx.juncbed_collect_fusions(True)
        ctx.juncbed_add_records(a)
        js = ctx.juncbed_finish(8)
        ins, dels = ctx.juncbed_indels()
        st = ctx.juncbed_fusions()
    assert [tuple(int(x) for x in r) for r in js.tolist()] == [tuple(int(x) for x in r) for r in want.tolist()]
    assert len(ins) == 0 and len(dels) == 0 and len(st) == 0


def _growing_calls():
    """three add calls of 100, 6000 and 12 000 records drawn from the planted families of the consensus tests, every read's records
    inside one call and read_idx numbered per call -> [(records, SEQ strings)], the genome.
      fusion reads    one record: a junction in front of the fusion op, a deletion in whichever anchor runs up the genome (the shape of
                      fusionsout_cases.crowd's kind 0 and of indelbed_cases.fusion_indel_cases), 14 break points x 4 directions; some
                      fail the edit distance or an anchor, some junction anchors are too short for the filter
      unsplit reads   one contiguous record of 60 bases or more with three indels (indelbed_cases.crowd's places), half of them over
                      the chrA ends of the break points
      spliced reads   three records a read (more than fusion_multireads): a deletion or an insertion, then a junction, either strand"""
    import fusionsout_cases as fc
    M, m, I, D, N, n = fc.M, fc.m, fc.I, fc.D, fc.N, fc.n
    rng = np.random.default_rng(29)
    genome = ["".join("ACGT"[k] for k in rng.integers(0, 4, 20000)) for _ in range(2)]
    anchors = (20, 21, 30, 49, 50, 51, 60)

    def fusion_read(read, x):
        k = x[0] % 14
        dr = (fc.FF, fc.FR, fc.RF, fc.RR)[x[1] % 4]
        l, r = 1000 + 40 * k, 500 + 28 * k
        a, b = anchors[x[2] % 7], (15 if x[3] % 22 == 0 else anchors[x[3] % 7])
        j = (5, 9, 25, 25, 25, 25, 25, 25)[x[4] % 8]
        up1, up2 = dr in (fc.FF, fc.FR), dr in (fc.FF, fc.RF)
        if up1:
            cig, left = [(M, j), (N, 80), (M, 10), (D, 2), (M, a - 10)], l + 1 - (a + 2 + j + 80)
        else:
            cig, left = [(m, j), (n, 80), (m, a)], l - 1 + (a + j + 80)
        cig += [(dr, r)] + ([(M, 10), (D, 1 + k % 3), (M, b - 10)] if up2 else [(m, b)])
        return [(1, left, x[5] % 2 == 1, cig, 2, read, ((0,) * 13 + (1, 2, 4))[x[6] % 16])]

    def unsplit_read(read, x):
        k = x[0] % 14
        ref, left = (1, 1000 + 40 * k - 30) if x[1] % 2 else (2, 3000 + 37 * (x[0] % 80))
        cig = [(M, 20), (I, 1 + k % 3), (M, 15), (D, 1 + k % 2), (M, 15), (I, 1 + (k // 3) % 3), (M, (10, 20, 40)[x[2] % 3])]
        return [(ref, left, False, cig, 0, read, (0, 0, 0, 0, 0, 0, 0, 1, 2, 3)[x[3] % 10])]

    def spliced_read(read, x):
        out = []
        for q in range(3):
            k = x[q] % 30
            left = 8000 + 150 * k + x[3 + q] % 2
            cig = [(M, 10 + x[q] % 3 * 7), ((I, D)[x[6] >> q & 1], 1 + k % 3), (M, 25 - left % 2), (N, 70 + k % 3), (M, (5, 20, 35)[x[7] >> q & 1])]
            out.append((2, left, (x[7] >> (4 + q)) & 1 == 1, cig, 0, read, 0))
        return out

    calls = []
    for n_fus, n_uns, n_spl in [(40, 30, 10), (4800, 900, 100), (6100, 4700, 400)]:
        kinds = rng.permutation([0] * n_fus + [1] * n_uns + [2] * n_spl)
        draws = rng.integers(0, 1 << 30, (len(kinds), 8)).tolist()
        recs = [r for read, kind in enumerate(kinds.tolist()) for r in (fusion_read, unsplit_read, spliced_read)[kind](read, draws[read])]
        calls.append((recs, ic.make_seqs(recs, len(recs))))
    return calls, genome


def _list_entries(recs, multi=2):
    """how many entries one add call appends to the junction, indel, F, U and J occurrence lists and to the group sizes (the rules
    at the head of thj_juncbed_impl.h, thj_juncbed_indel_impl.h and thj_juncbed_fusion_impl.h, from the restatements' walkers)"""
    group = {}
    for r in recs:
        group[r[5]] = group.get(r[5], 0) + 1
    n = dict(junction=0, indel=0, F=0, U=0, J=0, groups=len(recs))
    for r in recs:
        nj = len(ir.rec_juncs(r[:5]))
        f = fr._passes(r, 20, 2) is not None
        n["junction"] += nj
        n["indel"] += sum(1 for op, _ in r[3] if op in (3, 4, 5, 6))
        n["F"] += f
        n["U"] += fr.rec_fusion(r) is None and nj == 0 and r[6] <= 2 and fr.rec_unsplit(r)[2]
        n["J"] += nj if f or group[r[5]] > multi else 0
    return n


def test_lists_that_grow_across_add_calls_keep_what_they_held():
    """three add calls against one call on a fresh context, indels and fusions collected.  A list's first allocation is what the call
    needs plus a quarter plus 4096 entries, so a later call makes it grow -- with entries in it that have to be carried over -- when it
    brings more than that slack.  The second call does that for the junction, indel, F and J lists and for the group sizes, the third
    for all of these again and for the U list (F and U entries are one a record at most, so 6000 records cannot outgrow both)."""
    calls, genome = _growing_calls()
    assert [len(recs) for recs, _ in calls] == [100, 6000, 12000]
    held, cap, grew = {}, {}, {}
    for k, (recs, _) in enumerate(calls):
        for name, n in _list_entries(recs).items():
            need = held.get(name, 0) + n
            if need > cap.get(name, 0):
                grew.setdefault(name, []).append(k)
                cap[name] = need + need // 4 + 4096
            held[name] = need
            assert k > 0 or n > 0, name                        # after the first call every list holds entries
    assert all(grew[name] == [0, 1, 2] for name in ("junction", "indel", "F", "J", "groups")) and grew["U"] == [0, 2], grew
    # what the whole list must give, from the restatements alone (read_idx: the calls' reads numbered on)
    recs, seqs, base = [], [], 0
    for part, sq in calls:
        recs += [r[:5] + (r[5] + base, r[6]) for r in part]
        seqs += sq
        base += 1 + max(r[5] for r in part)
    want_j, want_i, want_d = ir.consensus([r[:5] for r in recs], seqs)
    want_f = fr.fusions(recs, genome)
    assert len(want_j) > 50 and len(want_i) > 50 and len(want_d) > 50 and len(want_f) > 50
    assert any(row[2] > 0 for row in want_f)                   # some unsupport: the U list matters

    def run(ctx, pieces):
        ctx.upload_genome(host.pack_genome(genome))
        ctx.juncbed_reset()
        ctx.juncbed_collect_indels(True)
        ctx.juncbed_collect_fusions(True)
        for part, sq in pieces:
            ctx.juncbed_add_records_seq(host.aln_array_from_tuples(part), [ir.ins_letters(r[:5], s) for r, s in zip(part, sq)])
        js = ctx.juncbed_finish(8)
        return (js,) + ctx.juncbed_indels() + (ctx.juncbed_fusions(),)
    with host.Context(0) as ctx:
        grown = run(ctx, calls)
    with host.Context(0) as ctx:
        fresh = run(ctx, [(recs, seqs)])
    assert all(g.tobytes() == f.tobytes() for g, f in zip(grown, fresh))
    js, ins, dels, st = grown
    assert [tuple(int(x) for x in r) for r in js.tolist()] == [tuple(int(x) for x in r) for r in orc.junction_consensus(orc.jrecs_from_tuples(recs)).tolist()]
    assert (ir.junc_rows(js), ir.ins_rows(ins), ir.del_rows(dels)) == (want_j, want_i, want_d)
    assert fr.stat_rows(st) == want_f
