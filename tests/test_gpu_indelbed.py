"""GPU: insertions.bed and deletions.bed from the junction consensus pass (thj_juncbed_collect_indels, _add_records_seq,
_add_span_seq_async, _indel_counts, _indel_download; thj_junctions --insertions-out / --deletions-out) against the recorded
outputs of the reference's nine regression cases and against the Python restatement of the reference (tests/indelbed_ref.py,
itself pinned in tests/test_indelbed_cpu.py)."""
import functools
import os
import subprocess

import numpy as np
import pytest

import indelbed_cases as ic
import indelbed_ref as ir
import orc
import ref_regression as rr
from test_hostsim_spanning import SPAN_CASES, span_inputs
from tophat_amd import host

pytestmark = pytest.mark.gpu
M, I, D, N = ic.M, ic.I, ic.D, ic.N
_RC = str.maketrans("ACGTN", "TGCAN")


def _run(ctx, recs, seqs, pieces=1, anchor=8, configure=None):
    """reset, collect, add (in `pieces` calls), finish -> (junction rows, insertion rows, deletion rows, the three arrays)"""
    if configure:
        ctx.juncbed_configure(configure)
    ctx.juncbed_reset()
    ctx.juncbed_collect_indels(True)
    a = host.aln_array_from_tuples(recs)
    letters = [ir.ins_letters(r, s) for r, s in zip(recs, seqs)]
    cut = [len(a) * k // pieces for k in range(pieces + 1)]
    for k in range(pieces):
        ctx.juncbed_add_records_seq(a[cut[k]:cut[k + 1]], letters[cut[k]:cut[k + 1]])
    js = ctx.juncbed_finish(anchor)
    ins, dels = ctx.juncbed_indels()
    return ir.junc_rows(js), ir.ins_rows(ins), ir.del_rows(dels), (js, ins, dels)


def _check(ctx, recs, seqs, pieces=1):
    want = ir.consensus(recs, seqs)
    got = _run(ctx, recs, seqs, pieces)
    assert got[0] == want[0]
    assert got[1] == want[1]
    assert got[2] == want[2]
    return want, got[3]


@pytest.fixture()
def ctx():
    with host.Context(0) as c:
        c.upload_genome(host.pack_genome(ic.GENOME))
        yield c


# ---------------------------------------------------------------------------------------------- recorded cases
@pytest.mark.parametrize("case", rr.CASES)
def test_recorded_alignments_give_the_three_recorded_bed_files(case):
    recs = rr.recorded_alignment_records(case)
    seqs = ir.recorded_seqs(rr.GOLD, case)
    genome = "".join(l.strip() for l in open(os.path.join(rr.GOLD, case, "genome.fa")) if not l.startswith(">")).upper()
    with host.Context(0) as c:
        c.upload_genome(host.pack_genome([orc.fold_genome_char(genome)]))
        _, _, _, (js, ins, dels) = _run(c, recs, seqs, pieces=2)
    gold = lambda f: open(os.path.join(rr.GOLD, case, f)).read()
    assert host.insertions_bed_text(ins, ["fake"]) == gold("insertions.bed")
    assert host.deletions_bed_text(dels, ["fake"]) == gold("deletions.bed")
    assert host.junctions_bed_text(js, ["fake"]) == gold("junctions.bed")


# ---------------------------------------------------------------------------------------------- resident path
@functools.lru_cache(maxsize=None)
def _span_expected(k):
    cfg = SPAN_CASES[k]
    case, p, seqs, g, sb, juncs, ins = span_inputs(cfg, cfg.get("n_reads", 400))
    alns = orc.spanning(p, g, sb, juncs, ins)
    recs = [(a.ref_id, a.left, a.antisense_splice, [(c >> 28, c & 0x0FFFFFFF) for c in a.cigar], a.ref_id2) for a in alns]
    sq = []
    for a in alns:                                          # SEQ of the record: the read, reverse-complemented for FLAG 0x10
        s = bytes(sb.bases[sb.read_off[a.read_idx]:sb.read_off[a.read_idx + 1]]).decode()
        sq.append(s.translate(_RC)[::-1] if a.antisense else s)
    return (case, p, seqs, sb, juncs, ins, alns), ir.consensus(recs, sq)


def test_span_seeds_hold_both_kinds_of_indel():
    assert any(len(_span_expected(k)[1][1]) >= 1 and len(_span_expected(k)[1][2]) >= 1 for k in range(len(SPAN_CASES)))


@pytest.mark.parametrize("k", range(len(SPAN_CASES)), ids=lambda k: "seed%d_rl%d_L%d" % (SPAN_CASES[k]["seed"], SPAN_CASES[k]["read_len"], SPAN_CASES[k]["seg_len"]))
def test_resident_spanning_records_give_the_restatements_sets(k):
    (case, p, seqs, sb, juncs, ins, want_alns), want = _span_expected(k)
    with host.Context(0) as c:
        c.upload_genome(host.pack_genome(seqs))
        c.upload_span_sets(juncs, ins)
        batch = c.upload_span_batch(sb)
        assert c.spanning(p, [batch]) == want_alns
        c.juncbed_reset()
        c.juncbed_collect_indels(True)
        c.juncbed_add_span_seq(batch)                      # the letters come from the batch's read planes, on the device
        js = c.juncbed_finish(8)
        i1, d1 = c.juncbed_indels()
        js2 = c.juncbed_finish(8)                           # finishing twice changes nothing
        i2, d2 = c.juncbed_indels()
    assert (js.tolist(), i1.tolist(), d1.tolist()) == (js2.tolist(), i2.tolist(), d2.tolist())
    assert (ir.junc_rows(js), ir.ins_rows(i1), ir.del_rows(d1)) == want


# ---------------------------------------------------------------------------------------------- hand-made
def test_first_record_keeps_its_letters(ctx):
    a = (1, 100, False, [(M, 20), (I, 2), (M, 20)])
    s1, s2 = "A" * 20 + "CG" + "A" * 20, "A" * 20 + "TT" + "A" * 20
    want, _ = _check(ctx, [a, a], [s1, s2])
    assert [(x[2], x[5]) for x in want[1]] == [("CG", 2)]
    want, _ = _check(ctx, [a, a], [s2, s1])
    assert [(x[2], x[5]) for x in want[1]] == [("TT", 2)]
    # the same through two add calls: the order of the calls is the order of the records
    want, _ = _check(ctx, [a, a], [s2, s1], pieces=2)
    assert want[1][0][2] == "TT"


def test_lengths_two_and_three_at_one_place(ctx):
    a = (1, 100, False, [(M, 20), (I, 3), (M, 20)])
    b = (1, 100, False, [(M, 20), (I, 2), (M, 20)])
    want, (_, ins, _) = _check(ctx, [a, b], ["A" * 20 + "GGG" + "A" * 20, "A" * 20 + "TT" + "A" * 20])
    assert [x[2] for x in want[1]] == ["TT", "GGG"]
    assert host.insertions_bed_text(ins, ic.NAMES) == ir.insertions_bed(want[1], ic.NAMES)


def test_the_cap_at_1000_is_the_insertion_printers(ctx):
    a = (1, 100, False, [(M, 20), (I, 2), (M, 20)])
    b = (1, 300, False, [(M, 20), (D, 2), (M, 20)])
    want, (_, ins, dels) = _check(ctx, [a] * 1001 + [b] * 1001, ["A" * 20 + "CG" + "A" * 20] * 1001 + ["A" * 40] * 1001)
    assert int(ins[0]["support"]) == 1001 and int(dels[0]["support"]) == 1001
    assert host.insertions_bed_text(ins, ic.NAMES) == ir.insertions_bed(want[1], ic.NAMES) and host.insertions_bed_text(ins, ic.NAMES).endswith("\tCG\t1000\n")
    assert host.deletions_bed_text(dels, ic.NAMES) == ir.deletions_bed(want[2], ic.NAMES) and host.deletions_bed_text(dels, ic.NAMES).endswith("\t-\t1001\n")


def test_a_deletion_on_a_filtered_record_does_not_count(ctx):
    dj = (1, 100, False, [(M, 20), (D, 2), (M, 20), (N, 200), (M, 5)])            # its junction fails min_anchor
    dc = (1, 100, False, [(M, 20), (D, 2), (M, 30)])
    want, _ = _check(ctx, [dj, dc], ["A" * 45, "A" * 50])
    assert [x[5] for x in want[2]] == [1]
    want, _ = _check(ctx, [dj], ["A" * 45])
    assert want[2] == []


def test_fusion_alignments_with_indels_on_both_sides(ctx):
    recs = ic.fusion_indel_cases() * 2
    seqs = ic.make_seqs(recs, 11)
    want, _ = _check(ctx, recs, seqs)
    assert {x[0] for x in want[1]} == {1, 2} and {x[0] for x in want[2]} == {1, 2} and len(want[1]) >= 8 and len(want[2]) >= 8
    # the clipped record's letters are SEQ[20:23]
    clipped = ic.fusion_indel_cases()[-2]
    assert any(x[2] == seqs[recs.index(clipped)][20:23] for x in want[1])


def test_an_insertion_holding_N(ctx):
    a = (2, 500, False, [(M, 20), (I, 3), (M, 20)])
    want, (_, ins, _) = _check(ctx, [a], ["A" * 20 + "NCN" + "A" * 20])
    assert want[1][0][2] == "NCN" and host.insertions_bed_text(ins, ic.NAMES) == "track name=insertions description=\"TopHat insertions\"\nchrB\t519\t519\tNCN\t1\n"


def test_sixteen_bases_are_held_and_seventeen_refused(ctx):
    a16 = (1, 100, False, [(M, 20), (I, 16), (M, 20)])
    a17 = (1, 100, False, [(M, 20), (I, 17), (M, 20)])
    s16 = "A" * 20 + "ACGTNACGTTGCAACG" + "A" * 20
    want, (_, ins, _) = _check(ctx, [a16], [s16])
    assert host.insertions_bed_text(ins, ic.NAMES).endswith("\tACGTNACGTTGCAACG\t1\n")
    ctx.juncbed_reset()
    ctx.juncbed_collect_indels(True)
    with pytest.raises(host.ThjError, match=r"\(-1\).*17 bases"):
        ctx.juncbed_add_records_seq(host.aln_array_from_tuples([a16, a17]), ["ACGTNACGTTGCAACG", "ACGTNACGTTGCAACGT"])
    ctx.juncbed_finish(8)
    ins, dels = ctx.juncbed_indels()
    assert len(ins) == 0 and len(dels) == 0                  # nothing was counted, the good record of the call included


def test_add_records_without_letters(ctx):
    a = (1, 100, False, [(M, 20), (I, 2), (M, 20), (N, 300), (M, 20)])
    b = (1, 100, False, [(M, 20), (D, 2), (M, 20), (N, 300), (M, 20)])
    arr = host.aln_array_from_tuples([a, b])
    ctx.juncbed_reset()
    ctx.juncbed_collect_indels(True)
    with pytest.raises(host.ThjError, match=r"\(-1\)"):
        ctx.juncbed_add_records(arr)
    ctx.juncbed_add_records(arr[1:])                        # deletions need no letters
    ctx.juncbed_finish(8)
    ins, dels = ctx.juncbed_indels()
    assert len(ins) == 0 and ir.del_rows(dels) == ir.consensus([b])[2]
    # collection off: today's junction result, no indels
    ctx.juncbed_reset()
    ctx.juncbed_add_records(arr)
    js = ctx.juncbed_finish(8)
    ins, dels = ctx.juncbed_indels()
    assert len(ins) == 0 and len(dels) == 0
    assert ir.junc_rows(js) == ir.junc_rows(orc.junction_consensus(orc.jrecs_from_tuples([a, b]))) and len(js) == 2      # the insertion does not move the junction, the deletion does


@pytest.mark.parametrize("n", [63, 64, 65, 129])
def test_wave_wide_reservations(ctx, n):
    kinds = [(1, 100, False, [(M, 20), (I, 2), (M, 20)]), (1, 400, False, [(M, 50)]), (2, 300, False, [(M, 20), (D, 3), (M, 20)]),
             (1, 100, False, [(M, 20), (N, 100), (M, 20)]), (2, 700, True, [(M, 10), (I, 1), (M, 10), (D, 2), (M, 10), (N, 90), (M, 12), (I, 3), (M, 9)])]
    recs = [kinds[(k * 7 + k // 5) % 5] for k in range(n)]
    want, _ = _check(ctx, recs, ic.make_seqs(recs, n, "ACGTN"))
    assert len(want[1]) >= 3 and len(want[2]) >= 2


def test_a_crowd(ctx):
    recs = ic.crowd()
    seqs = ic.make_seqs(recs, 17)
    want, _ = _check(ctx, recs, seqs, pieces=3)
    assert len(want[1]) > 20 and len(want[2]) > 20
    accepted = ir.first_pass(recs)
    assert sum(1 for r in recs if not ir.kept(r, accepted)) > 50                       # the filter does drop records
    last = {}
    for r, s in zip(recs, seqs):
        if ir.kept(r, accepted):
            for x in ir.rec_inss(r, s):
                last[(x[0], x[1], len(x[2]))] = x[2]
    assert any(last[(x[0], x[1], len(x[2]))] != x[2] for x in want[1])                 # "the last one wins" would not pass


# ---------------------------------------------------------------------------------------------- overflow
def test_indel_table_overflow_is_loud_and_recoverable(ctx):
    # more distinct deletions than the minimum table (2^16 slots, three quarters usable) holds; no junction at all
    n = 50000
    a = np.zeros(n, dtype=host.ALN_DTYPE)
    k = np.arange(n)
    a["ref_id"], a["left"], a["n_cigar"] = 1, 100 + (k % 5000) * 3, 3
    a["cigar"][:, 0], a["cigar"][:, 1], a["cigar"][:, 2] = (M << 28) | 20, (D << 28) | (1 + k // 5000), (M << 28) | 20
    ctx.juncbed_configure(1)                                 # rounds up to the minimum table
    ctx.juncbed_reset()
    ctx.juncbed_collect_indels(True)
    ctx.juncbed_add_records_seq(a, [""] * n)
    with pytest.raises(host.ThjError, match=r"\(-4\).*indel table full"):
        ctx.juncbed_finish(8)
    ctx.juncbed_configure(1 << 17)
    ctx.juncbed_reset()
    ctx.juncbed_collect_indels(True)
    ctx.juncbed_add_records_seq(a, [""] * n)
    ctx.juncbed_finish(8)
    ins, dels = ctx.juncbed_indels()
    assert len(ins) == 0 and len(dels) == n and int(dels["support"].sum()) == n
    d = np.stack([dels["left"].astype(np.int64), dels["right"].astype(np.int64)], axis=1)
    want = np.unique(np.stack([a["left"].astype(np.int64) + 19, a["left"].astype(np.int64) + 20 + 1 + k // 5000], axis=1), axis=0)
    assert (d == want).all()


# ---------------------------------------------------------------------------------------------- the executable
def test_thj_junctions_writes_the_three_files(tmp_path):
    from locked_make import locked_make
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    locked_make(os.path.join(here, "hostio"))
    names, seqs = ic.NAMES, ic.GENOME
    open(tmp_path / "ref.fa", "w").write("".join(">%s\n%s\n" % (n_, s_) for n_, s_ in zip(names, seqs)))
    open(tmp_path / "hdr.sam", "w").write("@HD\tVN:1.0\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % (n_, len(s_)) for n_, s_ in zip(names, seqs)))
    letters = {1: "M", 2: "m", 3: "I", 4: "i", 5: "D", 6: "d", 11: "N", 12: "n", 13: "S"}
    plain = [(1, 100, False, [(M, 20), (I, 2), (M, 20)]), (1, 100, False, [(M, 20), (I, 2), (M, 25)]), (2, 300, True, [(M, 20), (D, 3), (M, 20), (N, 100), (M, 4)]),
             (2, 300, False, [(M, 20), (D, 3), (M, 20)]), (1, 900, False, [(M, 50)]), (1, 100, False, [(M, 20), (I, 3), (M, 20)])]
    recs = ic.fusion_indel_cases() * 2 + plain * 2
    rseq = ic.make_seqs(recs, 23, "ACGTN")
    lines = []                                                # hostio_check's trimmed SAM form: QNAME FLAG RNAME POS MAPQ CIGAR SEQ QUAL tags
    for k, (rec, sq) in enumerate(zip(recs, rseq)):
        ref, left, anti, cig = rec[:4]
        xs = "XS:A:%s" % ("-" if anti else "+")
        if len(rec) > 4:                                      # the two-record XF:Z form (bwt_map.cpp:2047-2083); the columns of the two records do not matter here
            cg = "".join("%d%s" % ((ln + 1, "F") if op in (7, 8, 9, 10) else (ln, letters[op])) for op, ln in cig)
            xf = "%s-%s %d %s %s %s" % (names[ref - 1], names[rec[4] - 1], left + 1, cg, sq, "I" * len(sq))
            lines.append("%d\t0\t%s\t%d\t255\t10M\t%s\t%s\tNM:i:0\t%s\tXF:Z:1 %s" % (k + 1, names[ref - 1], left + 1, "A" * 10, "I" * 10, xs, xf))
            lines.append("%d\t0\t%s\t%d\t255\t10M\t%s\t%s\tNM:i:0\t%s\tXF:Z:2 %s" % (k + 1, names[rec[4] - 1], 7, "A" * 10, "I" * 10, xs, xf))
        else:
            cg = "".join("%d%s" % (ln, letters[op]) for op, ln in cig)
            lines.append("%d\t0\t%s\t%d\t255\t%s\t%s\t%s\tNM:i:0\t%s" % (k + 1, names[ref - 1], left + 1, cg, sq, "I" * len(sq), xs))
    assert len(lines) >= 40
    open(tmp_path / "recs.sam", "w").write("\n".join(lines) + "\n")
    subprocess.check_call([os.path.join(here, "hostio", "hostio_check"), "sam2bam", str(tmp_path / "hdr.sam"), str(tmp_path / "recs.sam"), str(tmp_path / "in.bam")])
    exe = os.path.join(root, "tophat_amd", "bin", "thj_junctions")
    out = tmp_path / "with"
    out.mkdir()
    subprocess.check_call([exe, "--sam-header", str(tmp_path / "hdr.sam"), "--insertions-out", str(out / "insertions.bed"), "--deletions-out", str(out / "deletions.bed"),
                           str(tmp_path / "ref.fa"), str(out / "junctions.bed"), str(tmp_path / "in.bam")], stderr=subprocess.DEVNULL)
    # the reader drops what cannot touch any of the three files (the 50M record); the restatement ignores it just the same
    wj, wi, wd = ir.consensus(recs, rseq)
    assert open(out / "insertions.bed").read() == ir.insertions_bed(wi, names)
    assert open(out / "deletions.bed").read() == ir.deletions_bed(wd, names)
    assert open(out / "junctions.bed").read() == ir.junctions_bed(wj, names)
    assert len(wi) >= 8 and len(wd) >= 8 and len(wj) >= 8
    plain_dir = tmp_path / "without"
    plain_dir.mkdir()
    subprocess.check_call([exe, "--sam-header", str(tmp_path / "hdr.sam"), str(tmp_path / "ref.fa"), str(plain_dir / "junctions.bed"), str(tmp_path / "in.bam")],
                          stderr=subprocess.DEVNULL)
    assert open(plain_dir / "junctions.bed").read() == open(out / "junctions.bed").read()
    assert sorted(os.listdir(plain_dir)) == ["junctions.bed"]
