"""GPU: the junction consensus with annotated junctions (thj_juncbed_known_junctions, thj_junctions --gtf-juncs) and the read filter
(thj_juncbed_read_filter, thj_junctions --read-filters) against the restatement (jbknown_ref.py) on the planted cases of
jbknown_cases.py, on a crowd with 30 % of its junctions annotated, with the indel and fusion sets collected, and through the
executable on both of its routes."""
import os
import subprocess

import numpy as np
import pytest

import fusionsout_cases as fc
import fusionsout_ref as fr
import indelbed_cases as ic
import indelbed_ref as ir
import jbknown_cases as jc
import jbknown_ref as jr
import orc
from ingest_cases import cw, record, tag, write_bam
from test_gpu_binaries_reported import BAM_OP, EXE, NIB, members_of, write_ref
from tophat_amd import host

pytestmark = pytest.mark.gpu


def alns(recs, mism=None):
    a = host.aln_array_from_tuples(recs)
    if mism is not None:
        a["mismatches"] = mism
    return a


def run(ctx, recs, anchor=8, known=None, limits=None, mism=None, seqs=None):
    """one consensus through the Context -> (junction rows, insertion rows, deletion rows); seqs: the indel sets are collected"""
    ctx.juncbed_reset()
    if seqs is not None:
        ctx.juncbed_collect_indels(True)
    if known is not None:
        ctx.juncbed_known_junctions(known)
    if limits is not None:
        ctx.juncbed_read_filter(True, *limits)
    if seqs is not None:
        ctx.juncbed_add_records_seq(alns(recs, mism), [ir.ins_letters(r[:5], s) for r, s in zip(recs, seqs)])
    else:
        ctx.juncbed_add_records(alns(recs, mism))
    js = ir.junc_rows(ctx.juncbed_finish(anchor))
    if seqs is None:
        return js, [], []
    ins, dels = ctx.juncbed_indels()
    return js, ir.ins_rows(ins), ir.del_rows(dels)


@pytest.fixture(scope="module")
def ctx():
    with host.Context(0) as c:
        c.upload_genome(host.pack_genome(jc.GENOME))
        yield c


def test_annotated_junctions_by_hand(ctx):
    for label, anchor, recs, known, want_j, want_d in jc.KNOWN_CASES:
        seqs = ic.make_seqs(recs, 1)
        got = run(ctx, recs, anchor, known, seqs=seqs)
        assert (got[0], got[2]) == (want_j, want_d), label
        assert got == jr.consensus(recs, seqs, anchor, known), label
        assert run(ctx, recs, anchor, known)[0] == want_j, label                      # and without the indel sets


def test_read_filter_by_hand(ctx):
    other = jc.rec(300, 20, 100, 20)
    for label, rec, nm, outcomes in jc.FILTER_CASES:
        recs, mism = [rec, other], [jr.mismatches(nm, rec[3]), 0]
        seqs = ic.make_seqs(recs, 2)
        for limits, (want_mm, _gap, _ed), want_drop in outcomes:
            assert mism[0] == want_mm
            got = run(ctx, recs, 8, None, limits, mism, seqs)
            assert got == jr.consensus(recs, seqs, 8, (), limits, mism), (label, limits)
            assert len(got[0]) == (1 if want_drop else 2) and (want_drop or len(got[1]) + len(got[2]) == sum(1 for op, _ in rec[3] if op in (jc.I, jc.D))), (label, limits)
        # the filter off: the mismatches field is not looked at
        assert run(ctx, recs, 8, None, None, mism, seqs) == ir.consensus(recs, seqs)


@pytest.mark.parametrize("min_anchor", (8, 12))
def test_crowd_with_a_third_annotated(ctx, min_anchor):
    recs = jc.crowd()
    known = jc.crowd_known(recs)
    want = jr.consensus(recs, min_anchor=min_anchor, known=known)[0]
    plain = jr.consensus(recs, min_anchor=min_anchor)[0]
    assert run(ctx, recs, min_anchor, known)[0] == want
    assert run(ctx, recs, min_anchor)[0] == plain == [tuple(int(x) for x in r)[:7] for r in orc.junction_consensus(orc.jrecs_from_tuples(recs), min_anchor).tolist()]
    # not vacuous: the annotation lets in a junction accept_if_valid turns down and one a stronger neighbour knocks out
    before, kept_before = jr.first_pass(recs, min_anchor)
    after, kept_after = jr.first_pass(recs, min_anchor, known)
    marked = [k for k in known if after[k] == jr.KNOWN]
    assert any(before[k] == jr.REJECTED for k in marked) and any(before[k] == jr.VALID and not kept_before[k] and kept_after[k] for k in marked)
    assert want != plain and len(want) > len(plain) > 50
    # ... with the filter on top: a quarter of the records over the limits
    mism = [int(x) for x in np.random.default_rng(5).integers(0, 4, len(recs))]
    got = run(ctx, recs, min_anchor, known, (2, 2, 2), mism)[0]
    assert got == jr.consensus(recs, min_anchor=min_anchor, known=known, limits=(2, 2, 2), mism=mism)[0] != want


def test_indel_sets_follow_the_annotation_and_the_filter(ctx):
    """indelbed_cases' crowd: indels of lengths 1..3 beside junctions whose anchors are sometimes too short"""
    recs = ic.crowd(seed=5, n_recs=1500)
    seqs = ic.make_seqs(recs, 7)
    distinct = sorted({j[:4] for r in recs for j in ir.rec_juncs(r)})
    known = distinct[::3]
    mism = [int(x) for x in np.random.default_rng(11).integers(0, 4, len(recs))]
    plain = ir.consensus(recs, seqs)
    seen = set()
    for kn, limits in ((known, None), (None, (2, 3, 4)), (known, (2, 2, 3))):
        got = run(ctx, recs, 8, kn, limits, mism, seqs)
        assert got == jr.consensus(recs, seqs, 8, kn or (), limits, mism)
        assert got[1] != plain[1] and got[2] != plain[2] and len(got[1]) > 10 and len(got[2]) > 10
        seen.add(repr(got))
    assert len(seen) == 3
    assert run(ctx, recs, 8, None, None, mism, seqs) == plain


def test_a_filtered_record_is_no_member_of_its_reads_group():
    """fusions collected: with the filter on, every set is what the records under the limits give on their own -- a read with three
    alignments of which one is dropped counts as a read with two (--fusion-multireads 2)"""
    recs = fc.crowd(seed=12, n_reads=300)
    mism = [int(x) for x in np.random.default_rng(3).integers(0, 4, len(recs))]
    limits = (2, 9, 9)
    gone = [jr.dropped(m, r[3], limits) for r, m in zip(recs, mism)]
    live = fc.renumber([r for r, g in zip(recs, gone) if not g])
    want = fr.fusions(live, fc.GENOME)
    assert want != fr.fusions(recs, fc.GENOME) and len(want) >= 4
    sizes = {}
    for r in recs:
        sizes[r[5]] = sizes.get(r[5], 0) + 1
    assert any(sizes[r[5]] == 3 and g for r, g in zip(recs, gone)) and 0 < sum(gone) < len(recs)
    with host.Context(0) as c:
        c.upload_genome(host.pack_genome(fc.GENOME))
        c.juncbed_reset()
        c.juncbed_collect_fusions(True)
        c.juncbed_read_filter(True, *limits)
        c.juncbed_add_records(alns(recs, mism))
        js = ir.junc_rows(c.juncbed_finish(8))
        st = c.juncbed_fusions()
    assert fr.stat_rows(st) == want
    assert js == ir.consensus([r[:5] for r in live])[0]


def test_contract(ctx):
    recs = jc.STRONG + jc.WEAK
    known, both = [(1, 122, 620, 1)], [(1, 119, 620, 0, 20, 20, 3), (1, 122, 620, 1, 20, 20, 1)]
    ctx.juncbed_reset()
    ctx.juncbed_add_records(alns(recs))
    for call in (lambda: ctx.juncbed_known_junctions(known), lambda: ctx.juncbed_read_filter(True), lambda: ctx.juncbed_known_junctions([]), lambda: ctx.juncbed_read_filter(False)):
        with pytest.raises(host.ThjError, match=r"\(-5\).*records were added already"):
            call()
    assert ir.junc_rows(ctx.juncbed_finish(8)) == both[:1]
    # set, then a reset: the plain answer again
    assert run(ctx, recs, 8, known, (0, 0, 0), [1] * 4)[0] == []
    assert run(ctx, recs, 8, known)[0] == both
    assert run(ctx, recs, 8, None, None, [1] * 4)[0] == both[:1]
    # each switch can be taken back before the first add
    ctx.juncbed_reset()
    ctx.juncbed_known_junctions(known)
    ctx.juncbed_read_filter(True, 0, 0, 0)
    ctx.juncbed_known_junctions([])
    ctx.juncbed_read_filter(False)
    ctx.juncbed_add_records(alns(recs, [1] * 4))
    assert ir.junc_rows(ctx.juncbed_finish(8)) == both[:1]
    # entries that can equal no junction are ignored -- and do not stand for the junction their key would fold onto; duplicates, any order,
    # a structured array as well as a list
    odd = [(0, 122, 620, 1), (3, 122, 620, 1), (1, 620, 620, 1), (1, 620, 122, 1), (1, 122, 122 + (1 << 29), 1), (1, 30000, 30100, 0), (2, -2, 50, 0)]
    assert run(ctx, recs, 8, odd)[0] == both[:1]
    assert run(ctx, recs, 8, odd + known * 3 + [(2, 7, 90, 0)])[0] == both
    arr = np.zeros(2, dtype=host.JUNC_DTYPE)
    arr[0], arr[1] = (2, 7, 90, 0), known[0]
    assert run(ctx, recs, 8, arr)[0] == both
    with pytest.raises(host.ThjError, match=r"\(-1\)"):
        ctx.juncbed_reset()
        ctx.juncbed_read_filter(True, -1, 2, 2)


# ---------------------------------------------------------------- the executable

NAMES = ["chrA", "chrB"]
EXE_GENOME = ["ACGT" * 25000, "TTGCA" * 8000]
ANCHOR = 12


def planted():
    """about 50 records: every case of jbknown_cases shifted to a place of its own (contig chrA, 2000 bases apart), the filter cases with
    their NM (one without the tag), and records over the limits on the junctions of good ones -> (records, NMs, SEQs, annotation)"""
    recs, nms, known = [], [], []

    def shift(r, off):
        return (r[0], r[1] + off, r[2], r[3])
    for k, (_label, _anchor, rs, kn, _j, _d) in enumerate(jc.KNOWN_CASES):
        off = 2000 * k
        recs += [shift(r, off) for r in rs]
        nms += [0] * len(rs)
        known += [(ref, l + off, rt + off, a) for ref, l, rt, a in kn]
    for k, (_label, r, nm, _o) in enumerate(jc.FILTER_CASES):
        off = 2000 * (len(jc.KNOWN_CASES) + k)
        recs += [shift(r, off), shift(jc.rec(300, 20, 100, 20), off)]
        nms += [nm, 0]
    for k in range(6):                                         # good records on chrB, and one over the limits that would widen their junction
        recs += [jc.rec(1000 + 900 * k, 20, 300, 20, anti=k % 2 == 1, ref=2)] * 2 + [(2, 990 + 900 * k, k % 2 == 1, [(jc.M, 10), (jc.I, 1), (jc.M, 20), (jc.N, 300), (jc.M, 40)])]
        nms += [0, 1, 3 + k % 2]
    return recs, nms, ic.make_seqs(recs, 23), known


def bam_of(recs, nms, seqs):
    out = []
    for k, (r, nm, sq) in enumerate(zip(recs, nms, seqs)):
        aux = (b"" if nm is None else tag("NM", "i", nm)) + tag("XS", "A", "-" if r[2] else "+")
        out.append(record("r%d" % k, tid=r[0] - 1, pos=r[1], cigar=[cw(BAM_OP[op], ln) for op, ln in r[3]], seq=[NIB[c] for c in sq], aux=aux))
    return out


def thj_junctions(tmp_path, tag_, ref_fa, hdr, bam, extra, env):
    d = tmp_path / tag_
    d.mkdir()
    args = [EXE, "--sam-header", str(hdr), "--min-anchor", str(ANCHOR), "--insertions-out", str(d / "insertions.bed"), "--deletions-out", str(d / "deletions.bed")] + extra
    r = subprocess.run(args + [str(ref_fa), str(d / "junctions.bed"), str(bam)], capture_output=True, text=True, env=dict(os.environ, **env), timeout=120)
    assert r.returncode == 0, (tag_, r.stderr[-1000:])
    return {f: open(d / f).read() for f in ("junctions.bed", "insertions.bed", "deletions.bed")}, r.stderr


def test_thj_junctions_with_the_new_options(tmp_path):
    recs, nms, seqs, known = planted()
    assert 45 <= len(recs) <= 60
    mism = [jr.mismatches(nm, r[3]) for r, nm in zip(recs, nms)]
    ref_fa, hdr = write_ref(tmp_path, NAMES, EXE_GENOME)
    bam = write_bam(str(tmp_path / "in.bam"), members_of(bam_of(recs, nms, seqs), 9), targets=tuple((n, len(s)) for n, s in zip(NAMES, EXE_GENOME))).path
    gtf = tmp_path / "gtf.juncs"
    gtf.write_text("".join("%s\t%d\t%d\t%s\n" % (NAMES[ref - 1], l, rt, "-" if a else "+") for ref, l, rt, a in known) + "chrZ\t1\t2\t+\n" + "chrA\t119\t620\t+\textra\n" * 2)
    known_read = known + [(1, 119, 620, 0)]                     # (case 0's own junction, at offset 0: its record is then kept -- the restatement says so too)

    def text(js, ins, dels):
        return {"junctions.bed": ir.junctions_bed(js, NAMES), "insertions.bed": ir.insertions_bed(ins, NAMES), "deletions.bed": ir.deletions_bed(dels, NAMES)}
    settings = {
        "plain": ([], (), None),
        "gtf": (["--gtf-juncs", str(gtf)], known_read, None),
        "filters": (["--read-filters"], (), (2, 2, 2)),
        "both": (["--gtf-juncs", str(gtf), "--read-filters", "--read-edit-dist", "3"], known_read, (2, 2, 3)),
        "limits_without_the_switch": (["--read-mismatches", "0", "--read-gap-length", "0", "--read-edit-dist", "0"], (), None),
    }
    wants = {}
    for name, (extra, kn, limits) in settings.items():
        want = text(*jr.consensus(recs, seqs, ANCHOR, kn, limits, mism))
        wants[name] = want
        host_got, host_err = thj_junctions(tmp_path, name + "_host", ref_fa, hdr, bam, extra, {"THJ_HOST_INGEST": "1"})
        dev_got, dev_err = thj_junctions(tmp_path, name + "_dev", ref_fa, hdr, bam, extra, {"THJ_DEVICE_INGEST": "1", "THJ_PIECE_MEMBERS": "2"})
        assert "alignment records: read on the host (THJ_HOST_INGEST)" in host_err and "alignment records: parsed on the device for" in dev_err
        assert host_got == want, name
        assert dev_got == host_got, name
        if kn:
            assert "Loaded %d GFF junctions from %s.\n" % (len(set(known_read)), gtf) in host_err and "Loaded %d GFF junctions" % len(set(known_read)) in dev_err
    # without the new options: today's files, which the oracle and indelbed_ref give
    assert wants["plain"] == wants["limits_without_the_switch"] == text(*ir.consensus(recs, seqs, ANCHOR))
    assert wants["plain"]["junctions.bed"] == orc.junctions_bed(orc.junction_consensus(orc.jrecs_from_tuples(recs), ANCHOR), NAMES)
    assert len({repr(wants[k]) for k in ("plain", "gtf", "filters", "both")}) == 4
    assert wants["gtf"]["deletions.bed"] != wants["plain"]["deletions.bed"] and wants["filters"]["insertions.bed"] != wants["plain"]["insertions.bed"]


def test_thj_junctions_filters_fusion_alignments_by_the_cigar_of_their_tag(tmp_path):
    """fusion alignments in their two-record XF:Z form with NM = all their indel bases: the reference subtracts the I and D of the cigar
    rebuilt from the tag -- not the i and d of pieces that run down the genome, and not the 10M of the records' own columns -- so a record
    with more than two lower-case indel bases is dropped at --read-mismatches 2 although every mismatch it has is an indel"""
    from test_gpu_binaries_reported import bam_records
    M, m, I, i_, D, d, FR, RF = 1, 2, 3, 4, 5, 6, 8, 9
    base = ic.fusion_indel_cases() + [(1, 2500, False, [(M, 25), (I, 1), (M, 20), (FR, 9100), (m, 15), (d, 2), (m, 25)], 2),      # two lower-case bases: kept
                                      (2, 4500, False, [(m, 20), (i_, 1), (m, 24), (RF, 800), (M, 30), (D, 2), (M, 15)], 1)]      # one
    recs = [r[:4] + (r[4] if len(r) > 4 else 0, "q%d" % k, jr.gap_length(r[3])) for k, r in enumerate(base)]
    mism = [jr.mismatches(r[6], r[3]) for r in recs]
    lower = [sum(ln for op, ln in r[3] if op in (4, 6)) for r in recs]
    assert mism == lower and any(m > 2 for m in mism) and any(0 < m <= 2 for m in mism) and any(m == 0 and r[6] > 2 for m, r in zip(mism, recs))
    seqs = ic.make_seqs(recs, 31)
    ref_fa, hdr = write_ref(tmp_path, ic.NAMES, ic.GENOME)
    bam = write_bam(str(tmp_path / "in.bam"), members_of(bam_records(recs, seqs, ic.NAMES), 5), targets=tuple((n, len(s)) for n, s in zip(ic.NAMES, ic.GENOME))).path
    limits = (2, 99, 99)
    extra = ["--read-filters", "--read-gap-length", "99", "--read-edit-dist", "99"]
    js, ins, dels = jr.consensus([r[:5] for r in recs], seqs, ANCHOR, (), limits, mism)
    want = {"junctions.bed": ir.junctions_bed(js, ic.NAMES), "insertions.bed": ir.insertions_bed(ins, ic.NAMES), "deletions.bed": ir.deletions_bed(dels, ic.NAMES)}
    plain = ir.consensus([r[:5] for r in recs], seqs, ANCHOR)
    assert (js, ins, dels) != plain and len(ins) < len(plain[1]) and len(dels) < len(plain[2]) and len(dels) > 3
    host_got, _ = thj_junctions(tmp_path, "host", ref_fa, hdr, bam, extra, {"THJ_HOST_INGEST": "1"})
    dev_got, dev_err = thj_junctions(tmp_path, "dev", ref_fa, hdr, bam, extra, {"THJ_DEVICE_INGEST": "1"})
    assert "parsed on the device" in dev_err
    assert host_got == want and dev_got == want


def test_thj_junctions_keeps_the_switches_over_the_host_fallback(tmp_path):
    """a record that straddles two BGZF members: the device route declines the file, the consensus is reset and read again by the
    host readers -- with the annotation and the filter set again"""
    recs, nms, seqs, known = planted()
    mism = [jr.mismatches(nm, r[3]) for r, nm in zip(recs, nms)]
    ref_fa, hdr = write_ref(tmp_path, NAMES, EXE_GENOME)
    r = bam_of(recs, nms, seqs)
    bam = write_bam(str(tmp_path / "cut.bam"), [(r[:20] + [r[20][:30]], 6), ([r[20][30:]] + r[21:], 6)], targets=tuple((n, len(s)) for n, s in zip(NAMES, EXE_GENOME))).path
    gtf = tmp_path / "gtf.juncs"
    gtf.write_text("".join("%s\t%d\t%d\t%s\n" % (NAMES[ref - 1], l, rt, "-" if a else "+") for ref, l, rt, a in known))
    got, err = thj_junctions(tmp_path, "fallback", ref_fa, hdr, bam, ["--gtf-juncs", str(gtf), "--read-filters"], {"THJ_DEVICE_INGEST": "1"})
    assert "alignment records: read on the host (" in err and "straddle" in err
    js, ins, dels = jr.consensus(recs, seqs, ANCHOR, known, (2, 2, 2), mism)
    assert got == {"junctions.bed": ir.junctions_bed(js, NAMES), "insertions.bed": ir.insertions_bed(ins, NAMES), "deletions.bed": ir.deletions_bed(dels, NAMES)}
    assert got["junctions.bed"] != ir.junctions_bed(ir.consensus(recs, seqs, ANCHOR)[0], NAMES)
