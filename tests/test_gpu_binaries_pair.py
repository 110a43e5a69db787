"""GPU: thj_junctions --right-maps over BAMs written with the helpers of ingest_cases.py: junctions.bed, insertions.bed and deletions.bed byte
for byte against the restatement (pair_ref.py) for the defaults, --report-mixed-alignments and --max-multihits 2 --suppress-hits, the count line, the refusals, and
the same left file without --right-maps."""
import os
import subprocess

import indelbed_cases as ic
import indelbed_ref as ir
import pair_cases as pc
import pair_ref as pr
import pytest
from ingest_cases import cw, record, tag, write_bam
from test_gpu_best import NAMES, TARGETS
from test_gpu_binaries_reported import BAM_OP, EXE, NIB, members_of, write_ref

pytestmark = pytest.mark.gpu


def side_bam(S, seqs, suffix, numbers=None):
    """the records of a side: QNAME = the insert's number, with the /1 or /2 prep_reads may leave"""
    out = []
    for k, (r, sq) in enumerate(zip(S["recs"], seqs)):
        nm = S["mism"][k] + sum(ln for op, ln in r[3] if op in (pc.I, 5))
        aux = tag("NM", "i", nm) + tag("AS", "i" if k % 2 else "c", S["AS"][k]) + tag("XS", "A", "-" if r[2] else "+")
        num = S["reads"][k] if numbers is None else numbers[S["reads"][k]]
        out.append(record("%d%s" % (num, suffix if num % 3 else ""), tid=r[0] - 1, pos=r[1], flag=0x10 if S["anti"][k] else 0, cigar=[cw(BAM_OP[op], ln) for op, ln in r[3]],
                          seq=[NIB[x] for x in sq], aux=aux))
    return out


def run_exe(tmp_path, name, ref_fa, hdr, left, right, extra, env=None):
    d = tmp_path / name
    d.mkdir()
    args = [EXE, "--sam-header", str(hdr), "--insertions-out", str(d / "insertions.bed"), "--deletions-out", str(d / "deletions.bed")] + extra
    args += ([] if right is None else ["--right-maps", str(right)]) + [str(ref_fa), str(d / "junctions.bed"), str(left)]
    r = subprocess.run(args, capture_output=True, text=True, env=dict(os.environ, **(env or {})), timeout=120)
    return r, ({f: open(d / f).read() for f in FILES} if r.returncode == 0 else None)


FILES = ("junctions.bed", "insertions.bed", "deletions.bed")


def text(rows):
    js, ins, dels = rows
    return {"junctions.bed": ir.junctions_bed(js, NAMES), "insertions.bed": ir.insertions_bed(ins, NAMES), "deletions.bed": ir.deletions_bed(dels, NAMES)}


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pairs")
    c = pc.crowd(fusion_ops=False)
    ref_fa, hdr = write_ref(tmp, NAMES, pc.GENOME)
    numbers = {k: 1000 + 7 * k for k in range(600)}             # numbers as prep_reads gives them: rising, not dense
    c["seqs"] = {"L": ic.make_seqs(c["L"]["recs"], 3), "R": ic.make_seqs(c["R"]["recs"], 4)}
    lrec = side_bam(c["L"], c["seqs"]["L"], "/1", numbers)
    rrec = side_bam(c["R"], c["seqs"]["R"], "/2", numbers)
    left = write_bam(str(tmp / "left.bam"), members_of(lrec, 9), targets=TARGETS).path
    right = write_bam(str(tmp / "right.bam"), members_of(rrec, 11), targets=TARGETS).path
    return c, ref_fa, hdr, left, right, lrec, rrec


def test_right_maps(tmp_path, files):
    c, ref_fa, hdr, left, right, _l, _r = files
    mixed = (200, 20, 10000000, True, False)
    settings = {
        "defaults": (["--best-alignments", "--max-multihits", "3"], {}),
        "mixed": (["--best-alignments", "--max-multihits", "3", "--report-mixed-alignments"], {"pair": mixed}),
        "suppressed": (["--best-alignments", "--max-multihits", "2", "--suppress-hits"], {"best": (2, True, 6)}),
        "window": (["--best-alignments", "--max-multihits", "3", "--inner-dist-mean", "150", "--inner-dist-std-dev", "30", "--fusion-min-dist", "900", "--report-discordant-pair-alignments",
                    "--bowtie2-max-penalty", "5"], {"pair": (150, 30, 900, False, True), "best": (3, False, 5)}),
    }
    texts = set()
    for name, (extra, over) in settings.items():
        d = dict(c, **over)
        r, bed = run_exe(tmp_path, name, ref_fa, hdr, left, right, extra, {"THJ_DEVICE_INGEST": "1"} if name == "mixed" else None)
        assert r.returncode == 0, (name, r.stderr[-800:])
        assert bed == text(pr.consensus(d["L"], d["R"], d["best"], d["pair"], seqs=c["seqs"])), name
        assert bed["insertions.bed"].count("\n") > 3 and bed["deletions.bed"].count("\n") > 3, name
        st = pr.choose(d["L"], d["R"], d["best"], d["pair"])["counts"]
        assert "paired alignments: %d inserts with both sides, %d with a pair reported, %d over --max-multihits %d" % (st[0], st[1], st[2], d["best"][0]) in r.stderr, name
        assert "%d singletons, %d reads without a mate's alignment left out" % (st[3], st[4]) in r.stderr, name
        assert "alignment records: read on the host (paired input)" in r.stderr
        assert ("paired input is read on the host" in r.stderr) == (name == "mixed")
        texts.add(repr(bed))
    assert len(texts) == 4


def test_two_files_a_side(tmp_path, files):
    """the files of a side in the order given"""
    c, ref_fa, hdr, left, right, lrec, rrec = files
    # cut between two reads
    at = 400
    while c["L"]["reads"][at] == c["L"]["reads"][at - 1]:
        at += 1
    l1 = write_bam(str(tmp_path / "l1.bam"), members_of(lrec[:at], 50), targets=TARGETS).path
    l2 = write_bam(str(tmp_path / "l2.bam"), members_of(lrec[at:], 50), targets=TARGETS).path
    r, bed = run_exe(tmp_path, "two", ref_fa, hdr, "%s,%s" % (l1, l2), right, ["--best-alignments", "--max-multihits", "3"])
    assert r.returncode == 0, r.stderr[-800:]
    assert bed == text(pr.consensus(c["L"], c["R"], c["best"], c["pair"], seqs=c["seqs"]))
    # the other way round the numbers fall: refused, BamMerge is not built
    r, _ = run_exe(tmp_path, "falls", ref_fa, hdr, "%s,%s" % (l2, l1), right, ["--best-alignments"])
    assert r.returncode != 0 and "BamMerge is not built" in r.stderr


def test_refusals(tmp_path, files):
    c, ref_fa, hdr, left, right, lrec, _r = files
    for name, extra, msg in (("nobest", [], "--right-maps needs --best-alignments"),
                             ("acc", ["--best-alignments", "--accepted-hits-out", str(tmp_path / "a.bam")], "--accepted-hits-out beside --right-maps is not built"),
                             ("fus", ["--best-alignments", "--fusions-out", str(tmp_path / "f.out")], "is not built"),
                             ("fsearch", ["--best-alignments", "--fusion-search"], "--fusion-search grading of pairs is not built"),
                             ("sd0", ["--best-alignments", "--inner-dist-std-dev", "0"], "inner_dist_std_dev")):
        r, _ = run_exe(tmp_path, name, ref_fa, hdr, left, right, extra)
        assert r.returncode != 0 and msg in r.stderr, (name, r.stderr[-500:])
    # a read name that is no number ends the run and is named
    bad = list(lrec)
    rc = c["L"]["recs"][5]
    bad[5] = record("read_five/1", tid=rc[0] - 1, pos=rc[1], cigar=[cw(BAM_OP[op], ln) for op, ln in rc[3]], seq=[NIB["A"]] * sum(ln for op, ln in rc[3] if op in (1, 3)),
                    aux=tag("NM", "i", 0) + tag("AS", "c", 0))
    b = write_bam(str(tmp_path / "named.bam"), members_of(bad, 50), targets=TARGETS).path
    r, _ = run_exe(tmp_path, "named", ref_fa, hdr, b, right, ["--best-alignments"])
    assert r.returncode != 0 and "read_five/1" in r.stderr and "is no read number" in r.stderr
    # a number that read_idx cannot hold says so
    bad[5] = record("4294967296/1", tid=rc[0] - 1, pos=rc[1], cigar=[cw(BAM_OP[op], ln) for op, ln in rc[3]], seq=[NIB["A"]] * sum(ln for op, ln in rc[3] if op in (1, 3)),
                    aux=tag("NM", "i", 0) + tag("AS", "c", 0))
    b = write_bam(str(tmp_path / "large.bam"), members_of(bad, 50), targets=TARGETS).path
    r, _ = run_exe(tmp_path, "large", ref_fa, hdr, b, right, ["--best-alignments"])
    assert r.returncode != 0 and "read number 4294967296 is too large" in r.stderr


def test_without_right_maps_as_before(tmp_path, files):
    """the same left file without --right-maps: the single-end answer over it, as before"""
    import best_ref as br
    c, ref_fa, hdr, left, _right, _l, _r = files
    L = c["L"]
    r, bed = run_exe(tmp_path, "single", ref_fa, hdr, left, None, ["--best-alignments", "--max-multihits", "3"])
    assert r.returncode == 0 and "paired" not in r.stderr
    assert bed == text(br.consensus(L["recs"], c["seqs"]["L"], 8, (), None, L["mism"], (3, False, 6), L["reads"], L["AS"], L["anti"]))
