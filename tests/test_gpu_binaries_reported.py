"""GPU: thj_junctions on its device route (THJ_DEVICE_INGEST=1: the alignment BAMs inflated and parsed on the device,
thj_juncbed_add_bam) with pieces of 1 and 3 BGZF members and of the default size, against its host route (THJ_HOST_INGEST=1): all four output files byte-identical, and the
line on stderr that says which route was taken.  Inputs: the reference's nine regression cases (their recorded bed files still come
out byte for byte), the fusion crowd of test_gpu_fusionsout, the spanning BAMs of two --fusion-search golden cases, and a BAM whose
records straddle members (the device route declines it)."""
import os
import re
import subprocess

import pytest

import fusionsout_cases as fc
import fusionsout_ref as fr
import indelbed_ref as ir
import ref_regression as rr
from ingest_cases import cw, record, tag, write_bam

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EXE = os.path.join(ROOT, "tophat_amd", "bin", "thj_junctions")
BAM_OP = {1: 0, 3: 1, 5: 2, 11: 3, 13: 4}
NIB = {"=": 0, "A": 1, "C": 2, "G": 4, "T": 8, "N": 15}
LETTER = {1: "M", 2: "m", 3: "I", 4: "i", 5: "D", 6: "d", 11: "N", 12: "n", 13: "S"}
DEV = {"THJ_DEVICE_INGEST": "1"}                        # the device route is opt-in (it measured no faster than the host readers)
ROUTES = (("pieces_of_1", dict(DEV, THJ_PIECE_MEMBERS="1")), ("pieces_of_3", dict(DEV, THJ_PIECE_MEMBERS="3")), ("default", DEV),
          ("host", dict(DEV, THJ_HOST_INGEST="1")))
FILES = ("junctions.bed", "insertions.bed", "deletions.bed", "fusions.out")


def bam_records(recs, seqs, names, qnames=None):
    """(ref_id, left, antisense_splice, [(op, len)][, ref_id2, read, edit_dist]) -> BAM records; a fusion alignment as its two XF:Z
    records (bwt_map.cpp:2047-2083)"""
    out = []
    for k, (rec, sq) in enumerate(zip(recs, seqs)):
        ref, left, anti, cig = rec[:4]
        ref2 = rec[4] if len(rec) > 4 else 0
        name = str(rec[5]) if len(rec) > 5 else (qnames[k] if qnames else "r%d" % k)
        aux = tag("NM", "i", rec[6] if len(rec) > 6 else 0) + tag("XS", "A", "-" if anti else "+")
        if ref2:
            cg = "".join("%d%s" % ((ln + 1, "F") if op in (7, 8, 9, 10) else (ln, LETTER[op])) for op, ln in cig)
            xf = "%s-%s %d %s %s %s" % (names[ref - 1], names[ref2 - 1], left + 1, cg, sq, "I" * len(sq))
            for part, tid, pos in (("1", ref - 1, left), ("2", ref2 - 1, 6)):
                out.append(record(name, tid=tid, pos=pos, cigar=[cw(0, 10)], seq=[1] * 10, aux=aux + tag("XF", "Z", part + " " + xf)))
        else:
            out.append(record(name, tid=ref - 1, pos=left, cigar=[cw(BAM_OP[op], ln) for op, ln in cig], seq=[NIB[c] for c in sq], aux=aux))
    return out


def members_of(records, per):
    return [(records[i:i + per], 6) for i in range(0, len(records), per)] or [([], 6)]


def run_routes(tmp_path, ref_fa, hdr_sam, bams, opts, expect_host=None):
    """thj_junctions once per route -> {route: {file: text}}; the route lines are checked here"""
    got = {}
    for route, env in ROUTES:
        d = tmp_path / route
        d.mkdir()
        args = [EXE, "--sam-header", str(hdr_sam)]
        for o, f in opts:
            args += [o, str(d / f)]
        args += [str(ref_fa), str(d / "junctions.bed"), ",".join(str(b) for b in bams)]
        r = subprocess.run(args, capture_output=True, text=True, env=dict(os.environ, **env), timeout=120)
        assert r.returncode == 0, (route, r.stderr[-1000:])
        lines = [l for l in r.stderr.split("\n") if l.startswith("alignment records: ")]
        assert len(lines) == 1, (route, r.stderr[-1000:])
        if route == "host":
            assert lines[0] == "alignment records: read on the host (THJ_HOST_INGEST)"
        elif expect_host:
            assert re.fullmatch(r"alignment records: read on the host \(.*%s.*\)" % expect_host, lines[0]), lines[0]
        else:
            m = re.fullmatch(r"alignment records: parsed on the device for (\d+) pieces?", lines[0])
            assert m, (route, lines[0])
            got.setdefault("pieces", {})[route] = int(m.group(1))
        got[route] = {f: open(d / f).read() for f in FILES if os.path.exists(d / f)}
        assert set(got[route]) == {"junctions.bed"} | {f for _o, f in opts}
    for route, _env in ROUTES[:-1]:
        assert got[route] == got["host"], route
    return got


def write_ref(tmp_path, names, seqs):
    open(tmp_path / "ref.fa", "w").write("".join(">%s\n%s\n" % (n, s) for n, s in zip(names, seqs)))
    open(tmp_path / "hdr.sam", "w").write("@HD\tVN:1.0\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % (n, len(s)) for n, s in zip(names, seqs)))
    return tmp_path / "ref.fa", tmp_path / "hdr.sam"


INDEL_OPTS = (("--insertions-out", "insertions.bed"), ("--deletions-out", "deletions.bed"))


@pytest.mark.parametrize("case", rr.CASES)
def test_recorded_cases_through_every_route(tmp_path, case):
    recs = rr.recorded_alignment_records(case)
    seqs = ir.recorded_seqs(rr.GOLD, case)
    genome = "".join(l.strip() for l in open(os.path.join(rr.GOLD, case, "genome.fa")) if not l.startswith(">"))
    ref_fa, hdr = write_ref(tmp_path, ["fake"], [genome])
    w = write_bam(str(tmp_path / "in.bam"), members_of(bam_records(recs, seqs, ["fake"]), 7), targets=(("fake", len(genome)),))
    got = run_routes(tmp_path, ref_fa, hdr, [w.path], INDEL_OPTS)
    for f in FILES[:3]:
        assert got["default"][f] == open(os.path.join(rr.GOLD, case, f)).read(), f
    n_members = len(w.member_len)
    assert got["pieces"]["default"] == 1 and got["pieces"]["pieces_of_1"] == n_members and got["pieces"]["pieces_of_3"] == (n_members + 2) // 3


def test_fusion_crowd_through_every_route(tmp_path):
    names, seqs = fc.NAMES, fc.GENOME
    ref_fa, hdr = write_ref(tmp_path, names, seqs)
    recs = fc.crowd(seed=12, n_reads=150)
    assert {sum(1 for r in recs if r[5] == k) for k in range(150)} >= {1, 2, 3}
    rseq = []
    for rec in recs:
        n = sum(ln for op, ln in rec[3] if op in (1, 2))
        rseq.append("ACGT" * (n // 4) + "ACGT"[:n % 4])
    records = bam_records(recs, rseq, names)
    bams = [write_bam(str(tmp_path / "a.bam"), members_of(records, 25), targets=tuple((n, len(s)) for n, s in zip(names, seqs))).path]
    got = run_routes(tmp_path, ref_fa, hdr, bams, (("--fusions-out", "fusions.out"),))
    want = fr.fusions_out(fr.fusions(recs, seqs), names)
    assert got["default"]["fusions.out"] == want and want.count("\n") >= 4
    assert got["default"]["junctions.bed"] == ir.junctions_bed(ir.consensus([r[:5] for r in recs])[0], names)
    assert got["pieces"]["pieces_of_1"] > got["pieces"]["pieces_of_3"] > got["pieces"]["default"] == 1


@pytest.mark.parametrize("case", ["pe100_fusion_span", "pe100_fusion_span3"])
def test_spanning_bams_of_a_fusion_search(tmp_path, case):
    d = os.path.join(HERE, "golden", case)
    bams = [os.path.join(d, "expected.span_%s.bam" % sd) for sd in ("left", "right")]
    got = run_routes(tmp_path, os.path.join(d, "ref.fa"), os.path.join(d, "hdr.sam"), bams, INDEL_OPTS + (("--fusions-out", "fusions.out"),))
    assert got["default"]["fusions.out"].count("\n") >= 1 and got["default"]["junctions.bed"].count("\n") >= 2
    assert got["pieces"]["default"] == 2


def test_a_straddling_record_takes_the_host_route(tmp_path):
    names, seqs = fc.NAMES, fc.GENOME
    ref_fa, hdr = write_ref(tmp_path, names, seqs)
    recs = fc.crowd(seed=3, n_reads=40)
    rseq = ["A" * sum(ln for op, ln in rec[3] if op in (1, 2)) for rec in recs]
    r = bam_records(recs, rseq, names)
    w = write_bam(str(tmp_path / "cut.bam"), [(r[:20] + [r[20][:30]], 6), ([r[20][30:]] + r[21:], 6)], targets=tuple((n, len(s)) for n, s in zip(names, seqs)))
    got = run_routes(tmp_path, ref_fa, hdr, [w.path], (("--fusions-out", "fusions.out"),), expect_host="straddle")
    assert got["host"]["fusions.out"] == fr.fusions_out(fr.fusions(recs, seqs), names)


def test_without_the_switch_the_host_readers_are_taken(tmp_path):
    names, seqs = fc.NAMES, fc.GENOME
    ref_fa, hdr = write_ref(tmp_path, names, seqs)
    recs = fc.crowd(seed=3, n_reads=10)
    w = write_bam(str(tmp_path / "in.bam"), members_of(bam_records(recs, ["A" * sum(ln for op, ln in rec[3] if op in (1, 2)) for rec in recs], names), 10),
                  targets=tuple((n, len(s)) for n, s in zip(names, seqs)))
    env = {k: v for k, v in os.environ.items() if k not in ("THJ_DEVICE_INGEST", "THJ_HOST_INGEST")}
    r = subprocess.run([EXE, "--sam-header", str(hdr), str(ref_fa), str(tmp_path / "junctions.bed"), w.path], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and "alignment records: read on the host (THJ_DEVICE_INGEST is not set)" in r.stderr
