"""GPU: thj_junctions --right-maps --accepted-pairs-out over BAM files made from the crowd: the output BAM inflates to the restatement's records
(accepted_pair_ref.py) in order, the three bed files are those of the run without the switch, and what stays refused beside it says so."""
import gzip
import os
import subprocess

import pytest

import accepted_pair_cases as apc
import accepted_pair_ref as apr
from ingest_cases import bam_header, tag, write_bam
from test_gpu_binaries_reported import EXE, members_of, write_ref
from tophat_amd import bamio

pytestmark = pytest.mark.gpu
TARGETS = tuple((n, len(s)) for n, s in zip(apc.NAMES, apc.pc.GENOME))
FILES = ("junctions.bed", "insertions.bed", "deletions.bed")


def run_exe(tmp_path, name, ref_fa, hdr, left, right, extra):
    d = tmp_path / name
    d.mkdir()
    args = [EXE, "--sam-header", str(hdr), "--insertions-out", str(d / "insertions.bed"), "--deletions-out", str(d / "deletions.bed")] + extra
    args += ["--right-maps", str(right), str(ref_fa), str(d / "junctions.bed"), str(left)]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    return r, ({f: open(d / f).read() for f in FILES} if r.returncode == 0 else None)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("accpairs")
    c = apc.crowd()
    # the splice strand travels as XS:A (the executable reads it from there), beside the crowd's other tags
    sides = {"L": c["L"], "R": c["R"]}
    raw = apc.raw_of(c, lambda s, k: tag("XS", "A", "-" if sides[s]["recs"][k][2] else "+") + (b"" if k % 7 == 3 else apc.crowd_extra(s, k)))
    ref_fa, hdr = write_ref(tmp, apc.NAMES, apc.pc.GENOME)
    left = write_bam(str(tmp / "left.bam"), members_of(raw["L"], 9), targets=TARGETS).path
    right = write_bam(str(tmp / "right.bam"), members_of(raw["R"], 11), targets=TARGETS).path
    return c, raw, ref_fa, hdr, left, right


@pytest.mark.parametrize("name,extra,over,cfg", (
    ("mixed", ["--report-mixed-alignments", "--library-type", "fr-firststrand", "--rg-id", "grp"], {}, apc.cfg_of(2, "grp")),
    ("discordant", ["--report-discordant-pair-alignments"], {"pair": (200, 20, 10000000, False, True)}, apc.cfg_of()),
))
def test_accepted_hits_for_pairs(tmp_path, files, name, extra, over, cfg):
    c, raw, ref_fa, hdr, left, right = files
    c = dict(c, **over)
    opts = ["--best-alignments", "--max-multihits", "3"] + extra
    plain, bed0 = run_exe(tmp_path, "plain", ref_fa, hdr, left, right, opts)
    assert plain.returncode == 0, plain.stderr[-800:]
    out = str(tmp_path / "accepted_hits.bam")
    r, bed = run_exe(tmp_path, "acc", ref_fa, hdr, left, right, opts + ["--accepted-pairs-out", out])
    assert r.returncode == 0, r.stderr[-800:]
    assert bed == bed0 and bed["junctions.bed"].count("\n") > 5           # the three bed files, byte for byte
    want, seen = apr.accepted(c, raw, cfg)
    assert seen["pairs"] > 100 and len(want) > 400
    data = gzip.open(out, "rb").read()
    header = bam_header(TARGETS, open(hdr).read())
    assert data[:len(header)] == header and data[len(header):] == b"".join(want)
    names, recs = bamio.read_bam(out)
    assert names == apc.NAMES and list(recs) == [bamio.parse_bam_record(w[4:], apc.NAMES) for w in want]
    assert "accepted hits: %d records, %d bytes" % (len(want), sum(len(w) for w in want)) in r.stderr and not os.path.exists(out + ".index")


def test_what_stays_refused(tmp_path, files):
    _c, _raw, ref_fa, hdr, left, right = files
    out = ["--best-alignments", "--accepted-pairs-out", str(tmp_path / "a.bam")]
    sam = tmp_path / "left.sam"
    sam.write_text(open(hdr).read() + "0\t0\tchrA\t1001\t255\t40M\t*\t0\t0\t%s\t%s\tNM:i:0\tAS:i:0\n" % ("A" * 40, "I" * 40))
    r, _ = run_exe(tmp_path, "sam", ref_fa, hdr, sam, right, out)
    assert r.returncode != 0 and "accepted hits need BAM inputs of whole BGZF members" in r.stderr, r.stderr[-500:]
    r, _ = run_exe(tmp_path, "fus", ref_fa, hdr, left, right, out + ["--fusions-out", str(tmp_path / "f.out")])
    assert r.returncode != 0 and "is not built" in r.stderr
    r, _ = run_exe(tmp_path, "fsearch", ref_fa, hdr, left, right, out + ["--fusion-search"])
    assert r.returncode != 0 and "--fusion-search grading of pairs is not built" in r.stderr
    # the single-end switch beside --right-maps stays refused and names the paired one
    r, _ = run_exe(tmp_path, "single", ref_fa, hdr, left, right, ["--best-alignments", "--accepted-hits-out", str(tmp_path / "b.bam")])
    assert r.returncode != 0 and "--accepted-hits-out beside --right-maps is not built" in r.stderr and "--accepted-pairs-out" in r.stderr
