"""GPU: thj_junctions --sort-bam [--sort-max-mem N] beside --accepted-hits-out (single-end) and --accepted-pairs-out (paired), over the small
inputs the accepted-hits executable tests build.  Three runs each -- without the switch, with it, with it and --sort-max-mem 2000 (many
blocks: the reference's merge path): the sorted files' record streams are the restatement of samtools sort's loop (bamsort_ref.py)
applied to the unsorted run's records, the header is unchanged, every member inflates and is cut where bam_write1's rule cuts, the bed
files are the same in all three runs, the unsorted file is what the accepted-hits tests expect of it, and --sort-bam alone ends the run."""
import os
import re
import zlib

import pytest

import accepted_pair_cases as apc
import accepted_pair_ref as apr
import bamsort_ref as bs
from ingest_cases import bam_header, write_bam
from test_gpu_accepted import NAMES, TARGETS, cfg_of, cut_case, expected, members, order, planted, raw_records, run_exe      # noqa: F401 (order: a fixture)
from test_gpu_binaries_accepted_pair import TARGETS as PAIR_TARGETS, files, run_exe as run_pairs      # noqa: F401 (files: a fixture)
from test_gpu_binaries_reported import members_of, write_ref
from tophat_amd import host
import best_cases as bc

pytestmark = pytest.mark.gpu
DEFAULT_MAX_MEM = 500000000


def held_against_the_restatement(unsorted_path, sorted_path, header, max_mem, stderr):
    """the sorted file against the restatement's order of the unsorted file's records -> how many blocks"""
    base = members(open(unsorted_path, "rb").read())
    assert base[0][0] == header
    raw = bs.split_records(b"".join(m[0] for m in base[1:]))
    recs = [bs.parse_head(x) for x in raw]
    want_order, nb = bs.order(recs, max_mem)
    want = [raw[k] for k in want_order]
    ms = members(open(sorted_path, "rb").read())
    assert all(zlib.crc32(m[0]) & 0xFFFFFFFF == m[1] and len(m[0]) == m[2] for m in ms) and ms[-1][2] == 0      # every member inflates; the empty one ends the file
    assert ms[0][0] == header                                                                                  # the header, in a member of its own, unchanged
    assert b"".join(m[0] for m in ms[1:]) == b"".join(want)
    cuts = host.bgzf_plan_cuts([len(w) for w in want])
    assert [m[2] for m in ms] == [len(header)] + [e - (cuts[k - 1] if k else 0) for k, e in enumerate(cuts)] + [0]
    line = re.search(r"sort bam: (\d+) records in (\d+) blocks? \(--sort-max-mem (\d+)\), [0-9.]+ ms", stderr)
    assert line and (int(line.group(1)), int(line.group(2)), int(line.group(3))) == (len(raw), nb, max_mem), stderr[-600:]
    assert "accepted hits: %d records, %d bytes" % (len(raw), sum(len(x) for x in raw)) in stderr
    assert want_order != list(range(len(raw)))                  # the sort had something to do
    return nb


def test_single_end(tmp_path, order):
    c, raws = cut_case()
    c2 = planted([1, 2, 16, 17, 20, 21, 1, 3], seed=8)
    raws2 = raw_records(c2)
    ref_fa, hdr = write_ref(tmp_path, NAMES, bc.GENOME)
    b1 = write_bam(str(tmp_path / "one.bam"), members_of(raws, 2), targets=TARGETS).path
    b2 = write_bam(str(tmp_path / "two.bam"), members_of(raws2, 7), targets=TARGETS).path
    opts = ["--best-alignments", "--library-type", "fr-firststrand", "--rg-id", "grp"]
    env = {"THJ_PIECE_MEMBERS": "4"}
    outs = {k: str(tmp_path / (k + ".bam")) for k in ("plain", "sorted", "blocks")}
    bed0, err0, _d = run_exe(tmp_path, "plain", ref_fa, hdr, [b1, b2], opts + ["--accepted-hits-out", outs["plain"]], env)
    bed1, err1, _d = run_exe(tmp_path, "sorted", ref_fa, hdr, [b1, b2], opts + ["--accepted-hits-out", outs["sorted"], "--sort-bam"], env)
    bed2, err2, _d = run_exe(tmp_path, "blocks", ref_fa, hdr, [b1, b2], opts + ["--accepted-hits-out", outs["blocks"], "--sort-bam", "--sort-max-mem", "2000"], env)
    assert bed0 == bed1 == bed2 and bed0["junctions.bed"] is not None and "sort bam" not in err0
    # the run without the switch: what the accepted-hits tests expect of the file, member for member
    both = dict(c, recs=c["recs"] + c2["recs"], reads=c["reads"] + [r + 8 for r in c2["reads"]], AS=c["AS"] + c2["AS"], mism=c["mism"] + c2["mism"], anti=c["anti"] + c2["anti"])
    want, _seen = expected(both, raws + raws2, cfg_of(2, "grp"), order)
    header = bam_header(TARGETS, open(hdr).read())
    ms = members(open(outs["plain"], "rb").read())
    cuts = host.bgzf_plan_cuts([len(w) for w in want])
    assert ms[0][0] == header and b"".join(m[0] for m in ms[1:]) == b"".join(want)
    assert [m[2] for m in ms] == [len(header)] + [e - (cuts[k - 1] if k else 0) for k, e in enumerate(cuts)] + [0]
    assert held_against_the_restatement(outs["plain"], outs["sorted"], header, DEFAULT_MAX_MEM, err1) == 1
    assert held_against_the_restatement(outs["plain"], outs["blocks"], header, 2000, err2) > 8
    assert not os.path.exists(outs["sorted"] + ".index")


@pytest.mark.parametrize("name,extra,over,cfg", (
    ("mixed", ["--report-mixed-alignments", "--library-type", "fr-firststrand", "--rg-id", "grp"], {}, apc.cfg_of(2, "grp")),
))
def test_paired(tmp_path, files, name, extra, over, cfg):
    c, raw, ref_fa, hdr, left, right = files
    c = dict(c, **over)
    opts = ["--best-alignments", "--max-multihits", "3"] + extra
    outs = {k: str(tmp_path / (k + ".bam")) for k in ("plain", "sorted", "blocks")}
    r0, bed0 = run_pairs(tmp_path, "plain", ref_fa, hdr, left, right, opts + ["--accepted-pairs-out", outs["plain"]])
    r1, bed1 = run_pairs(tmp_path, "sorted", ref_fa, hdr, left, right, opts + ["--accepted-pairs-out", outs["sorted"], "--sort-bam"])
    r2, bed2 = run_pairs(tmp_path, "blocks", ref_fa, hdr, left, right, opts + ["--accepted-pairs-out", outs["blocks"], "--sort-bam", "--sort-max-mem", "2000"])
    assert r0.returncode == 0 and r1.returncode == 0 and r2.returncode == 0, (r0.stderr[-500:], r1.stderr[-500:], r2.stderr[-500:])
    assert bed0 == bed1 == bed2 and bed0["junctions.bed"].count("\n") > 5 and "sort bam" not in r0.stderr
    want, seen = apr.accepted(c, raw, cfg)
    assert seen["pairs"] > 100 and len(want) > 400
    header = bam_header(PAIR_TARGETS, open(hdr).read())
    ms = members(open(outs["plain"], "rb").read())
    cuts = host.bgzf_plan_cuts([len(w) for w in want])
    assert ms[0][0] == header and b"".join(m[0] for m in ms[1:]) == b"".join(want)
    assert [m[2] for m in ms] == [len(header)] + [e - (cuts[k - 1] if k else 0) for k, e in enumerate(cuts)] + [0]
    assert held_against_the_restatement(outs["plain"], outs["sorted"], header, DEFAULT_MAX_MEM, r1.stderr) == 1
    assert held_against_the_restatement(outs["plain"], outs["blocks"], header, 2000, r2.stderr) > 8
    # both strands are among the records, so the merge's strand rule had a say in where ties across blocks went
    recs = [bs.parse_head(x) for x in want]
    assert {x[2] for x in recs} == {0, 1}


def test_sort_bam_alone_ends_the_run(tmp_path):
    c = planted([2, 3], seed=2)
    raws = raw_records(c)
    ref_fa, hdr = write_ref(tmp_path, NAMES, bc.GENOME)
    bam = write_bam(str(tmp_path / "in.bam"), members_of(raws, 2), targets=TARGETS).path
    r = run_exe(tmp_path, "alone", ref_fa, hdr, [bam], ["--best-alignments", "--sort-bam"], ok=False)
    assert r.returncode != 0 and "--sort-bam needs --accepted-hits-out FILE" in r.stderr
    r = run_exe(tmp_path, "zero", ref_fa, hdr, [bam], ["--best-alignments", "--accepted-hits-out", str(tmp_path / "a.bam"), "--sort-bam", "--sort-max-mem", "0"], ok=False)
    assert r.returncode != 0 and "--sort-max-mem needs a number of bytes of at least 1" in r.stderr
