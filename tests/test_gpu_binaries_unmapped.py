"""GPU: thj_junctions --left-reads / --right-reads --unmapped-left-out / --unmapped-right-out --align-summary-out over BAM files made from
the crowds: the two unmapped files inflate to the restatement's records (unmapped_ref.py) in order, align_summary.txt is the restatement's
text, the bed file is that of the run without the options, on the host route and on the device route; and what is refused says so."""
import gzip
import os
import subprocess

import pytest

import accepted_pair_cases as apc
import unmapped_cases as uc
import unmapped_ref as ur
from ingest_cases import bam_header, tag, write_bam
from test_gpu_binaries_reported import EXE, members_of, write_ref
from test_unmapped_cpu import ref_paired, ref_single

pytestmark = pytest.mark.gpu
TARGETS = tuple((n, len(s)) for n, s in zip(apc.NAMES, apc.pc.GENOME))


def raws_of(S, numbers):
    """a side's alignments as BAM records: QNAME = the read's number, the splice strand as XS:A"""
    return [apc.raw_record("%d" % numbers[S["reads"][k]], r, S["anti"][k], S["AS"][k], tag("XS", "A", "-" if r[2] else "+"), S["mism"][k]) for k, r in enumerate(S["recs"])]


def run_exe(tmp_path, name, ref_fa, hdr, left, extra, env=None):
    d = tmp_path / name
    d.mkdir()
    args = [EXE, "--sam-header", str(hdr)] + [str(x).replace("@", str(d)) for x in extra] + [str(ref_fa), str(d / "junctions.bed"), str(left)]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120, env=dict(os.environ, **(env or {})))
    return r, d


def records_of(path, hdr):
    data = gzip.open(path, "rb").read()
    header = bam_header(TARGETS, open(hdr).read())
    assert data[:len(header)] == header
    return data[len(header):]


@pytest.mark.parametrize("route", ({}, {"THJ_DEVICE_INGEST": "1", "THJ_PIECE_MEMBERS": "3"}))
def test_single_end(tmp_path, route):
    c = uc.single_crowd()
    ref_fa, hdr = write_ref(tmp_path, apc.NAMES, apc.pc.GENOME)
    left = write_bam(str(tmp_path / "left.bam"), members_of(raws_of(c, c["numbers"]), 9), targets=TARGETS).path
    reads = write_bam(str(tmp_path / "reads.bam"), members_of(c["file"], 13), targets=()).path
    opts = ["--best-alignments", "--max-multihits", "2", "--read-filters", "--read-mismatches", "0"]
    plain, d0 = run_exe(tmp_path, "plain", ref_fa, hdr, left, opts, route)
    assert plain.returncode == 0, plain.stderr[-800:]
    r, d = run_exe(tmp_path, "um", ref_fa, hdr, left, opts + ["--left-reads", reads, "--unmapped-left-out", "@/unmapped_left.bam", "--align-summary-out", "@/align_summary.txt"], route)
    assert r.returncode == 0, r.stderr[-800:]
    assert open(d / "junctions.bed").read() == open(d0 / "junctions.bed").read()
    want, _r, stats = ref_single(c, (2, False, 6))
    assert len(want) > 50 and records_of(d / "unmapped_left.bam", hdr) == b"".join(want)
    assert open(d / "align_summary.txt").read() == ur.align_summary(stats, 2)
    assert "left reads: %d unmapped records" % len(want) in r.stderr


def test_paired(tmp_path):
    c = uc.paired_crowd()
    ref_fa, hdr = write_ref(tmp_path, apc.NAMES, apc.pc.GENOME)
    left = write_bam(str(tmp_path / "left.bam"), members_of(raws_of(c["L"], c["numbers"]), 9), targets=TARGETS).path
    right = write_bam(str(tmp_path / "right.bam"), members_of(raws_of(c["R"], c["numbers"]), 11), targets=TARGETS).path
    lreads = write_bam(str(tmp_path / "left_reads.bam"), members_of(c["left_file"], 13), targets=()).path
    rreads = write_bam(str(tmp_path / "right_reads.bam"), members_of(c["right_file"], 17), targets=()).path
    opts = ["--best-alignments", "--max-multihits", "2", "--report-mixed-alignments", "--max-report-intron", str(c["max_report_intron"]), "--right-maps", right]
    plain, d0 = run_exe(tmp_path, "plain", ref_fa, hdr, left, opts)
    assert plain.returncode == 0, plain.stderr[-800:]
    r, d = run_exe(tmp_path, "um", ref_fa, hdr, left, opts + ["--left-reads", lreads, "--right-reads", rreads, "--unmapped-left-out", "@/unmapped_left.bam", "--unmapped-right-out",
                                                              "@/unmapped_right.bam", "--align-summary-out", "@/align_summary.txt"], {"THJ_PIECE_MEMBERS": "4"})
    assert r.returncode == 0, r.stderr[-800:]
    assert open(d / "junctions.bed").read() == open(d0 / "junctions.bed").read()
    wl, wr, stats = ref_paired(c, (2, False, 6), (200, 20, 10000000, True, False))
    assert len(wl) > 50 and len(wr) > 50
    assert records_of(d / "unmapped_left.bam", hdr) == b"".join(wl) and records_of(d / "unmapped_right.bam", hdr) == b"".join(wr)
    assert open(d / "align_summary.txt").read() == ur.align_summary(stats, 2)
    # the counters alone: no unmapped file is asked for
    r, d = run_exe(tmp_path, "summary", ref_fa, hdr, left, opts + ["--left-reads", lreads, "--right-reads", rreads, "--align-summary-out", "@/align_summary.txt"])
    assert r.returncode == 0 and open(d / "align_summary.txt").read() == ur.align_summary(stats, 2) and not os.path.exists(d / "unmapped_left.bam")


def test_what_is_refused(tmp_path):
    c = uc.single_case()
    ref_fa, hdr = write_ref(tmp_path, apc.NAMES, apc.pc.GENOME)
    left = write_bam(str(tmp_path / "left.bam"), members_of(raws_of(c, c["numbers"]), 9), targets=TARGETS).path
    reads = write_bam(str(tmp_path / "reads.bam"), members_of(c["file"], 13), targets=()).path
    um = ["--left-reads", reads, "--align-summary-out", "@/align_summary.txt"]
    fq = tmp_path / "reads.fq"
    fq.write_text("@5\nACGT\n+\nIIII\n")
    r, _d = run_exe(tmp_path, "fastq", ref_fa, hdr, left, ["--best-alignments", "--left-reads", fq, "--align-summary-out", "@/a.txt"])
    assert r.returncode != 0 and "FASTQ reads files are not built" in r.stderr, r.stderr[-500:]
    sam = tmp_path / "left.sam"
    sam.write_text(open(hdr).read() + "10\t0\tchrA\t1001\t255\t40M\t*\t0\t0\t%s\t%s\tNM:i:0\tAS:i:0\n" % ("A" * 40, "I" * 40))
    r, _d = run_exe(tmp_path, "sam", ref_fa, hdr, sam, ["--best-alignments"] + um)
    assert r.returncode != 0 and "beside SAM inputs is not built" in r.stderr, r.stderr[-500:]
    r, _d = run_exe(tmp_path, "host", ref_fa, hdr, left, ["--best-alignments"] + um, {"THJ_HOST_INGEST": "1"})
    assert r.returncode != 0 and "THJ_HOST_INGEST=1 is not built" in r.stderr, r.stderr[-500:]
    r, _d = run_exe(tmp_path, "nobest", ref_fa, hdr, left, um)
    assert r.returncode != 0 and "need --best-alignments" in r.stderr
    r, _d = run_exe(tmp_path, "right", ref_fa, hdr, left, ["--best-alignments", "--right-reads", reads] + um)
    assert r.returncode != 0 and "need --right-maps" in r.stderr
    r, _d = run_exe(tmp_path, "noreads", ref_fa, hdr, left, ["--best-alignments", "--align-summary-out", "@/a.txt"])
    assert r.returncode != 0 and "need --left-reads" in r.stderr
    # and the hand-worked single-end case end to end
    r, d = run_exe(tmp_path, "ok", ref_fa, hdr, left, ["--best-alignments", "--max-multihits", "2", "--read-filters", "--unmapped-left-out", "@/u.bam"] + um)
    assert r.returncode == 0, r.stderr[-800:]
    written, stats = c["want"][False]
    assert open(d / "align_summary.txt").read() == ur.align_summary(stats, 2)
    want, _r, _s = ref_single(c)
    assert records_of(d / "u.bam", hdr) == b"".join(want) and len(want) == len(written)
