"""GPU: long_spanning_reads --fusion-search with a junction database that holds fusion contigs, every input BAM: the device-side
ingest splices the fusion contigs' records itself (thj_span_juncdb_fusion_contigs), so the whole device path -- ingest, stitch,
records, BGZF members -- stays on, and the result is what the host readers give and what the fixtures hold."""
import gzip
import os
import subprocess

import pytest

from golden_util import FUSION_SPAN_CASES, GOLD
from tophat_amd.bamio import read_bam, write_bam_from_sam

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tophat_amd", "bin")


def reads_bam_from_fastq(fq, out, tmp_path):
    """the reads as prep_reads leaves them: an unaligned BAM, integer names"""
    lines = open(fq).read().split("\n")
    sam = str(tmp_path / (os.path.basename(out) + ".sam"))
    with open(sam, "w") as f:
        f.write("@HD\tVN:1.0\tSO:unsorted\n")
        for i in range(0, len(lines) - 3, 4):
            f.write("\t".join([lines[i][1:].split()[0], "4", "*", "0", "0", "*", "*", "0", "0", lines[i + 1], lines[i + 3]]) + "\n")
    write_bam_from_sam(sam, out)


@pytest.mark.parametrize("side", ["left", "right"])
@pytest.mark.parametrize("name", FUSION_SPAN_CASES)
def test_fusion_search_all_inputs_bam(name, side, tmp_path):
    d = os.path.join(GOLD, name)
    opts = open(os.path.join(d, "options.txt")).read().split("\n")
    argv = opts[0].split()
    seglen = dict(x.split("=") for x in opts[1].split())["segment_length"]
    nseg = len([f for f in os.listdir(d) if f.startswith("left_seg") and f.endswith(".to_spliced.sam")])
    assert "--fusion-search" in argv and nseg >= 1

    def conv(fn):
        o = str(tmp_path / (fn[:-4] + ".bam"))
        write_bam_from_sam(os.path.join(d, fn), o)
        return o
    segs = [conv("%s_seg%d.sam" % (side, k + 1)) for k in range(nseg)]
    spliced = [conv("%s_seg%d.to_spliced.sam" % (side, k + 1)) for k in range(nseg)]
    assert any("|fus|" in l for l in open(os.path.join(d, "%s_seg1.to_spliced.sam" % side)) if l.startswith("@SQ")), "the junction database has fusion contigs"
    reads = str(tmp_path / ("%s_reads.bam" % side))
    reads_bam_from_fastq(os.path.join(d, "%s.fq" % side), reads, tmp_path)
    want = [tuple(l.rstrip("\n").split("\t")) for l in open(os.path.join(d, "expected.span_%s.sam" % side))]
    want_stream = gzip.open(os.path.join(d, "expected.span_%s.bam" % side), "rb").read()
    streams = {}
    for tag, extra in (("dev", {}), ("host", {"THJ_HOST_INGEST": "1"})):
        bam = str(tmp_path / ("span_%s_%s.bam" % (side, tag)))
        cmd = [os.path.join(BIN, "long_spanning_reads"), "--segment-length", seglen, "--sam-header", os.path.join(d, "hdr.sam")] + argv + [
            os.path.join(d, "ref.fa"), reads, os.path.join(d, "expected.juncs"), os.path.join(d, "expected.insertions"),
            os.path.join(d, "expected.deletions"), os.path.join(d, "expected.fusions"), bam, ",".join(segs), ",".join(spliced)]
        r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, **extra))
        assert r.returncode == 0, r.stderr[-2000:]
        _, recs = read_bam(bam)
        recs = [tuple(str(x) for x in rec) for rec in recs]
        assert recs == want, tag
        assert any(x.startswith("XF:Z:") for rec in recs for x in rec), "fusion alignments (two records with XF:Z) are present"
        streams[tag] = gzip.open(bam, "rb").read()
        assert streams[tag] == want_stream, tag
        if tag == "dev":
            assert "made on the device for 1 shard, on the host for 0" in r.stderr, r.stderr[-1500:]
            assert "declined them: 0" in r.stderr
            assert "reading on the host" not in r.stderr
        else:
            assert "made on the device" not in r.stderr
    assert streams["dev"] == streams["host"]
