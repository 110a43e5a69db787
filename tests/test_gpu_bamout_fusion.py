"""GPU: long_spanning_reads --fusion-search with the device-side BAM writer on: a pass that holds fusion alignments stays on the device
(thj_span_bam_encode_records: two records with XF:Z per fusion alignment, thj_k_bam_write_fusion), in one shard and in three, and
writes the stream the host encoder writes (THJ_HOST_BAM=1).  The case is written here (xf_case.py): three random contigs, about 400
chimeric reads of two 50-base pieces in all four directions, 400 plain and spliced reads in between."""
import collections
import gzip
import os
import subprocess

import pytest

import xf_case
from test_gpu_binaries_spliced import index_positions
from tophat_amd.bamio import read_bam

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tophat_amd", "bin")


def xf_tag(rec):
    for t in rec[8:]:
        if str(t).startswith("XF:Z:"):
            return str(t)[5:]
    return None


def test_fusion_alignments_stay_on_the_device(tmp_path):
    case = xf_case.make_case(str(tmp_path / "case"))
    # the case is worth relying on: the CPU oracle finds fusion alignments of every direction in it
    want_dirs = collections.Counter(a.cigar[[(c >> 28) in (7, 8, 9, 10) for c in a.cigar].index(True)] >> 28 for a in case["alns"] if a.is_fusion())
    assert all(want_dirs[d] >= 8 for d in (7, 8, 9, 10)), want_dirs
    runs = {}
    for tag, env in (("one", {"THJ_SHARDS": "1"}), ("three", {"THJ_SHARDS": "3"}), ("host", {"THJ_SHARDS": "1", "THJ_HOST_BAM": "1"})):
        bam = str(tmp_path / ("span_%s.bam" % tag))
        r = subprocess.run(xf_case.lsr_command(BIN, case, bam), capture_output=True, text=True, env=dict(os.environ, **env), timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        runs[tag] = (bam, r.stderr, gzip.open(bam, "rb").read())
    assert runs["one"][2] == runs["host"][2] and runs["three"][2] == runs["host"][2]
    assert index_positions(runs["one"][0]) == index_positions(runs["three"][0]) == index_positions(runs["host"][0])
    assert "made on the device for 1 shard, on the host for 0" in runs["one"][1], runs["one"][1][-1500:]
    assert "made on the device for 3 shards, on the host for 0" in runs["three"][1], runs["three"][1][-1500:]
    for tag in ("one", "three"):
        assert "device-side BAM output not possible" not in runs[tag][1] and "reading on the host" not in runs[tag][1], runs[tag][1][-1500:]
    assert "made on the device" not in runs["host"][1]
    # what came out: the oracle's alignments, fusion alignments of every direction, each one's two records side by side
    _, recs = read_bam(runs["one"][0])
    n_fusion = sum(1 for a in case["alns"] if a.is_fusion())
    assert len(recs) == len(case["alns"]) + n_fusion
    dirs = collections.Counter()
    k = 0
    while k < len(recs):
        xf = xf_tag(recs[k])
        if xf is None:
            k += 1
            continue
        assert xf.startswith("1 ") and k + 1 < len(recs), recs[k][:6]
        nxt = xf_tag(recs[k + 1])
        assert nxt == "2 " + xf[2:] and recs[k + 1][0] == recs[k][0], (recs[k][:6], recs[k + 1][:6])
        dirs[xf_case.direction_of(xf.split(" ")[3])] += 1
        k += 2
    assert sum(dirs.values()) == n_fusion
    assert all(dirs[d] >= 8 for d in ("ff", "fr", "rf", "rr")), dirs
    assert {"ff": want_dirs[7], "fr": want_dirs[8], "rf": want_dirs[9], "rr": want_dirs[10]} == dict(dirs)
