"""GPU: which of ONE read's sightings wins a contested insertion of stage 1 -- the planted self-contests of tests/ins_tandem.py (a
read inside a tandem repeat whose hits lie on two diagonals and report one place with different letters) through the kernels, the
pair call, the executable's input routes and stage 2's sets.  Every result is compared with the oracle's events bit for bit, and
every contest's place must carry the letters of the sighting the reference visits first: segment pair, then li, then ri -- the
low 16 bits of ins_prio, which the flat2_read hand-off, the four-lanes-a-read and the wave enumerations, the queue's task words
and their three unpackers each restate."""
import os
import subprocess

import pytest

import ins_tandem as it
import orc
from tophat_amd import host
from tophat_amd.batch import events_to_span_inputs, merge_events
from util import assert_events_equal
from xf_case import rewrap_with_index

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tophat_amd", "bin")


@pytest.fixture(scope="module")
def lib():
    return host.load_lib()   # fails loudly when the extension is missing


def _ctx(sc):
    ctx = host.Context(0)
    ctx.upload_genome(host.pack_genome(sc.seqs))
    return ctx


def _check(sc, got, want, what):
    assert_events_equal(got, want, "%s %s" % (sc.name, what))
    it.assert_first_wins(sc, got, what)


@pytest.mark.parametrize("name", it.NAMES)
def test_one_batch(lib, name):
    """every scenario's contests in one batch.  Which kernel a read takes is decided by its hits alone: at most two a segment --
    thj_k_sj_general's first pass (flat2_read) and, as the read has a task, its second; up to 8, up to 32, more: its two instances,
    thj_k_segjuncs_shared; `overflow` fills a workgroup's task queue"""
    sc, want = it.scenario(name), it.expected(name)
    b = sc.batches[0]
    with _ctx(sc) as ctx:
        got = ctx.segjuncs([(sc.params(0), ctx.upload_batch(b.sb, ordinal_base=b.ordinal_base))])
    print(name, "contests", len(sc.contests), {k: got.stats[k] for k in ("windows", "indel_pairs", "overflow_blocks", "hits_read")})
    _check(sc, got, want, "one batch")
    assert got.stats["indel_pairs"] == want.stats["indel_pairs"] and got.stats["windows"] == want.stats["windows"]
    assert got.stats["hits_read"] == len(b.sb.hits)
    nseg = b.rl // sc.L
    per_read = {int(n) for n in (b.sb.seg_off[nseg::nseg] - b.sb.seg_off[:-1:nseg])}
    per_seg = b.sb.seg_off[1:] - b.sb.seg_off[:-1]
    if name == "two":
        assert int(per_seg.max()) == 2 and 6 in per_read
    if name == "paths":
        assert it.PATHS_HITS <= per_read, sorted(per_read)
    if name == "overflow":
        assert got.stats["overflow_blocks"] >= 1


@pytest.mark.parametrize("name", ["two", "paths"])
def test_two_batches_and_their_launch_order(lib, name):
    """the contests' batch as two with ordinal_base running on, launched in both orders: a read's own sightings keep their order
    whatever its ordinal is"""
    sc, want = it.scenario(name), it.expected(name)
    with _ctx(sc) as ctx:
        runs = [(sc.params(0), ctx.upload_batch(sb, ordinal_base=base)) for sb, base in it.halves(sc)]
        _check(sc, ctx.segjuncs(runs), want, "two batches")
        _check(sc, ctx.segjuncs(runs[::-1]), want, "two batches, launched backwards")


def test_pair_call(lib):
    """`two` as the left side of thj_segjuncs_run_pair_async with a plain right batch, and the two sides one after the other"""
    sc, want = it.scenario("two"), it.expected_pair("two")
    with _ctx(sc) as ctx:
        runs = [(sc.params(bi), ctx.upload_batch(sc.batches[bi].sb, ordinal_base=sc.batches[bi].ordinal_base)) for bi in (0, 1)]
        ctx.reset()
        ctx.run_pair(runs[0][0], runs[0][1], runs[1][0], runs[1][1])
        _check(sc, ctx.download(ctx.finish()), want, "pair call")
        _check(sc, ctx.segjuncs(runs), want, "left, right")


def _reads_bam(fq, out, tmp_path):
    """the reads as prep_reads leaves them: an unaligned BAM, integer names"""
    from tophat_amd.bamio import write_bam_from_sam
    lines = open(fq).read().split("\n")
    sam = str(tmp_path / "reads.sam")
    with open(sam, "w") as f:
        f.write("@HD\tVN:1.0\tSO:unsorted\n")
        for i in range(0, len(lines) - 3, 4):
            f.write("\t".join([lines[i][1:].split()[0], "4", "*", "0", "0", "*", "*", "0", "0", lines[i + 1], lines[i + 3]]) + "\n")
    write_bam_from_sam(sam, out)
    rewrap_with_index(out, 100)


@pytest.mark.parametrize("name", ["two", "paths"])
def test_the_executable(lib, name, tmp_path):
    """the scenario as files through segment_juncs, by the host readers (SAM and FASTQ: one shard and one worker; five shards, three
    workers and batches of 100 reads; eight contexts and sixteen shards with the exchange step) and by the device ingest (every
    input a BAM: one shard, and five with batches of 100 reads): segment.insertions equal to the oracle's file, the first sighting's
    letters on every contest's line.  This is the only check that a read's hits of one segment reach the kernels in file order: every
    same-pair contest stands there twice, with either sighting first in the lists, and flips if they do not"""
    import pathlib
    from golden_util import events_text
    from tophat_amd.bamio import write_bam_from_sam
    from tophat_amd.batch import build_seg_batch
    from tophat_amd.samtext import parse_sam_hits, read_fastq
    sc = it.scenario(name)
    d = str(tmp_path / "case")
    paths, names = it.write_files(sc, d)
    ref_ids = {n: i + 1 for i, n in enumerate(names)}
    sides = {sd: dict(reads=read_fastq(paths["%s_fq" % sd]), segs=[list(parse_sam_hits(f, ref_ids, 500000)) for f in paths["%s_segs" % sd]]) for sd in ("left", "right")}
    og = orc.Genome(sc.seqs)
    want = None
    for sd, bi, other in (("left", 0, "right"), ("right", 1, "left")):
        b = build_seg_batch(sides[sd]["segs"], sides[sd]["reads"], [], sides[other]["segs"][-1])
        assert b.n_reads == sc.batches[bi].n_reads
        e = orc.segjuncs(sc.params(bi), og, b)
        want = e if want is None else merge_events(want, e)
    it.assert_first_wins(sc, want, "oracle on the files")
    wt = events_text(want, names, pathlib.Path(d))
    bam = {}
    for k in ("left_map", "right_map"):
        bam[k] = str(tmp_path / (k + ".bam"))
        write_bam_from_sam(paths[k], bam[k])
        rewrap_with_index(bam[k], 100)
    for sd in ("left", "right"):
        bam["%s_segs" % sd] = []
        for n, f in enumerate(paths["%s_segs" % sd]):
            bam["%s_segs" % sd].append(str(tmp_path / ("%s_seg%d.bam" % (sd, n + 1))))
            write_bam_from_sam(f, bam["%s_segs" % sd][-1])
            rewrap_with_index(bam["%s_segs" % sd][-1], 100)         # (as samtools cuts a BAM: no record across two BGZF members)
        bam["%s_fq" % sd] = str(tmp_path / ("%s_reads.bam" % sd))
        _reads_bam(paths["%s_fq" % sd], bam["%s_fq" % sd], tmp_path)
    texts = {}
    for tag, files, env in (("one", paths, {"THJ_SHARDS": "1", "THJ_WORKERS": "1"}), ("many", paths, {"THJ_SHARDS": "5", "THJ_WORKERS": "3", "THJ_BATCH_READS": "100"}),
                            ("ctx8", paths, {"THJ_CTX_PER_GPU": "8", "THJ_SHARDS": "16"}),
                            ("device", bam, {"THJ_SHARDS": "1", "THJ_WORKERS": "1"}), ("device-many", bam, {"THJ_SHARDS": "5", "THJ_WORKERS": "3", "THJ_BATCH_READS": "100"})):
        out = {k: str(tmp_path / ("%s.%s" % (tag, k))) for k in ("juncs", "insertions", "deletions", "fusions")}
        cmd = [os.path.join(BIN, "segment_juncs"), "--no-coverage-search", "--no-microexon-search", "--segment-length", str(sc.L), "--max-insertion-length", str(it.MAX_INS),
               "--sam-header", paths["hdr"], paths["ref"], out["juncs"], out["insertions"], out["deletions"], out["fusions"],
               files["left_fq"], files["left_map"], ",".join(files["left_segs"]), files["right_fq"], files["right_map"], ",".join(files["right_segs"])]
        r = subprocess.run(cmd, capture_output=True, text=True, env=dict({k: v for k, v in os.environ.items() if k != "THJ_HOST_INGEST"}, **env))
        assert r.returncode == 0, r.stderr[-2000:]
        if tag == "device":             # taken by the device-side ingest, no shard handed back to the host readers
            assert "reading on the host" not in r.stderr and "declined them: 0" in r.stderr, r.stderr[-1500:]
        texts[tag] = {k: open(out[k]).read() for k in ("juncs", "insertions", "deletions")}
        for k in ("insertions", "deletions", "juncs"):
            assert texts[tag][k] == wt[k], (tag, k)
        lines = set(texts[tag]["insertions"].splitlines())
        for c in sc.contests:
            assert "%s\t%d\t%d\t%s" % (names[c.key[0] - 1], c.key[1], c.key[1], c.winner) in lines, (tag, c.note)


def test_into_stage_2(lib):
    """thj_span_sets_from_segjuncs after `two`, then its batch stitched: the oracle's spanning records from the oracle's stage-1
    events.  long_spanning_reads joins two segment hits through an insertion of its set only where the read's bases equal the set's
    letters: a self-contest read has alignments through an insertion exactly where the oracle's spanning has them"""
    sc, want = it.scenario("two"), it.expected("two")
    g = orc.Genome(sc.seqs)
    jj, ii = events_to_span_inputs(want)
    sb = it.span_batch(sc, 0)
    p = sc.params(0)
    want_recs = orc.spanning(p, g, sb, jj, ii)
    b = sc.batches[0]
    with _ctx(sc) as ctx:
        ev = ctx.segjuncs([(p, ctx.upload_batch(b.sb, ordinal_base=b.ordinal_base))])
        _check(sc, ev, want, "stage 1")
        ctx.span_sets_from_segjuncs()
        got_recs = ctx.spanning(p, [ctx.upload_span_batch(sb)])
    through = lambda rs, row: [a for a in rs if a.read_idx == row and any((q >> 28) == 3 for q in a.cigar)]      # noqa: E731
    rows = {rid: k for k, rid in enumerate(sb.read_id.tolist())}
    n_through = 0
    for c in sc.contests:
        assert through(got_recs, rows[c.rid]) == through(want_recs, rows[c.rid]), c.note
        n_through += bool(through(want_recs, rows[c.rid]))
    print("contest reads with an alignment through an insertion:", n_through, "of", len(sc.contests))
    assert got_recs == want_recs and len(want_recs) > 300
