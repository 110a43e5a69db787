"""GPU: --fusion-search on reads of more than eight segments or 256 bases (up to 16 and 512) -- thj_k_fusion_wide, thj_k_stitch_fusion_wide
and thj_k_stitch_huge_wide through the C ABI and the executables, against the oracle (stage 2: every shape, up to 480 bases)."""
import os
import subprocess

import numpy as np
import pytest

import orc
from test_fusion_long_reads_cpu import ORACLE_MAXSEQ, SHAPES, family_workload, fusion_list_from_events, stage2_inputs, workload
from tophat_amd import host
from tophat_amd.params import Params

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tophat_amd", "bin")
KEYS = ("ref_id1", "ref_id2", "left", "right", "dir", "count", "edit_dist")


def rows(f):
    return [tuple(int(x[k]) for k in KEYS) for x in f]


def test_stage1_matches_oracle_narrow_and_wide_in_one_pass():
    """every shape's batches, both sides, through ctx.fusions -- and one pass that mixes a 250-base batch (thj_k_fusion) with a 400-base one
    (thj_k_fusion_wide): their events reduce into one set"""
    strs = workload(*SHAPES[0])[0]
    with host.Context(0) as ctx:
        ctx.upload_genome(host.pack_genome(strs))
        for rl, L in SHAPES:
            _, _, _, fz, sides, fus, _ = workload(rl, L)
            runs = [(p, ctx.upload_batch(sb)) for p, sb, _ in sides]
            assert rows(ctx.fusions(runs)) == rows(fus), (rl, L)
            assert len(fus) > 0.8 * len(fz)
        mixed, want = [], None
        for rl, L in ((250, 25), (400, 25)):
            for p, sb, f in workload(rl, L)[4]:
                mixed.append((p, ctx.upload_batch(sb)))
                want = f if want is None else orc.merge_fusions(want, f)
        assert rows(ctx.fusions(mixed)) == rows(want)


@pytest.mark.parametrize("rl,L", SHAPES, ids=lambda v: str(v))
def test_stage2_matches_oracle_or_kernel_logic(rl, L):
    """the oracle's records at every shape: it takes reads of up to 512 bases, so no shape falls back to the kernel logic on the CPU"""
    strs, n, fz, juncs, ins, fl, spb, _ = stage2_inputs(rl, L)
    p = Params(fusion_search=1, fusion_min_dist=100000, segment_length=L)
    assert rl <= ORACLE_MAXSEQ
    want = orc.spanning_fusion(p, orc.Genome(strs), spb, juncs, ins, fl, True)
    with host.Context(0) as ctx:
        ctx.upload_genome(host.pack_genome(strs))
        ctx.upload_span_sets(juncs, ins)
        ctx.upload_span_fusions(fl)
        got = ctx.spanning(p, [ctx.upload_span_batch(spb)], md_resolver=host.span_md_resolver(strs, [spb]))
    assert got == want
    joined = {a.read_idx for a in got if a.is_fusion()}
    assert joined <= fz and len(joined) >= 0.8 * len(fz)


@pytest.mark.parametrize("rl,L", [(250, 25), (400, 25)], ids=lambda v: str(v))
def test_stage1_repeat_family_many_segments(rl, L):
    """the repeat-family shape of test_hostsim_fusions.family_fusion_batches at 10 segments (thj_k_fusion) and 16 segments / 7 words
    (thj_k_fusion_wide): the reads the workgroup takes together, the FusionSimpleSet of the oracle"""
    strs, batches, heavy_pairs, heavy_mates, _ = family_workload(rl, L)
    assert heavy_pairs > 20 and heavy_mates > 20
    g = orc.Genome(strs)
    want = None
    for p, sb in batches:
        f = orc.fusions(p, g, sb, p.fusion_anchor_length, p.fusion_min_dist)
        want = f if want is None else orc.merge_fusions(want, f)
    with host.Context(0) as ctx:
        ctx.upload_genome(host.pack_genome(strs))
        got = ctx.fusions([(p, ctx.upload_batch(sb)) for p, sb in batches])
    assert len(want) > 50 and rows(got) == rows(want)


def test_stage2_repeat_family_ten_segments():
    """2 x 250 bp on the family: its reads through thj_k_stitch_fusion_wide and thj_k_stitch_huge_wide, the oracle's records"""
    from tophat_amd.batch import JUNC_DTYPE
    from bench import sample_spanbatch
    strs, batches, _, _, w = family_workload(250, 25)
    g = orc.Genome(strs)
    fus = None
    for p, sb in batches:
        f = orc.fusions(p, g, sb, p.fusion_anchor_length, p.fusion_min_dist)
        fus = f if fus is None else orc.merge_fusions(fus, f)
    fl = fusion_list_from_events(fus)
    nj = np.zeros(0, dtype=JUNC_DTYPE)
    p = Params(fusion_search=1, segment_length=25, fusion_min_dist=30000)
    spb = sample_spanbatch(w["left"], 2400)
    want = orc.spanning_fusion(p, g, spb, nj, [], fl, True)
    assert any(a.is_fusion() for a in want)
    with host.Context(0) as ctx:
        ctx.upload_genome(host.pack_genome(strs))
        ctx.upload_span_sets(nj, [])
        ctx.upload_span_fusions(fl)
        assert ctx.spanning(p, [ctx.upload_span_batch(spb)], md_resolver=host.span_md_resolver(strs, [spb])) == want


def repeat_span_batch_10(copies, n_reads, seed):
    """test_hostsim_spanning.repeat_span_batch at 2 x 250 bp's shape: reads of ten segments from a `copies`-fold tandem repeat, every segment
    hitting every copy"""
    from tophat_amd.batch import SPAN_HIT_DTYPE, SpanBatch
    rng = np.random.default_rng(seed)
    unit = "".join(rng.choice(list("ACGT"), size=400))
    flank = "".join(rng.choice(list("ACGT"), size=3000))
    seq = flank + unit * copies + flank
    L, nseg, rl = 25, 10, 250
    hits, seg_off, bases, read_off = [], [0], bytearray(), [0]
    for _r in range(n_reads):
        off = int(rng.integers(0, 400 - rl))
        for s in range(nseg):
            for c in range(copies):
                hits.append((1, 3000 + c * 400 + off + s * L, 2 if s == nseg - 1 else 0, 0, 0, 1, [(1 << 28) | L, 0, 0, 0, 0]))
            seg_off.append(len(hits))
        bases += unit[off:off + rl].encode()
        read_off.append(len(bases))
    sb = SpanBatch(nseg, np.arange(1, n_reads + 1, dtype=np.uint32), np.array(read_off, dtype=np.int64),
                   np.frombuffer(bytes(bases), dtype=np.uint8).copy(), np.full(len(bases), ord("I"), dtype=np.uint8),
                   np.array(seg_off, dtype=np.uint32), np.array(hits, dtype=SPAN_HIT_DTYPE))
    return seq, sb


def test_stage2_wave_per_read_wide():
    """reads with more joined alignments than a thread keeps at ten segments: thj_k_stitch_fusion_wide hands them to thj_k_stitch_huge_wide,
    a wave a read -- 6 copies (276 alignments a read) and 20 copies (3 440 a read, 68 800 records for 20 reads)"""
    from test_hostsim_spanning import repeat_fusion_list
    from tophat_amd.batch import JUNC_DTYPE
    nj = np.zeros(0, dtype=JUNC_DTYPE)
    for copies, n_reads in ((6, 30), (20, 20)):
        seq, sb = repeat_span_batch_10(copies, n_reads, 94 + copies)
        fl = repeat_fusion_list(sb)
        pw = Params(fusion_search=1, fusion_min_dist=300, max_report_intron=300)
        want = orc.spanning_fusion(pw, orc.Genome([seq]), sb, nj, [], fl, True)
        assert len(want) == n_reads * (9 * copies * (copies - 1) + copies)
        with host.Context(0) as ctx:
            ctx.upload_genome(host.pack_genome([seq]))
            ctx.upload_span_sets(nj, [])
            ctx.upload_span_fusions(fl)
            assert ctx.spanning(pw, [ctx.upload_span_batch(sb)]) == want


def test_two_by_250_through_both_executables(tmp_path):
    """a paired 2 x 250 bp case with chimeric reads, ten segments: segment_juncs --fusion-search writes the oracle's .fusions byte for byte,
    long_spanning_reads --fusion-search with that list writes the oracle's records, fusion alignments (XF:Z) among them.  (make_case breaks a
    chimeric read anywhere; one in thirty breaks on a segment boundary and has every segment mapped: those are the reads stage 2 joins.)"""
    from golden_util import fusions_text
    from tophat_amd.bamio import read_bam
    from tophat_amd.batch import build_seg_batch, build_span_batch, merge_events
    from tophat_amd.synth import make_case, write_case
    case = make_case(seed=25, paired=True, read_len=250, seg_len=25, n_reads=600, fusion_reads=2500, contig_lens=(60000, 50000, 40000),
                     exon_range=(300, 700))
    d = str(tmp_path / "case")
    paths = write_case(case, d)
    seqs = [orc.fold_genome_char(s) for s in case.seqs]
    og = orc.Genome(seqs)
    extra = dict(fusion_min_dist=1000, inner_dist_mean=50, inner_dist_std_dev=20)
    ev = fus = None
    for sd, side, other in (("left", 1, "right"), ("right", 2, "left")):
        b = build_seg_batch(case.seg_recs[sd], case.reads[sd], case.full_recs[other], case.seg_recs[other][-1])
        assert b.nseg == 10
        p = Params(read_side=side, **extra)
        e = orc.segjuncs(p, og, b)
        f = orc.fusions(p, og, b, p.fusion_anchor_length, p.fusion_min_dist)
        ev = e if ev is None else merge_events(ev, e)
        fus = f if fus is None else orc.merge_fusions(fus, f)
    out = {k: str(tmp_path / ("out." + k)) for k in ("juncs", "insertions", "deletions", "fusions")}
    opts = ["--fusion-search", "--fusion-min-dist", "1000"]
    r = subprocess.run([os.path.join(BIN, "segment_juncs"), "--no-coverage-search", "--no-microexon-search", "--segment-length", "25",
                        "--sam-header", paths["hdr"], "--inner-dist-mean", "50", "--inner-dist-std-dev", "20"] + opts +
                       [paths["ref"], out["juncs"], out["insertions"], out["deletions"], out["fusions"],
                        paths["left_fq"], paths["left_map"], ",".join(paths["left_segs"]),
                        paths["right_fq"], paths["right_map"], ",".join(paths["right_segs"])], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = case.names
    assert open(out["fusions"]).read() == fusions_text(fus, ev.juncs, names, tmp_path)
    fl = orc.read_fusions_file(out["fusions"], {n: i + 1 for i, n in enumerate(names)})
    assert len(fl) > 20
    from tophat_amd.batch import events_to_span_inputs
    jj, ii = events_to_span_inputs(ev)
    n_xf = 0
    for sd in ("left", "right"):
        bam = str(tmp_path / ("span_%s.bam" % sd))
        r = subprocess.run([os.path.join(BIN, "long_spanning_reads"), "--segment-length", "25", "--sam-header", paths["hdr"]] + opts +
                           [paths["ref"], paths["%s_fq" % sd], out["juncs"], out["insertions"], out["deletions"], out["fusions"], bam,
                            ",".join(paths["%s_segs" % sd])], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        sb = build_span_batch(case.seg_recs[sd], case.reads[sd], case.quals[sd])
        alns = orc.spanning_fusion(Params(fusion_search=1, fusion_min_dist=1000), og, sb, jj, ii, fl, True)
        want = []
        for a in alns:
            rid = int(sb.read_id[a.read_idx])
            want += [tuple(str(x) for x in rec) for rec in a.sam_records(rid, names, case.reads[sd][rid], case.quals[sd][rid])]
        _, recs = read_bam(bam)
        got = [tuple(str(x) for x in (rr[0], rr[1], rr[2], rr[3], rr[5], rr[6], rr[7]) + tuple(rr[8:])) for rr in recs]
        assert got == want, sd
        n_xf += sum(1 for rec in got if any(x.startswith("XF:Z:") for x in rec))
    assert n_xf >= 40
