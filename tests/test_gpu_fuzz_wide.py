"""GPU: the wide-shape batches of wide_fuzz (up to 16 segments and 512 bases) through the real kernels and the C ABI against the oracle:
segment_juncs' instances (thj_k_sj_flat<16>, thj_k_sj_general, thj_k_fusion_wide), the stitch tiers, thj_k_stitch_fusion(_wide) and
thj_k_stitch_huge(_wide) on random hit geometry, passes that mix narrow and wide batches, the 16-op record limit and the shape limits."""
import os

import numpy as np
import pytest

import orc
from test_fusion_long_reads_cpu import rand_long_span_batch
from tophat_amd import host
from tophat_amd.batch import JUNC_DTYPE, SpanBatch, merge_events
from tophat_amd.params import Params
from util import assert_events_equal
from wide_fuzz import (GRID, concat_span, fusion_set_near_hits, genome, n_ops, rand_seg_batch, rand_span_batch, seg_case, seg_with_true_hits,
                       shape_id, short_exon_case, span_case, span_sets)

pytestmark = pytest.mark.gpu
N_CASES = max(len(GRID), int(os.environ.get("THJ_FUZZ_SEEDS", str(len(GRID)))))
CASES = [(k, GRID[k % len(GRID)]) for k in range(N_CASES)]
NO_FUS = np.zeros(0, dtype=orc.SPAN_FUSION_DTYPE)
NO_JUNCS = np.zeros(0, dtype=JUNC_DTYPE)


def case_id(c):
    return "%d-%s" % (c[0], shape_id(c[1]))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_fuzz_wide_segment_juncs_gpu(case):
    seed, shape = case
    seqs, b, p = seg_case(seed, shape, 600)
    g = orc.Genome(seqs)
    want = orc.segjuncs(p, g, b)
    wf = orc.fusions(p, g, b, p.fusion_anchor_length, p.fusion_min_dist)
    assert want.stats["windows"] > 0 and len(want.juncs) > 0
    with host.Context(0) as ctx:
        ctx.upload_genome(host.pack_genome(seqs))
        db = ctx.upload_batch(b)
        got = ctx.segjuncs([(p, db)])
        gf = ctx.fusions([(p, db)])
    assert_events_equal(got, want, "case %s" % case_id(case))
    for k in ("windows", "indel_pairs", "rescue_pairs"):
        assert got.stats[k] == want.stats[k], k
    assert gf.tolist() == wf.tolist()


def run_spanning(ctx, p, seqs, batches):
    return ctx.spanning(p, [ctx.upload_span_batch(sb) for sb in batches], md_resolver=host.span_md_resolver(seqs, batches))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_fuzz_wide_spanning_gpu(case):
    """plain (junctions and insertions), then the fusion tier with fusion search off and on; the tiers the reads took are counted"""
    seed, shape = case
    seqs, sb, p, ja, il, fus = span_case(seed, shape, 600)
    g = orc.Genome(seqs)
    want = orc.spanning(p, g, sb, ja, il)
    assert len({a.read_idx for a in want}) > 50
    with host.Context(0) as ctx:
        ctx.upload_genome(host.pack_genome(seqs))
        ctx.upload_span_sets(ja, il)
        assert run_spanning(ctx, p, seqs, [sb]) == want
        closure, multi, _ = ctx.span_tier_counts()
        # reads reached the multihit list (above eight segments the general kernel takes it as it is), and up to eight segments the
        # closure kernels
        assert multi > 0 and (closure > 0 or sb.nseg > 8), (closure, multi)
        ctx.upload_span_fusions(fus)
        for fs in (0, 1):
            p.fusion_search = fs
            wf = orc.spanning_fusion(p, g, sb, ja, il, fus, bool(fs))
            if fs:
                assert any(a.is_fusion() for a in wf)
            else:
                assert wf == want
            assert run_spanning(ctx, p, seqs, [sb]) == wf, "fusion_search %d" % fs
            assert ctx.span_tier_counts()[1] > 0                   # reads on the multihit list: the fusion tier's input


def test_mixed_narrow_and_wide_batches_in_one_pass():
    """one ctx.fusions pass, one ctx.segjuncs pass and one ctx.spanning pass over a 256-base batch (8 x 32: thj_k_fusion, thj_k_stitch_fusion) and a 512-base
    batch (16 x 32: thj_k_fusion_wide, thj_k_stitch_fusion_wide) on one genome: each batch's reads come out as the oracle gives them for
    that batch alone (the instance is picked per batch)"""
    rng = np.random.default_rng(47003)
    seqs = genome(rng, 2)
    g = orc.Genome(seqs)
    segs = [seg_with_true_hits(rand_seg_batch(rng, seqs, 400, 32, rl // 32, True, rl=rl),
                               rand_long_span_batch(rng, seqs, 400, 32, rl // 32, rl=rl, n_rate=0.005, ends=True)) for rl in (256, 512)]
    p = Params(segment_length=32, read_side=1, fusion_min_dist=1000, inner_dist_mean=50, inner_dist_std_dev=20)
    want = [orc.fusions(p, g, b, p.fusion_anchor_length, p.fusion_min_dist) for b in segs]
    assert len(want[0]) > 0 and len(want[1]) > 0
    sbs = [concat_span(rand_span_batch(rng, seqs, 200, 32, rl // 32, rl=rl),
                       rand_long_span_batch(rng, seqs, 200, 32, rl // 32, rl=rl, n_rate=0.005, ends=True)) for rl in (256, 512)]
    ja, il = span_sets(rng, concat_span(*sbs))
    fl = fusion_set_near_hits(rng, concat_span(*sbs))
    # (at most six mismatches: every MD string fits the device record, none is resolved on the host)
    ps = Params(segment_length=32, read_mismatches=6, read_edit_dist=8, fusion_min_dist=1000)
    with host.Context(0) as ctx:
        ctx.upload_genome(host.pack_genome(seqs))
        dsegs = [ctx.upload_batch(segs[0]), ctx.upload_batch(segs[1], segs[0].n_reads)]        # (read ordinals run on through the pass)
        got = ctx.fusions([(p, db) for db in dsegs])
        assert got.tolist() == orc.merge_fusions(want[0], want[1]).tolist()
        ev = [orc.segjuncs(p, g, b) for b in segs]
        assert_events_equal(ctx.segjuncs([(p, db) for db in dsegs]), merge_events(ev[0], ev[1]))
        ctx.upload_span_sets(ja, il)
        ctx.upload_span_fusions(fl)
        for fs in (0, 1):
            ps.fusion_search = fs
            w0, w1 = (orc.spanning_fusion(ps, g, sb, ja, il, fl, bool(fs)) for sb in sbs)
            assert len(w0) > 50 and len(w1) > 50
            if fs:
                assert any(a.is_fusion() for a in w0) and any(a.is_fusion() for a in w1)
            # the records of batch 0, then those of batch 1, each numbered by its read within its batch
            got = ctx.spanning(ps, [ctx.upload_span_batch(sb) for sb in sbs])
            assert got[:len(w0)] == w0 and got[len(w0):] == w1, "fusion_search %d" % fs


def test_stitch_huge_on_repeat_reads_narrow_and_wide():
    """reads whose every segment hits every copy of a tandem repeat, fusion search on: more joined alignments than a thread keeps, so
    thj_k_stitch_fusion(_wide) hands them to thj_k_stitch_huge(_wide) (THJ_ERETRY grows the workspace; Context.spanning reruns the pass)"""
    for L, nseg, extra, copies, n_reads in ((25, 4, 0, 14, 12), (32, 16, 0, 5, 8), (20, 16, 1, 5, 8), (64, 7, 63, 6, 8)):
        seq, sb = repeat_batch(copies, n_reads, L, nseg, extra, seed=L + nseg)
        fl = repeat_fusions(sb, L)
        p = Params(fusion_search=1, segment_length=L, fusion_min_dist=300, max_report_intron=300, max_seg_multihits=100)
        want = orc.spanning_fusion(p, orc.Genome([seq]), sb, NO_JUNCS, [], fl, True)
        assert len(want) > 96 * n_reads
        with host.Context(0) as ctx:
            ctx.upload_genome(host.pack_genome([seq]))
            ctx.upload_span_sets(NO_JUNCS, [])
            ctx.upload_span_fusions(fl)
            assert run_spanning(ctx, p, [seq], [sb]) == want, (L, nseg, extra)


def repeat_batch(copies, n_reads, L, nseg, extra, seed):
    """test_hostsim_spanning.repeat_span_batch at any shape: reads of nseg x L (+ extra) bases from a `copies`-fold tandem repeat, every
    segment hitting every copy"""
    from tophat_amd.batch import SPAN_HIT_DTYPE
    rng = np.random.default_rng(seed)
    rl = nseg * L + extra
    U = max(400, rl + 150)
    unit = "".join(rng.choice(list("ACGT"), size=U))
    flank = "".join(rng.choice(list("ACGT"), size=3000))
    seq = flank + unit * copies + flank
    hits, seg_off, bases, read_off = [], [0], bytearray(), [0]
    for _r in range(n_reads):
        off = int(rng.integers(0, U - rl))
        for s in range(nseg):
            ln = L if s < nseg - 1 else rl - s * L
            for c in range(copies):
                hits.append((1, 3000 + c * U + off + s * L, 2 if s == nseg - 1 else 0, 0, 0, 1, [(1 << 28) | ln, 0, 0, 0, 0]))
            seg_off.append(len(hits))
        bases += unit[off:off + rl].encode()
        read_off.append(len(bases))
    sb = SpanBatch(nseg, np.arange(1, n_reads + 1, dtype=np.uint32), np.array(read_off, dtype=np.int64),
                   np.frombuffer(bytes(bases), dtype=np.uint8).copy(), np.full(len(bases), ord("I"), dtype=np.uint8),
                   np.array(seg_off, dtype=np.uint32), np.array(hits, dtype=SPAN_HIT_DTYPE))
    return seq, sb


def repeat_fusions(sb, L):
    """test_hostsim_spanning.repeat_fusion_list at segment length L: a break point at every segment boundary, between any two copies"""
    rows = set()
    h = sb.hits
    for r in range(sb.n_reads):
        so = sb.seg_off[r * sb.nseg:(r + 1) * sb.nseg + 1]
        for s_ in range(sb.nseg - 1):
            for a in h[so[s_]:so[s_ + 1]]:
                for b_ in h[so[s_ + 1]:so[s_ + 2]]:
                    if int(b_["left"]) != int(a["left"]) + L:
                        rows.add((1, 1, int(a["left"]) + L - 1, int(b_["left"]), 7))
                        rows.add((1, 1, int(b_["left"]), int(a["left"]) + L - 1, 7))
    return np.array(sorted(rows), dtype=orc.SPAN_FUSION_DTYPE)


def test_more_than_16_cigar_ops_yield_no_alignment():
    """a joined alignment of more than 16 CIGAR ops has no device record.  Reads of 16 x 16 bases over 17..60-base exons: the
    oracle joins some into 17 ops (and more); the device gives the oracle's records minus exactly those, in every path"""
    seqs, sb, ja = short_exon_case()
    g = orc.Genome(seqs)
    p = Params(segment_length=16, min_report_intron=30)
    want = orc.spanning(p, g, sb, ja, [])
    assert sum(1 for a in want if n_ops(a) > 16) >= 10 and sum(1 for a in want if n_ops(a) <= 16) >= 50
    keep = [a for a in want if n_ops(a) <= 16]
    with host.Context(0) as ctx:
        ctx.upload_genome(host.pack_genome(seqs))
        ctx.upload_span_sets(ja, [])
        assert run_spanning(ctx, p, seqs, [sb]) == keep
        ctx.upload_span_fusions(NO_FUS)
        p.fusion_search = 1
        assert orc.spanning_fusion(p, g, sb, ja, [], NO_FUS, True) == want
        assert run_spanning(ctx, p, seqs, [sb]) == keep


def test_shape_limits_are_refused():
    """a 513-base read (nine plane words) or 17 segments: THJ_EINVAL from both stages, nothing run"""
    rng = np.random.default_rng(5)
    seqs = genome(rng, 1)
    p = Params(segment_length=32)
    with host.Context(0) as ctx:
        ctx.upload_genome(host.pack_genome(seqs))
        for rl, L in ((513, 32), (17 * 16, 16)):
            b = rand_seg_batch(rng, seqs, 4, L, rl // L, False, rl=rl)
            with pytest.raises(host.ThjError, match=r"\(-1\)"):
                ctx.segjuncs([(Params(segment_length=L), ctx.upload_batch(b))])
            with pytest.raises(host.ThjError, match=r"\(-1\)"):
                ctx.fusions([(Params(segment_length=L), ctx.upload_batch(b))])
            sb = rand_span_batch(rng, seqs, 4, L, rl // L, rl=rl)
            with pytest.raises(host.ThjError, match=r"\(-1\)"):
                run_spanning(ctx, p, seqs, [sb])


def test_junction_before_a_contig_start_is_listed_last_of_its_contig():
    """regression: a split at a contig's first base gives a junction with left = -1 (0xFFFFFFFF as Junction keeps it).  The device keys
    sort by genome position and listed it first within its contig; Junction::operator< compares left unsigned and lists it last"""
    seqs, b, p = seg_case(4, (135, 8), 600)
    want = orc.segjuncs(p, orc.Genome(seqs), b)
    assert any(int(j["left"]) == 0xFFFFFFFF for j in want.juncs)
    with host.Context(0) as ctx:
        ctx.upload_genome(host.pack_genome(seqs))
        got = ctx.segjuncs([(p, ctx.upload_batch(b))])
    assert got.juncs.tolist() == want.juncs.tolist()
