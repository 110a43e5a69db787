"""GPU, test_gpu_fullsize_fusion's properties at 2 x 250 bp (ten segments: thj_k_stitch_fusion_wide, thj_k_stitch_huge_wide) and 2 M pairs:
2 % of the pairs with a chimeric left read, and a nine-copy repeat family further apart than --fusion-min-dist (5 % of the pairs), whose
reads with nine or more (first, second segment) hit pairs go to thj_k_stitch_huge_wide a wave a read -- some 15 000 of them, in all its
workgroups (a pass that answers THJ_ERETRY is run again, as the executables do).

* the planted fusions are found (stage 1) and the chimeric reads are joined through them (stage 2);
* sample parity: stage-1 fusions of the first reads are among the full run's; the stage-2 records of the first reads equal the oracle's
  given the full junction / fusion sets;
* idempotence, and two half batches concatenate to the full batch's records;
* structure: one fusion op per fusion alignment, its second contig valid, every CIGAR spans the read;
* the reads that are neither chimeric nor from the family come out exactly as they do with fusion search off.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import orc
from bench import CHR20_LEN, cbatch_from_tensors, sample_segbatch, sample_spanbatch, span_cbatch_from_tensors
from test_gpu_fullsize_properties import half
from test_scale_workload_cpu import fusion_list_from_events
from tophat_amd import host
from tophat_amd.batch import events_to_span_inputs
from tophat_amd.params import Params, READ_LEFT, READ_RIGHT
from tophat_amd.synth import make_device_workload, make_scale_genome

pytestmark = pytest.mark.gpu
PAIRS = 2_000_000
RL = 250


def span_pass(ctx, p, sp):
    """one pass, run again while thj_span_finish answers THJ_ERETRY (a pool or the workspace was enlarged) -> (records, passes)"""
    for k in range(1, 5):
        ctx.span_reset()
        ctx.span_run(p, sp)
        n = C.c_int64()
        rc = ctx.lib.thj_span_finish(ctx._ctx, C.byref(n))
        if rc != -7:
            break
    assert rc == 0, rc
    return ctx.span_download(n.value).copy(), k


def test_fullsize_fusion_search_two_by_250():
    dev = torch.device("cuda", 0)
    seqs, genes = make_scale_genome(1, [CHR20_LEN // 2, CHR20_LEN // 4, CHR20_LEN // 4], 20000, exon_len=600)
    S, copies = 120_000, 9
    for k in range(1, copies):
        seqs[0][k * S:(k + 1) * S] = seqs[0][:S]
    fam = (genes[:, 0] == 0) & (genes[:, 3] + 600 + 1000 < S)
    uniq = (genes[:, 0] != 0) | (genes[:, 1] >= copies * S + 1000)
    genes = genes[fam | uniq]
    strs = [s.tobytes().decode() for s in seqs]
    w = make_device_workload(100, seqs, genes, None, PAIRS, dev, exon_len=600, read_len=RL, fusion_frac=0.02, multi_frac=0.05,
                             dup_shift=S, max_copies=copies)
    torch.cuda.synchronize()
    assert w["left"]["nseg"] == 10
    fz = w["left"]["fusion_reads"].cpu().numpy()
    assert 0.015 * PAIRS < len(fz) < 0.025 * PAIRS
    so = w["left"]["span_off"].cpu().numpy().astype(np.int64)
    cnt = np.diff(so).reshape(PAIRS, 10)
    multi = np.nonzero((cnt > 1).any(1))[0]                                   # the family's reads
    assert len(multi) > 0.02 * PAIRS
    assert ((cnt[:, 0] * cnt[:, 1]) >= 9).sum() > 0.005 * PAIRS                # fusion_read_heavy: reads for the wave of thj_k_stitch_huge_wide
    stream = torch.cuda.Stream(device=dev)
    kw = dict(inner_dist_mean=50, inner_dist_std_dev=20, fusion_min_dist=100000)
    pl, pr = Params(read_side=READ_LEFT, **kw), Params(read_side=READ_RIGHT, **kw)
    with host.Context(0, stream=stream.cuda_stream) as ctx:
        ctx.upload_genome(host.pack_genome(strs))
        ctx.configure(1 << 22, 1 << 20)
        runs = [(pl, cbatch_from_tensors(w["left"], 0)), (pr, cbatch_from_tensors(w["right"], PAIRS))]
        ctx.reset()
        for p, cb in runs:
            ctx.run(p, cb)
        ev = ctx.download(ctx.finish())
        fus = ctx.fusions(runs)
        fkeys = {(int(x["ref_id1"]), int(x["ref_id2"]), int(x["left"]), int(x["right"]), int(x["dir"])) for x in fus}
        assert len(fkeys) > 0.8 * len(fz)
        assert any(k[0] != k[1] for k in fkeys) and {k[4] for k in fkeys} >= {7, 8}
        assert any(k[0] == k[1] == 1 and k[2] < copies * S and k[3] < copies * S and abs(k[3] - k[2]) > S // 2 for k in fkeys)   # between copies
        assert ctx.fusions(runs).tolist() == fus.tolist()                                     # idempotence
        og = orc.Genome(strs)
        m = 30_000
        fs = orc.fusions(pl, og, sample_segbatch(w["left"], m), pl.fusion_anchor_length, pl.fusion_min_dist)
        assert {(int(x["ref_id1"]), int(x["ref_id2"]), int(x["left"]), int(x["right"]), int(x["dir"])) for x in fs} <= fkeys

        # ---- stage 2
        ctx.span_sets_from_segjuncs()
        fl = fusion_list_from_events(fus)
        ctx.upload_span_fusions(fl)
        p2 = Params(fusion_search=1, fusion_min_dist=100000)
        sp = span_cbatch_from_tensors(w["left"], ctx)
        a, passes = span_pass(ctx, p2, sp)
        ops, lens = a["cigar"] >> 28, a["cigar"] & 0x0FFFFFFF
        nfo = np.isin(ops, (7, 8, 9, 10)).sum(1)
        assert set(np.unique(nfo).tolist()) <= {0, 1}
        fa = a[nfo == 1]
        joined = set(np.unique(fa["read_idx"]).tolist())
        assert len(joined & set(fz.tolist())) > 0.8 * len(fz)
        assert joined <= set(fz.tolist()) | set(multi.tolist())
        assert len(joined & set(multi.tolist())) > 300                      # family reads joined across copies
        assert ((fa["cigar"][:, 15] >= 1) & (fa["cigar"][:, 15] <= len(strs))).all()
        lens_r = np.where(np.arange(16)[None, :] < a["n_cigar"][:, None], lens, 0)
        assert ((lens_r * np.isin(ops, (1, 2, 3, 4, 13))).sum(1) == RL).all()
        key = a["read_idx"].astype(np.int64) * 65536 + a["order"]
        assert (np.diff(key) > 0).all()
        # sample parity against the oracle with the full sets
        juncs, ins = events_to_span_inputs(ev)
        want = orc.spanning_fusion(p2, og, sample_spanbatch(w["left"], m), juncs, ins, fl, True)
        assert sum(1 for x in want if x.is_fusion()) > 0.8 * int((fz < m).sum())
        resolver = host.span_md_resolver(strs, [sample_spanbatch(w["left"], m)])
        assert host.alns_from_array(a[a["read_idx"] < m], resolver) == want
        # idempotence (the workspace is now large enough: one pass)
        b, passes2 = span_pass(ctx, p2, sp)
        assert b.tobytes() == a.tobytes() and passes2 == 1
        # shard merge
        hs = [half(w["left"], k) for k in (0, 1)]
        parts = []
        for k in (0, 1):
            parts.append(span_pass(ctx, p2, span_cbatch_from_tensors(hs[k], ctx))[0])
        parts[1]["read_idx"] += hs[0]["n_reads"]
        assert np.concatenate(parts).tobytes() == a.tobytes()
        # fusion search off: the other reads' records are the same
        a0, _ = span_pass(ctx, Params(), sp)
        other = np.concatenate([fz, multi])
        keep, keep0 = ~np.isin(a["read_idx"], other), ~np.isin(a0["read_idx"], other)
        assert keep.sum() > 0.3 * PAIRS
        assert a[keep].tobytes() == a0[keep0].tobytes()
        print("passes", passes, "records", len(a), "fusion alignments", len(fa), "family reads joined", len(joined & set(multi.tolist())))
