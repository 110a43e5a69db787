"""CPU: the spanning records' AS and MD with base qualities that vary (phred 2..41), against the oracle.  The record builders note
the quality offsets of a record's first mismatches and load them together at the end; past that many mismatches they load them
one by one.  Both ways, and every tier's walk, must give the oracle's AS, XM, XO, XG, NM and MD."""
import dataclasses

import numpy as np
import pytest

import orc
import sim
from tophat_amd.batch import JUNC_DTYPE
from tophat_amd.params import Params
from test_hostsim_spanning import repeat_span_batch, span_inputs

QCAP = 6        # thj_span_core.h: qualities noted per record before the one-by-one loads

QUAL_CASES = [
    # W = 1, 2, 3 (150 bases: the read's planes come from memory in tier 0); high error rates: records with more than QCAP mismatches
    dict(seed=31, read_len=50, seg_len=25, extra=dict(read_mismatches=12, read_edit_dist=12, read_gap_length=3),
         gen=dict(boundary_bias=0.6, err=0.12, n_frac=0.3, indel_frac=0.3)),
    dict(seed=32, read_len=100, seg_len=25, extra=dict(read_mismatches=16, read_edit_dist=16, read_gap_length=3),
         gen=dict(boundary_bias=0.6, spliced_seg_frac=0.5, err=0.08, n_frac=0.3, indel_frac=0.4)),
    dict(seed=33, read_len=150, seg_len=25, extra=dict(read_mismatches=20, read_edit_dist=20, read_gap_length=3),
         gen=dict(boundary_bias=0.5, spliced_seg_frac=0.7, err=0.07, n_frac=0.3, indel_frac=0.4, repeat_frac=0.3)),
    # the default error rate: few mismatches a record, all through the grouped loads
    dict(seed=34, read_len=100, seg_len=25, extra={}, gen=dict(boundary_bias=0.6, spliced_seg_frac=0.5, n_frac=0.2, indel_frac=0.3)),
]


def random_quals(sb, seed):
    rng = np.random.default_rng(seed)
    q = rng.integers(33 + 2, 33 + 42, size=sb.quals.shape[0], dtype=np.uint8)
    return dataclasses.replace(sb, quals=q)


def qual_inputs(cfg, n_reads):
    case, p, seqs, g, sb, juncs, ins = span_inputs(cfg, n_reads)
    return case, p, seqs, g, random_quals(sb, cfg["seed"]), juncs, ins


def check_shape(cfg, want):
    assert len(want) > 50
    assert any(a.antisense for a in want) and any(not a.antisense for a in want)
    assert len({a.AS for a in want}) > 10                       # the qualities matter
    if cfg["read_len"] >= 100:
        if cfg["extra"]:
            assert sum(1 for a in want if a.XM > QCAP) > 5, max(a.XM for a in want)
        assert any("^" in a.MD for a in want if a.MD)           # deletions in the MD string


@pytest.mark.parametrize("cfg", QUAL_CASES, ids=lambda c: "seed%d_rl%d" % (c["seed"], c["read_len"]))
def test_records_with_random_quals_match_oracle(cfg):
    case, p, seqs, g, sb, juncs, ins = qual_inputs(cfg, 1500)
    want = orc.spanning(p, g, sb, juncs, ins)
    check_shape(cfg, want)
    for mode in (0, 1, 2, 3):       # chain entries -> join -> finish; the generic path alone; no packed tier / no chains; tiny packed limits
        got, status = sim.spanning(p, seqs, sb, juncs, ins, mode)
        assert status[1] == 0 and status[2] == 0
        got.sort(key=lambda a: a.read_idx)
        assert got == want, "mode %d" % mode


def mutated_repeat_batch(copies, n_reads, seed):
    """repeat_span_batch (every segment hits every copy: the packed multihit tier) with random qualities and a few bases of
    each copy changed, so that the copies' records differ in mismatches and AS"""
    seq, sb = repeat_span_batch(copies=copies, n_reads=n_reads, seed=seed)
    rng = np.random.default_rng(seed)
    s = list(seq)
    for c in range(copies):
        for k in rng.choice(400, size=int(rng.integers(0, 9)), replace=False):
            i = 3000 + c * 400 + int(k)
            s[i] = "N" if rng.random() < 0.1 else "ACGT"[("ACGT".index(s[i]) + 1) % 4]
    seq = "".join(s)
    # the segment hits' mismatch counts as the mutated genome gives them
    hits = sb.hits.copy()
    for r in range(sb.n_reads):
        read = bytes(sb.bases[sb.read_off[r]:sb.read_off[r + 1]]).decode()
        for sgi in range(sb.nseg):
            for h in hits[sb.seg_off[r * sb.nseg + sgi]:sb.seg_off[r * sb.nseg + sgi + 1]]:
                ln = int(h["cigar"][0]) & 0xFFFFFFF
                ref = seq[int(h["left"]):int(h["left"]) + ln]
                part = read[25 * sgi:25 * sgi + ln]
                mm = sum(1 for a, b in zip(ref, part) if a != b)
                h["mismatches"] = mm
                h["edit_dist"] = mm
    return seq, random_quals(dataclasses.replace(sb, hits=hits), seed)


def test_packed_tier_with_random_quals():
    nj = np.zeros(0, dtype=JUNC_DTYPE)
    seq, sb = mutated_repeat_batch(copies=12, n_reads=30, seed=41)
    p = Params(read_mismatches=8, read_edit_dist=8)
    want = orc.spanning(p, orc.Genome([seq]), sb, nj, [])
    assert len(want) > 100 and len({a.AS for a in want}) > 5
    for mode in (0, 3):
        got, status = sim.spanning(p, [seq], sb, nj, [], mode)
        assert status[1] == 0
        got.sort(key=lambda a: a.read_idx)
        assert got == want, mode
