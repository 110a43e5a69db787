"""CPU fuzz at the wide shapes (wide_fuzz.GRID: up to 16 segments and 512 bases, both sides of every plane-word boundary): the kernel
logic (tests/hostsim) against the plain-C oracle in both stages -- segment_juncs' events and fusions, long_spanning_reads' tiers in every
mode and its fusion tier with fusion search off and on.  test_gpu_fuzz_wide.py runs the same batches on the device."""
import os

import pytest

import orc
import sim
from util import assert_events_equal
from wide_fuzz import GRID, quadrant, seg_case, shape_id, span_case

# THJ_FUZZ_SEEDS=<n> widens the sweep; every shape of GRID runs at least once
N_CASES = max(len(GRID), int(os.environ.get("THJ_FUZZ_SEEDS", str(len(GRID)))))
CASES = [(k, GRID[k % len(GRID)]) for k in range(N_CASES)]


def case_id(c):
    return "%d-%s" % (c[0], shape_id(c[1]))


def test_grid_covers_every_instance_and_word_boundary():
    assert {quadrant(rl, L) for rl, L in GRID} == {(False, False), (False, True), (True, False), (True, True)}
    assert {256, 257, 320, 321, 384, 385, 448, 449, 511, 512} <= {rl for rl, _ in GRID}
    Ls = {L for _, L in GRID}
    assert {8, 13, 16, 18, 64} <= Ls and min(Ls) == 8
    for rl, L in GRID:
        n = rl // L
        assert 1 <= n <= 16 and 8 <= L <= 64 and rl <= 512 and L <= rl - (n - 1) * L < 2 * L
    assert any(rl // L == 16 and L == 8 for rl, L in GRID) and (512, 32) in GRID and (250, 25) in GRID
    assert any(rl // L == 7 and L == 64 and rl > 448 for rl, L in GRID)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_fuzz_wide_segment_juncs(case):
    seed, shape = case
    seqs, b, p = seg_case(seed, shape, 200)
    g = orc.Genome(seqs)
    want = orc.segjuncs(p, g, b)
    got = sim.segjuncs(p, seqs, b)
    assert_events_equal(got, want, "case %s" % case_id(case))
    for k in ("windows", "indel_pairs", "rescue_pairs"):
        assert got.stats[k] == want.stats[k], k
    assert want.stats["windows"] > 0
    wf = orc.fusions(p, g, b, p.fusion_anchor_length, p.fusion_min_dist)
    assert sim.fusions(p, seqs, b).tolist() == wf.tolist()


def test_fuzz_wide_segment_juncs_does_something():
    """over the default cases: indel pairs, rescue pairs (paired seeds), junctions and fusions all occur"""
    tot = dict(indel_pairs=0, rescue_pairs=0, juncs=0, fusions=0)
    for seed, shape in CASES[:len(GRID)]:
        seqs, b, p = seg_case(seed, shape, 40)
        g = orc.Genome(seqs)
        ev = orc.segjuncs(p, g, b)
        tot["indel_pairs"] += ev.stats["indel_pairs"]
        tot["rescue_pairs"] += ev.stats["rescue_pairs"]
        tot["juncs"] += len(ev.juncs)
        tot["fusions"] += len(orc.fusions(p, g, b, p.fusion_anchor_length, p.fusion_min_dist))
    assert all(v > 0 for v in tot.values()), tot


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_fuzz_wide_spanning(case):
    seed, shape = case
    seqs, sb, p, ja, il, _ = span_case(seed, shape, 80)
    g = orc.Genome(seqs)
    want = orc.spanning(p, g, sb, ja, il)
    assert len({a.read_idx for a in want}) >= 3
    for mode in (0, 1, 2, 3):
        got, status = sim.spanning(p, seqs, sb, ja, il, mode)
        assert status[1] == 0
        got.sort(key=lambda a: a.read_idx)
        assert got == want, "case %s mode %d" % (case_id(case), mode)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_fuzz_wide_fusion_tier(case):
    seed, shape = case
    seqs, sb, p, ja, il, fus = span_case(seed, shape, 80)
    g = orc.Genome(seqs)
    for fs in (0, 1):
        p.fusion_search = fs
        want = orc.spanning_fusion(p, g, sb, ja, il, fus, bool(fs))
        assert len({a.read_idx for a in want}) >= 3
        if fs and seed < len(GRID):                 # (every default case has fusion alignments; a few of a wide sweep's have none)
            assert any(a.is_fusion() for a in want)
        elif not fs:
            assert want == orc.spanning(p, g, sb, ja, il)
        for skip0 in (False, True):
            got, status = sim.spanning_fusion(p, seqs, sb, ja, il, fus, skip0)
            assert status[1] == 0
            got.sort(key=lambda a: a.read_idx)
            assert got == want, "case %s fusion_search %d skip_tier0 %s" % (case_id(case), fs, skip0)


def test_more_than_16_cigar_ops_yield_no_alignment_cpu():
    """a joined alignment of more than 16 CIGAR ops has no record.  Reads of 16 x 16 bases over 17..60-base exons, every intron in
    the junction set: the oracle joins some into 17 ops; the kernel logic gives its records minus exactly those, in every mode and through
    the fusion tier (test_gpu_fuzz_wide runs the device)"""
    import numpy as np
    from wide_fuzz import n_ops, short_exon_case
    from tophat_amd.params import Params
    seqs, sb, ja = short_exon_case()
    g = orc.Genome(seqs)
    p = Params(segment_length=16, min_report_intron=30)
    want = orc.spanning(p, g, sb, ja, [])
    assert sum(1 for a in want if n_ops(a) > 16) >= 10 and sum(1 for a in want if n_ops(a) <= 16) >= 50
    keep = [a for a in want if n_ops(a) <= 16]
    for mode in (0, 1, 2, 3):
        got, status = sim.spanning(p, seqs, sb, ja, [], mode)
        got.sort(key=lambda a: a.read_idx)
        assert got == keep, mode
    nf = np.zeros(0, dtype=orc.SPAN_FUSION_DTYPE)
    for fs in (0, 1):
        p.fusion_search = fs
        assert orc.spanning_fusion(p, g, sb, ja, [], nf, bool(fs)) == want
        for skip0 in (False, True):
            got, _ = sim.spanning_fusion(p, seqs, sb, ja, [], nf, skip0)
            got.sort(key=lambda a: a.read_idx)
            assert got == keep, (fs, skip0)
