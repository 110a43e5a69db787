"""Test infrastructure: the planted cases of the junction consensus with annotated junctions (--gtf-juncs) and the read filter, shared by
test_jbknown_cpu.py (restatement and CPU sim) and test_gpu_jbknown.py (the device).  Every case states what must come out, worked out
by hand from the reference's rules (jbknown_ref.py cites them); nothing here calls the product.

Records are indelbed_ref's (ref_id, left, antisense_splice, [(op, len) ...]); junction rows (ref, left, right, antisense, left_extent,
right_extent, support); deletion rows (ref, left, right, left_extent, right_extent, support)."""
import numpy as np

M, I, D, N = 1, 3, 5, 11
GENOME = ["ACGT" * 5000, "TTGCA" * 4000]                      # the contigs of every case here (the device tests upload them)


def rec(left, a, gap, b, anti=False, ref=1):
    """M a, N gap, M b: the junction (left + a - 1, left + a + gap) with extents a / b"""
    return (ref, left, anti, [(M, a), (N, gap), (M, b)])


STRONG, WEAK = [rec(100, 20, 500, 20)] * 3, [rec(103, 20, 497, 20, anti=True)]           # junctions (119, 620, +) x 3 and (122, 620, -) x 1
TWO = (1, 100, False, [(M, 20), (N, 300), (M, 30), (N, 400), (M, 5)])                   # junctions (119, 420) 20 / 30 and (449, 850) 30 / 5
WITH_DEL = (1, 100, False, [(M, 20), (D, 2), (M, 10), (N, 500), (M, 6)])                # deletion (119, 122) 20 / 10, junction (131, 632) 10 / 6

# (label, min_anchor, records, annotated junctions, junction rows, deletion rows)
KNOWN_CASES = [
    ("short_anchor_unknown", 12, [rec(100, 20, 500, 9)], [], [], []),
    ("short_anchor_known", 12, [rec(100, 20, 500, 9)], [(1, 119, 620, 0)], [(1, 119, 620, 0, 20, 9, 1)], []),
    ("known_but_under_the_final_filter", 12, [rec(100, 20, 500, 7)], [(1, 119, 620, 0)], [], []),
    ("long_intron_once_known", 8, [rec(100, 20, 60000, 20)], [(1, 119, 60120, 0)], [(1, 119, 60120, 0, 20, 20, 1)], []),
    ("long_intron_anchor_12_twice_known", 8, [rec(100, 20, 60000, 12)] * 2, [(1, 119, 60120, 0)], [(1, 119, 60120, 0, 20, 12, 2)], []),
    ("shadow_no_annotation", 8, STRONG + WEAK, [], [(1, 119, 620, 0, 20, 20, 3)], []),
    ("shadow_stronger_known", 8, STRONG + WEAK, [(1, 119, 620, 0)], [(1, 119, 620, 0, 20, 20, 3)], []),
    ("shadow_weaker_known", 8, STRONG + WEAK, [(1, 122, 620, 1)], [(1, 119, 620, 0, 20, 20, 3), (1, 122, 620, 1, 20, 20, 1)], []),
    ("two_junctions_unknown", 8, [TWO], [], [], []),
    ("two_junctions_second_known", 8, [TWO], [(1, 449, 850, 0)], [(1, 119, 420, 0, 20, 30, 1)], []),
    ("deletion_without_annotation", 8, [WITH_DEL], [], [], []),
    ("deletion_with_annotation", 8, [WITH_DEL], [(1, 131, 632, 0)], [], [(1, 119, 122, 20, 10, 1)]),
    ("known_nobody_shows", 8, [rec(100, 20, 500, 20)], [(1, 5000, 6000, 0)], [(1, 119, 620, 0, 20, 20, 1)], []),
    ("known_on_the_other_strand", 12, [rec(100, 20, 500, 9)], [(1, 119, 620, 1)], [], []),
]

# the read filter, decided from (NM, cigar).  (label, record, NM or None, [(limits, (mismatches, gap_length, edit_dist), dropped)])
SPL = [(N, 500), (M, 20)]
FILTER_CASES = [
    ("nm3_no_indel", (1, 100, False, [(M, 20)] + SPL), 3, [((2, 2, 2), (3, 0, 3), True), ((3, 2, 3), (3, 0, 3), False)]),
    ("nm3_with_1I", (1, 100, False, [(M, 20), (I, 1), (M, 10)] + SPL), 3, [((2, 2, 2), (2, 1, 3), True), ((2, 2, 3), (2, 1, 3), False)]),
    ("deletion_of_3", (1, 100, False, [(M, 20), (D, 3), (M, 10)] + SPL), 3, [((2, 2, 9), (0, 3, 3), True), ((2, 3, 9), (0, 3, 3), False)]),
    ("2D_without_NM", (1, 100, False, [(M, 20), (D, 2), (M, 10)] + SPL), None, [((2, 9, 9), (254, 2, 0), True), ((2, 2, 2), (254, 2, 0), True)]),
]


def crowd(seed=3, n=3000):
    """near-coincident junctions on both strands of two contigs (the crowd of test_gpu_juncbed.test_filters_on_the_device)"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        l0 = int(rng.integers(50, 400))
        out.append(rec(l0, int(rng.integers(5, 40)), int(rng.integers(60, 90)), int(rng.integers(5, 40)), anti=bool(rng.integers(0, 2)), ref=int(rng.integers(1, 3))))
    return out


def crowd_known(recs, seed=17, frac=0.3):
    """a seeded 30 % of the crowd's distinct junctions"""
    import indelbed_ref as ir
    distinct = sorted({j[:4] for r in recs for j in ir.rec_juncs(r)})
    rng = np.random.default_rng(seed)
    pick = rng.permutation(len(distinct))[:int(len(distinct) * frac)]
    return [distinct[k] for k in sorted(pick.tolist())]
