"""Test infrastructure: hand-worked cases and a seeded crowd for the choice among a read's alignments (thj_juncbed_best_alignments,
thj_junctions --best-alignments), shared by test_best_cpu.py (restatement and CPU sim) and test_gpu_best.py (the device).  Every case
states what must come out, worked by hand from the reference's text (best_ref.py cites the lines); nothing here calls the product.

A case is a dict: recs (indelbed_ref's records), reads, AS, mism, anti (lists of the records' length), known, limits, anchor, best =
(max_multihits, suppress_hits, bowtie2_max_penalty), and what is expected: want_j (junction rows: ref, left, right, antisense,
left_extent, right_extent, support), want_d (deletion rows: ref, left, right, left_extent, right_extent, support), want_i (the NUMBER
of insertion rows; their letters depend on the seeded SEQs and are compared against the restatement).
The genome is jbknown_cases.GENOME (two contigs of 20000 bases)."""
import numpy as np

from jbknown_cases import GENOME, rec                            # noqa: F401  (rec: M a, N gap, M b -> junction (left + a - 1, left + a + gap), extents a / b)

M, m, I, i_, D, d, FF, FR, RF, RR, N, n_ = 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12
MT_SEED1 = (1791095845, 4282876139, 3093770124, 4005303368, 491263, 550290313)      # the first outputs of mt19937 seeded 1


def plain(left, length, ref=1):
    return (ref, left, False, [(M, length)])


def with_del(left):
    """M20 D2 M20: the deletion (left + 19, left + 22), extents 20 / 20"""
    return (1, left, False, [(M, 20), (D, 2), (M, 20)])


def del_row(left):
    return (1, left + 19, left + 22, 20, 20, 1)


def case(label, reads_of, want_j=(), want_d=(), want_i=0, known=(), limits=None, anchor=8, best=(20, False, 6)):
    """reads_of = [[(record, AS[, mism[, antisense_align]]) ...] per read]"""
    recs, reads, AS, mism, anti = [], [], [], [], []
    for k, rd in enumerate(reads_of):
        for t in rd:
            recs.append(t[0]); reads.append(k); AS.append(t[1]); mism.append(t[2] if len(t) > 2 else 0); anti.append(bool(t[3]) if len(t) > 3 else False)
    return dict(label=label, recs=recs, reads=reads, AS=AS, mism=mism, anti=anti, known=list(known), limits=limits, anchor=anchor, best=best,
                want_j=list(want_j), want_d=list(want_d), want_i=want_i)


def contested(n_support, spliced, unspliced_as, spliced_as=0):
    """n_support reads of the spliced record alone, then one read with that record (AS spliced_as) and an unspliced one of its length"""
    rl = sum(ln for op, ln in spliced[3] if op == M)
    return [[(spliced, 0)] for _ in range(n_support)] + [[(spliced, spliced_as), (plain(spliced[1], rl), unspliced_as)]]


def cases():
    out = []
    J = (1, 119, 620, 0)
    S40 = rec(100, 20, 500, 20)                                  # read_len 40: min_extent 10
    # first-pass support 5, extents 20 / 20: penalty (int)(8 * 0) = 0, the spliced record (0) beats the unspliced one (-6)
    out.append(case("support5_long_extents", contested(4, S40, -6), want_j=[J + (20, 20, 5)]))
    # support 4: penalty 8, -8 < -6: the unspliced record is reported and the junction loses this read
    out.append(case("support4", contested(3, S40, -6), want_j=[J + (20, 20, 3)]))
    # support 5 and a first-pass right extent of 9 = min_extent - 1: penalty (int)(8 * 0.5f) = 4
    S9 = rec(100, 31, 500, 9)                                    # junction (130, 631), extents 31 / 9, read_len 40
    K = (1, 130, 631, 0)
    out.append(case("short_extent_mp6_loses_to_minus3", contested(4, S9, -3), want_j=[K + (31, 9, 4)]))
    out.append(case("short_extent_mp6_ties_minus4", contested(4, S9, -4), want_j=[K + (31, 9, 5)]))
    # --bowtie2-max-penalty 5: (int)(7 * 0.5f) = 3, the reference's truncation
    out.append(case("short_extent_mp5_ties_minus3", contested(4, S9, -3), want_j=[K + (31, 9, 5)], best=(20, False, 5)))
    out.append(case("short_extent_mp5_loses_to_minus2", contested(4, S9, -2), want_j=[K + (31, 9, 4)], best=(20, False, 5)))
    # read_len 36: min_extent 9 -- an extent of 9 is long enough, one of 8 is not
    out.append(case("len36_extent9_no_penalty", contested(4, rec(100, 27, 500, 9), -3), want_j=[(1, 126, 627, 0, 27, 9, 5)]))
    out.append(case("len36_extent8_penalty4", contested(4, rec(100, 28, 500, 8), -3), want_j=[(1, 127, 628, 0, 28, 8, 4)]))
    # read_len 100: min_extent 10
    out.append(case("len100_extent10_no_penalty", contested(4, rec(100, 90, 500, 10), -3), want_j=[(1, 189, 690, 0, 90, 10, 5)]))
    out.append(case("len100_extent9_penalty4", contested(4, rec(100, 91, 500, 9), -3), want_j=[(1, 190, 691, 0, 91, 9, 4)]))
    # an annotated junction: + 2 beats the unspliced record of equal AS; without the annotation support 2 costs 8
    out.append(case("annotated_plus2", contested(1, S40, 0), want_j=[J + (20, 20, 2)], known=[J]))
    out.append(case("not_annotated_minus8", contested(1, S40, 0), want_j=[J + (20, 20, 1)]))
    # two junctions in one record (support 3 each): the penalties add, 0 - 8 - 8 = -16
    TWO = (1, 100, False, [(M, 20), (N, 300), (M, 30), (N, 400), (M, 20)])
    J1, J2 = (1, 119, 420, 0), (1, 449, 850, 0)
    out.append(case("two_junctions_minus16_loses_to_minus15", contested(2, TWO, -15), want_j=[J1 + (20, 30, 2), J2 + (30, 20, 2)]))
    out.append(case("two_junctions_minus16_beats_minus17", contested(2, TWO, -17), want_j=[J1 + (20, 30, 3), J2 + (30, 20, 3)]))
    # pass-1 duplicates: X and Y are equal under cmp_read_equal (left, right, sizes, mismatches 0, edit_dist 1) with different cigars on
    # one junction; they count ONCE in the first pass, so the junction has support 2 + 1 + 1 = 4, not 5, the contested read's spliced
    # record costs 8 and its unspliced one (-6) is reported.  Second pass of the X / Y read: both -8, tied, unique keeps X.
    X = (1, 100, False, [(M, 20), (N, 500), (M, 8), (I, 1), (M, 11)])
    Y = (1, 100, False, [(M, 20), (N, 500), (M, 9), (I, 1), (M, 10)])
    out.append(case("pass1_duplicates_count_once", [[(S40, 0)], [(S40, 0)], [(X, 0), (Y, 0)], [(S40, 0), (plain(100, 40), -6)]], want_j=[J + (20, 20, 3)], want_i=1))
    # equal keys, different AS: pass 1 keeps the first in order, X (right extent 8: still accepted at --min-anchor 8); pass 2 scores the
    # raw list, Y (0 - 8) beats X (-5 - 8) and is the one reported -- right extent 9
    out.append(case("equal_keys_different_AS", [[(X, -5), (Y, 0)]], want_j=[J + (20, 9, 1)], want_i=1))
    # rights A, B, A under otherwise equal fields (one gap base each, three ops); in operator< order A1 < B < A2 (first op 18 < 19 < 20), so
    # the first pass keeps all three.  B scores lower; A1 and A2 are then neighbours and the second unique removes A2: one deletion row
    A1 = (1, 3000, False, [(M, 18), (D, 1), (M, 22)])
    B = (1, 3000, False, [(M, 19), (I, 1), (M, 20)])
    A2 = (1, 3000, False, [(M, 20), (D, 1), (M, 20)])
    out.append(case("rights_A_B_A", [[(A2, -5), (B, -10), (A1, -5)]], want_d=[(1, 3017, 3019, 18, 22, 1)]))
    # the best-scoring record lies on a rejected junction (right anchor 5 < 8): excluded first, the next one (-6) is reported, not the third
    out.append(case("excluded_before_the_score", [[(rec(100, 20, 500, 5), 0), (with_del(3000), -6), (with_del(3100), -9)]], want_d=[del_row(3000)]))
    # a fusion alignment with a REF_SKIP behind its fusion op: the walkers put the junction on the second contig, (2, 5009, 5310), where
    # five other reads support it; AlignStatus asks for (1, 5009, 5310), finds nothing and takes off 6: -6 < -3, the unspliced record wins
    FUS = (1, 100, False, [(M, 20), (FF, 5000), (M, 10), (N, 300), (M, 20)], 2)
    out.append(case("fusion_junction_under_the_first_contig", [[(rec(4990, 20, 300, 20, ref=2), 0)] for _ in range(5)] + [[(FUS, 0), (plain(100, 50), -3)]],
                    want_j=[(2, 5009, 5310, 0, 20, 20, 5)]))
    # the cap.  Two reads that report something (one draw each), one that reports nothing (its only record lies on a rejected junction),
    # then a read of five tied records: its first draw is the generator's third output.
    #   max_multihits 2: 3093770124 % 5 = 4 -> [0 1 2 3]; 4005303368 % 4 = 0 -> [1 2 3]; 491263 % 3 = 1 -> [1 3]
    #   max_multihits 1: then 550290313 % 2 = 1 -> [1]
    tied = [(with_del(4000 + 100 * k), 0) for k in range(5)]
    lead = [[(with_del(3000), 0)], [(with_del(3100), 0)], [(rec(100, 20, 500, 5), 0)]]
    out.append(case("cap_2_of_5", lead + [tied], want_d=[del_row(3000), del_row(3100), del_row(4100), del_row(4300)], best=(2, False, 6)))
    out.append(case("cap_1_of_5", lead + [tied], want_d=[del_row(3000), del_row(3100), del_row(4100)], best=(1, False, 6)))
    out.append(case("cap_suppressed", lead + [tied], want_d=[del_row(3000), del_row(3100)], best=(2, True, 6)))
    out.append(case("cap_not_reached", lead + [tied], want_d=[del_row(3000), del_row(3100)] + [del_row(4000 + 100 * k) for k in range(5)], best=(5, False, 6)))
    return out


def crowd(seed=11, n_reads=3000, max_multihits=3):
    """a seeded crowd on about 60 junction sites whose support straddles 5: plain reads of one or two records, pairs that are equal
    under cmp_read_equal with different cigars, spliced against unspliced records, rights A B A, a best record on a junction whose
    anchor is too short, and reads of up to seven tied records -> a case dict without expectations (best = (max_multihits, False, 6))"""
    rng = np.random.default_rng(seed)
    sites = [(int(rng.integers(1, 3)), 300 + 300 * k + int(rng.integers(0, 20)), int(rng.integers(60, 120)), bool(rng.integers(0, 2))) for k in range(60)]
    weight = rng.integers(1, 12, len(sites)).astype(float)
    weight /= weight.sum()
    reads_of = []

    def spliced():
        ref, at, gap, anti = sites[int(rng.choice(len(sites), p=weight))]
        a, b = int(rng.integers(9, 30)), int(rng.integers(8, 30))
        return (ref, at - a, anti, [(M, a), (N, gap), (M, b)])

    for _ in range(n_reads):
        kind = int(rng.integers(0, 10))
        if kind <= 2:
            reads_of.append([(spliced(), int(-rng.integers(0, 4)))])
        elif kind == 3:
            s = spliced()
            reads_of.append([(s, int(-rng.integers(0, 10))), (plain(s[1], s[3][0][1] + s[3][2][1], s[0]), int(-rng.integers(0, 10)))])
        elif kind == 4:                                          # equal under cmp_read_equal, different cigars
            ref, at, gap, anti = sites[int(rng.choice(len(sites), p=weight))]
            a, b = int(rng.integers(9, 30)), int(rng.integers(8, 14))
            x = (ref, at - a, anti, [(M, a), (N, gap), (M, b), (I, 1), (M, 12)])
            y = (ref, at - a, anti, [(M, a), (N, gap), (M, b + 2), (I, 1), (M, 10)])
            reads_of.append([(y, int(-rng.integers(0, 3))), (x, int(-rng.integers(0, 3)))])
        elif kind == 5:                                          # rights A, B, A
            left, ref = int(rng.integers(200, 19000)), int(rng.integers(1, 3))
            a1, b, a2 = (ref, left, False, [(M, 18), (D, 1), (M, 22)]), (ref, left, False, [(M, 19), (I, 1), (M, 20)]), (ref, left, False, [(M, 20), (D, 1), (M, 20)])
            low = int(-rng.integers(0, 3))
            reads_of.append([(a2, -2), (b, -2 + low), (a1, -2)])
        elif kind == 6:                                          # the best record on a junction of its own whose anchor is too short for --min-anchor
            lone = (int(rng.integers(1, 3)), int(rng.integers(200, 19000)), False, [(M, 25), (N, int(rng.integers(130, 200))), (M, int(rng.integers(3, 8)))])
            reads_of.append([(lone, 0), (with_del(int(rng.integers(200, 19000))), -12), (spliced(), int(-rng.integers(0, 12)))])
        elif kind == 7:                                          # tied records, some reads over the cap
            k = int(rng.integers(2, 8))
            base = int(rng.integers(200, 18000))
            reads_of.append([(with_del(base + 40 * int(j)), 0) for j in rng.permutation(k)])
        elif kind == 8:                                          # a mismatching record beside a clean one, on either strand of the read
            s = spliced()
            reads_of.append([(s, -6, 1, int(rng.integers(0, 2))), (s, 0, 0, int(rng.integers(0, 2)))])
        else:
            reads_of.append([(spliced(), 0), (spliced(), 0)])
    c = case("crowd", reads_of, best=(max_multihits, False, 6))
    return c
