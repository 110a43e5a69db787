"""Test infrastructure: hand-worked cases and a seeded crowd for the choice among an insert's alignments (thj_juncbed_pair_alignments),
shared by test_pair_cpu.py (restatement and CPU sim) and test_gpu_pair.py (the device).  Every case states the junction rows that must
come out, worked by hand from the reference's text (pair_ref.py cites the lines); nothing here calls the product.

A case is a dict: L, R (the two sides in best_cases' form; reads = the insert's number), known, limits, anchor, best = (max_multihits,
suppress_hits, bowtie2_max_penalty), pair = (inner_dist_mean, inner_dist_std_dev, fusion_min_dist, report_mixed, report_discordant) and
want_j (junction rows: ref, left, right, antisense, left_extent, right_extent, support), want_d (deletion rows: ref, left, right, left_extent,
right_extent, support), want_i (the NUMBER of insertion rows; their letters depend on the SEQs) and, where a case states its SEQs (seqs),
want_ins (insertion rows: ref, left, letters, left_extent, right_extent, support).  The genome is jbknown_cases.GENOME.

The usual insert here: the left read is L0 = 40 unspliced bases at 1000 (it ends at 1040), forward; the right read's records are spliced,
reverse, `inner` bases behind it -- M20 N<gap> M20, the junction (1059 + inner, 1060 + inner + gap) -- so the junction rows say which right
record was reported.  With the defaults (mean 200, sd 20, penalty 6) a junction of first-pass support below 5 costs its record 8."""
import numpy as np

from best_cases import FF, I, M, N, plain                      # noqa: F401
from jbknown_cases import GENOME, rec                           # noqa: F401

PAIR = (200, 20, 10000000, False, False)
L0 = plain(1000, 40)


def right_at(inner, gap=100):
    return rec(1040 + inner, 20, gap, 20)


def jrow(inner, gap=100, support=1):
    return (1, 1059 + inner, 1060 + inner + gap, 0, 20, 20, support)


def side(reads_of, anti_default):
    """reads_of = [(insert number, [(record, AS[, mism[, antisense_align]]) ...])]"""
    out = dict(recs=[], reads=[], AS=[], mism=[], anti=[])
    for num, rd in reads_of:
        for t in rd:
            out["recs"].append(t[0]); out["reads"].append(num); out["AS"].append(t[1]); out["mism"].append(t[2] if len(t) > 2 else 0)
            out["anti"].append(bool(t[3]) if len(t) > 3 else anti_default)
    return out


def pcase(label, inserts, want_j=(), known=(), limits=None, anchor=8, best=(20, False, 6), pair=PAIR, want_d=(), want_i=0, seqs=None, want_ins=None):
    """inserts = [(left records, right records)] numbered from 0; an empty side: a singleton.  Left records are forward and right
    records reverse unless a record says otherwise."""
    L = side([(k, l) for k, (l, r) in enumerate(inserts) if l], False)
    R = side([(k, r) for k, (l, r) in enumerate(inserts) if r], True)
    return dict(label=label, L=L, R=R, known=list(known), limits=limits, anchor=anchor, best=best, pair=pair, want_j=list(want_j), want_d=list(want_d), want_i=want_i, seqs=seqs,
                want_ins=want_ins)


def seqs_of(c, seed=1):
    """SEQ of every record: the case's own where it states them, seeded ones otherwise"""
    import indelbed_cases as ic
    return c["seqs"] if c.get("seqs") else {"L": ic.make_seqs(c["L"]["recs"], seed), "R": ic.make_seqs(c["R"]["recs"], seed + 1)}


def two_rights(label, a, b, want, **kw):
    """one insert: L0 against two right records (inner, AS)"""
    return pcase(label, [([(L0, 0)], [(right_at(a[0]), a[1]), (right_at(b[0]), b[1])])], want_j=[jrow(x) for x in want], **kw)


def rescue(label, jl, jr, n_support, far_wins, a=20):
    """n_support left-only singletons show the junction (jl, jr) with a left anchor of `a` bases: they count in the first pass and, mixed
    alignments not being reported, contribute nothing to the second.  Then L0 against a near record (inner 200, AS -5: -5 - 8 = -13) and a far
    one (inner 700: inner1 = 1040, inner2 = 1740; AS 0: 0 - 8 = -8 when rescued, - 6 more = -14 when not)."""
    s = rec(jl - a + 1, a, jr - jl - 1, 20)
    return pcase(label, [([(s, 0)], [])] * n_support + [([(L0, 0)], [(right_at(200), -5), (right_at(700), 0)])], want_j=[jrow(700 if far_wins else 200)])


X = (1, 1240, False, [(M, 20), (N, 500), (M, 8), (I, 1), (M, 11)])       # X and Y are equal under cmp_read_equal (best_cases): junction (1259, 1760),
Y = (1, 1240, False, [(M, 20), (N, 500), (M, 9), (I, 1), (M, 10)])       # right extent 8 from X, 9 from Y; both 200 behind L0
JX = (1, 1259, 1760, 0, 20, 8, 1)
S = rec(1000, 20, 100, 20)                                       # a spliced LEFT record: it ends at 1140; junction (1019, 1120)
JS = (1, 1019, 1120, 0)
MATE = plain(1340, 40)                                           # 200 behind S
ALT = plain(1100, 40)                                            # an unspliced left record that ends at 1140 too


def cases():
    out = []
    # ---- the score's boundaries.  Both right records cost 8; the left record scores 0.
    # too_far is inner > 220.  220: no penalty (-8); 221: inner - 220 = 1 < sd, half the penalty (-11)
    out.append(two_rights("too_far_at_mean_plus_sd_no_penalty", (220, 0), (221, 0), [220]))
    out.append(two_rights("too_far_by_one_costs_3", (220, -3), (221, 0), [220, 221]))                  # -11 = -11
    # inner - 220 = 19 = sd - 1: half (6 / 2 = 3); = 20 = sd: the whole 6
    out.append(two_rights("too_far_sd_minus_1_half", (239, 0), (240, 0), [239]))                       # -11 > -14
    out.append(two_rights("too_far_sd_full", (239, -3), (240, 0), [239, 240]))                         # -14 = -14
    # too_close is inner < 180: min(3, (180 - inner) / 20 + 1).  141: 39 / 20 + 1 = 2; 140: 40 / 20 + 1 = 3 = max_penalty / 2
    out.append(two_rights("too_close_one_below_the_cap", (141, 0), (140, 0), [141]))                   # -10 > -11
    out.append(two_rights("too_close_at_the_cap", (141, -1), (140, 0), [140, 141]))                    # -11 = -11
    # max_penalty 5 (a junction then costs 7): the halves are 2.  239: -3 - 7 - 2 = -12; 240: 0 - 7 - 5 = -12
    out.append(two_rights("odd_penalty_half_is_2", (239, -3), (240, 0), [239, 240], best=(20, False, 5)))
    # ... and too_close is capped at 2: 179: -1 - 7 - (1 / 20 + 1 = 1) = -9; 100: 0 - 7 - min(2, 80 / 20 + 1 = 5) = -9
    out.append(two_rights("odd_penalty_too_close_cap_2", (179, -1), (100, 0), [100, 179], best=(20, False, 5)))
    # containment: the right record [1100, 1240) lies inside the left one [1000, 1300): inner distance 0, not 1100 - 1300 = -200.
    # max_penalty 40 (a junction costs 42, the cap is 20): 0 - 42 - (180 / 20 + 1 = 10) = -52; the other record, 200 behind 1300: -10 - 42 = -52.
    # (-200 would cost min(20, 380 / 20 + 1) = 20.)
    out.append(pcase("containment_inner_0", [([(plain(1000, 300), 0)], [(rec(1100, 20, 100, 20), 0), (rec(1500, 20, 100, 20), -10)])],
                     want_j=[(1, 1119, 1220, 0, 20, 20, 1), (1, 1519, 1620, 0, 20, 20, 1)], best=(20, False, 40)))
    # ---- the rescue (temp_dist = jl - 1040 + 1740 - jr must lie in [180, 220])
    out.append(rescue("rescue_support_10", 1100, 1600, 10, True))                                      # 60 + 140 = 200
    out.append(rescue("rescue_support_9", 1100, 1600, 9, False))
    out.append(rescue("rescue_left_at_inner1", 1040, 1540, 10, True))                                  # 0 + 200
    out.append(rescue("rescue_left_before_inner1", 1039, 1539, 10, False))
    out.append(rescue("rescue_right_at_inner2", 1240, 1740, 10, True))                                 # 200 + 0
    out.append(rescue("rescue_dist_180", 1100, 1620, 10, True))
    out.append(rescue("rescue_dist_179", 1100, 1621, 10, False))
    out.append(rescue("rescue_dist_220", 1100, 1580, 10, True))
    out.append(rescue("rescue_dist_221", 1100, 1579, 10, False))
    out.append(rescue("rescue_by_a_rejected_junction", 1100, 1600, 10, True, a=5))                     # left anchor 5 < 8: filter_junctions rejects it, the set keeps it
    # ---- fusion pairs.  OK (inner 200, AS -10: -18) first, then a record BAD (AS 0, gap 150) whose pair is a fusion pair: 0 - 8 - 6 = -14.
    # Without discordant pairs the first pass skips BAD's pair, BAD's junction is in no first-pass set and the second pass excludes BAD:
    # OK is reported.  With them BAD's pair raises the best and empties the list: BAD is reported.  (Were the pair no fusion pair it would
    # score at least -14 and win in both settings.)
    ok = (right_at(200), -10)
    disc = (200, 20, 10000000, False, True)
    reasons = {
        "other_contig": ((rec(1240, 20, 150, 20, ref=2), 0), (2, 1259, 1410, 0, 20, 20, 1), PAIR, disc),
        "equal_strands": ((right_at(200, 150), 0, 0, False), jrow(200, 150), PAIR, disc),
        "left_distance_negative": ((rec(500, 20, 150, 20), 0), (1, 519, 670, 0, 20, 20, 1), PAIR, disc),
        "beyond_fusion_min_dist": ((rec(9000, 20, 150, 20), 0), (1, 9019, 9170, 0, 20, 20, 1), (200, 20, 5000, False, False), (200, 20, 5000, False, True)),
    }
    for name, (bad, row, off, on) in reasons.items():
        out.append(pcase("fusion_" + name + "_skipped", [([(L0, 0)], [ok, bad])], want_j=[jrow(200)], pair=off))
        out.append(pcase("fusion_" + name + "_discordant", [([(L0, 0)], [ok, bad])], want_j=[row], pair=on))
    # left() distance exactly fusion_min_dist: no fusion pair, only too far: 0 - 8 - 6 = -14 beats -18 without discordant pairs
    out.append(pcase("fusion_min_dist_exact", [([(L0, 0)], [ok, (rec(6000, 20, 150, 20), 0)])], want_j=[(1, 6019, 6170, 0, 20, 20, 1)], pair=(200, 20, 5000, False, False)))
    # a fusion op: BAD = M20 FF3000 M20 (no junction), AS -5, comes first: a fusion pair, -5 - 6 = -11, skipped; OK (AS -2: -10) raises the best
    # and is reported.  Were it no fusion pair it would score -5, and OK, below it, would not enter the list.
    fus = ((1, 1240, False, [(M, 20), (FF, 3000), (M, 20)], 1), -5)
    out.append(pcase("fusion_op", [([(L0, 0)], [fus, (right_at(200), -2)])], want_j=[jrow(200)]))
    # the list holds two scores (max_penalty 5).  Five left-only singletons show A's and B's junctions: first-pass support 6, no penalty.
    # A (-10) enters; F, unspliced on the other contig, 0 - 5 = -5, raises the best and is skipped; B (-5) equals the best and enters: [A, B].
    a, b, f = right_at(200), right_at(205, 130), plain(1240, 40, ref=2)
    out.append(pcase("skipped_fusion_raises_the_best", [([(a, 0), (b, 0)], [])] * 5 + [([(L0, 0)], [(a, -10), (f, 0), (b, -5)])], want_j=[jrow(200), jrow(205, 130)],
                     best=(20, False, 5)))
    # ---- the per-side cutoff: max_multihits 2, five records a side.  The fifth (AS -1) is the best of the five; the sixth (AS 0) is not looked at.
    six = [(right_at(180 + 5 * k), -5 + k) for k in range(6)]
    out.append(pcase("sixth_record_is_not_looked_at", [([(L0, 0)], six)], want_j=[jrow(200)], best=(2, False, 6)))
    # ---- duplicates.  Three left-only singletons show X's junction (first-pass right extent 9, from Y, below min_extent 10: at support 5 it
    # costs (int)(8 * 0.5) = 4, below 5 it costs 8).  X (0) and Y (0) are neighbours after the first sort: one pair, support 3 + 1 = 4, X scores
    # -8 in the second pass and the unspliced W (-5) wins: no row.
    w = plain(1240, 40)
    out.append(pcase("pair_duplicates_neighbours", [([(X, 0)], [])] * 3 + [([(L0, 0)], [(X, 0), (Y, 0), (w, -5)])], want_j=[]))
    # X (0), W (-5), Y (-6): not neighbours, both pairs stay, support 3 + 2 = 5: X scores -4 and wins
    out.append(pcase("pair_duplicates_not_neighbours", [([(X, 0)], [])] * 3 + [([(L0, 0)], [(X, 0), (w, -5), (Y, -6)])], want_j=[JX], want_i=1))
    # ---- first-pass multiplicity.  Inserts 0-2: S with one mate: support 3.  Insert 3: S with two mates: two pairs, S counts twice: 5.
    # Insert 4: S (0) or ALT (-6) with one mate: at support 5 (its own pair makes 6) S costs nothing and wins.  Final: 3 + 2 + 1.
    one = ([(S, 0)], [(MATE, 0)])
    out.append(pcase("left_record_in_two_pairs", [one] * 3 + [([(S, 0)], [(MATE, 0), (plain(1345, 40), 0)]), ([(S, 0), (ALT, -6)], [(MATE, 0)])], want_j=[JS + (20, 20, 6)]))
    # the same with insert 3 like the others: support 3 + 1 + 1 = 5 ... so take one away: support 4, S costs 8 and ALT wins.  Final: 3.
    out.append(pcase("left_record_in_one_pair", [one] * 2 + [one, ([(S, 0), (ALT, -6)], [(MATE, 0)])], want_j=[JS + (20, 20, 3)]))
    # ---- no pair in the first pass: the hit groups as they came, unfiltered.  Insert 3's left record has 1 mismatch (limits 0 / 2 / 2): no
    # candidate, no pair, and the record counts all the same: support 3 + 1 + 1 = 5, S wins insert 4.  Final: 3 + 1 (the second pass filters).
    out.append(pcase("no_pair_counts_unfiltered", [one] * 3 + [([(S, 0, 1)], [(MATE, 0)]), ([(S, 0), (ALT, -6)], [(MATE, 0)])], want_j=[JS + (20, 20, 4)], limits=(0, 2, 2)))
    # ---- the cap and the draws (mixed alignments reported, max_multihits 2).  Insert 0, a left singleton, and insert 1, a right singleton, report:
    # one draw each.  Insert 2 reports one pair: the third draw.  Insert 3: T1 .. T4 (inner 180 .. 195, AS -1: -9 each) tie: 4005303368 % 4 = 0
    # erases T1, 491263 % 3 = 1 erases T3.  T2 and T4 are reported.
    tt = [(right_at(180 + 5 * k), -1) for k in range(4)]
    mixed = (200, 20, 10000000, True, False)
    lead = [([(L0, 0)], []), ([], [(w, 0)]), ([(L0, 0)], [(w, 0)])]
    out.append(pcase("cap_draws_after_singletons_and_a_pair", lead + [([(L0, 0)], tt)], want_j=[jrow(185), jrow(195)], best=(2, False, 6), pair=mixed))
    # Pairs above the ties (max_multihits 3, no mixed alignments: the singletons report nothing and do not draw; insert 2's draw is the first).
    # Insert 3: T1 .. T4 enter at -9; F (unspliced, other contig, AS -2: -8) raises the best and is skipped; B (inner 200, AS 0: -8) enters.  Sorted:
    # B, T1 .. T4; the score at place 2 is -9, one pair above it, four ties: 4282876139 % 4 = 3 erases T4, 3093770124 % 3 = 0 erases T1.
    withf = tt + [(plain(1240, 40, ref=2), -2), (right_at(200), 0)]
    out.append(pcase("cap_pairs_above_the_ties", lead + [([(L0, 0)], withf)], want_j=[jrow(185), jrow(190), jrow(200)], best=(3, False, 6)))
    # --suppress-hits with mixed alignments: the list is emptied, so both sides go down the single-end way; the right read's best record is the
    # unspliced F (-2): no row
    out.append(pcase("cap_suppressed", lead + [([(L0, 0)], withf)], want_j=[], best=(3, True, 6), pair=mixed))
    # The cap draws inside pair_best_alignments, also when the pairs are then given up.  Insert 0 = that insert with mixed alignments: 1791095845 %
    # 4 = 1 and 4282876139 % 3 = 2 are drawn, but the best grade is F's, a fusion grade: both sides go single-end -- the left read reports (third
    # draw), the right read reports F (fourth).  Insert 1: T1 .. T4 tie (first-pass support 2 each: still 8), 491263 % 4 = 3 erases T4.
    out.append(pcase("cap_draws_then_the_pairs_are_given_up", [([(L0, 0)], withf), ([(L0, 0)], tt)], want_j=[jrow(180), jrow(185), jrow(190)], best=(3, False, 6), pair=mixed))
    # ---- mixed alignments.  The only pair is a fusion pair (other contig): skipped, the list is empty.  First pass: no pair, both records count
    # (support 1 each).  With mixed alignments both reads take the single-end way and are reported; without, nothing is.
    lone = [([(S, 0)], [(rec(1300, 20, 100, 20, ref=2), 0)])]
    out.append(pcase("empty_list_mixed", lone, want_j=[JS + (20, 20, 1), (2, 1319, 1420, 0, 20, 20, 1)], pair=mixed))
    out.append(pcase("empty_list_default", lone, want_j=[]))
    # A (-10 - 8) enters, then the unspliced F on the other contig (0 - 6) raises the best and is skipped: the best grade is a fusion grade.
    # Default: the list [A] is reported.  Mixed: both sides single-end, and the right read alone prefers F (0) to A (-18): no row.
    bf = [([(L0, 0)], [(right_at(200), -10), (plain(1240, 40, ref=2), 0)])]
    out.append(pcase("best_grade_is_a_fusion_grade_default", bf, want_j=[jrow(200)]))
    out.append(pcase("best_grade_is_a_fusion_grade_mixed", bf, want_j=[], pair=mixed))
    # ---- the default: a lone mate counts in the first pass only.  Five singletons show S: support 5 + 1; S (0) beats ALT (-6); final: 1
    out.append(pcase("lone_mates_first_pass_only", [([(S, 0)], [])] * 5 + [([(S, 0), (ALT, -6)], [(MATE, 0)])], want_j=[JS + (20, 20, 1)]))
    out.append(pcase("lone_mates_four", [([(S, 0)], [])] * 3 + [([(S, 0), (ALT, -6)], [(MATE, 0)])], want_j=[]))      # 3 + 1 = 4: S costs 8
    # ---- the deletion and insertion sets.  A left record with a deletion (M20 D2 M20, it ends at 1042) and two mates 200 and 205 behind it: two
    # pairs tie at 0, both are reported, the record counts twice: the deletion's support is 2
    ld = (1, 1000, False, [(M, 20), (5, 2), (M, 20)])
    out.append(pcase("deletion_counts_once_per_pair", [([(ld, 0)], [(plain(1242, 40), 0), (plain(1247, 40), 0)])], want_d=[(1, 1019, 1022, 20, 20, 2)]))
    # Two insertions of one base at one place with different letters (max_penalty 5).  R1 (1 mismatch, so no duplicate of R2; AS -10) enters; F
    # (other contig, 0 - 5) raises the best and is skipped; R2 (-5) enters.  The list is sorted R2, R1: the right records are seen in that
    # order and R2's letter G is kept, although R1 (letter C) comes first among the records.
    r12 = (1, 1240, False, [(M, 20), (I, 1), (M, 19)])
    sq = {"L": ["A" * 40], "R": ["A" * 20 + "C" + "A" * 19, "T" * 40, "A" * 20 + "G" + "A" * 19]}
    out.append(pcase("insertion_letters_follow_the_pair_list", [([(L0, 0)], [(r12, -10, 1), (plain(1240, 40, ref=2), 0), (r12, -5, 0)])], want_i=1, seqs=sq,
                     want_ins=[(1, 1259, "G", 20, 19, 2)], best=(20, False, 5)))
    return out


def as_single(c, seqs=None):
    """the records of a case as ONE single-end input in visit order (every side a read): best_ref.consensus's arguments (with seqs = {"L": ..,
    "R": ..} the SEQs in that order too, as a sixth list)"""
    import pair_ref as pr
    recs, reads, AS, mism, anti, sq = [], [], [], [], [], []
    n = 0
    for _num, li, ri in pr.inserts(c["L"], c["R"]):
        for name, sd, idx in (("L", c["L"], li), ("R", c["R"], ri)):
            for k in idx:
                recs.append(sd["recs"][k]); reads.append(n); AS.append(sd["AS"][k]); mism.append(sd["mism"][k]); anti.append(sd["anti"][k])
                if seqs is not None:
                    sq.append(seqs[name][k])
            n += 1 if idx else 0
    return (recs, reads, AS, mism, anti) if seqs is None else (recs, reads, AS, mism, anti, sq)


def crowd(seed=5, n_inserts=600, max_multihits=3, fusion_ops=True):
    """a seeded crowd of inserts over about 30 junction sites: proper pairs at all distances around the window, too-far pairs over
    well-supported junctions, mates on the other contig, on the same strand and upstream, fusion ops, pair duplicates, many-record sides,
    singletons of both sides, mismatching records -> a case dict without expectations.  fusion_ops false: no record with a fusion op (a BAM needs two records and XF:Z for one)"""
    rng = np.random.default_rng(seed)
    sites = [(int(rng.integers(1, 3)), 400 + 600 * k + int(rng.integers(0, 30)), int(rng.integers(80, 400)), bool(rng.integers(0, 2))) for k in range(30)]
    weight = rng.integers(1, 12, len(sites)).astype(float)
    weight /= weight.sum()

    def spliced():
        ref, at, gap, anti = sites[int(rng.choice(len(sites), p=weight))]
        a, b = int(rng.integers(9, 30)), int(rng.integers(8, 30))
        return (ref, at - a, anti, [(M, a), (N, gap), (M, b)])

    def end(r):
        return r[1] + sum(ln for op, ln in r[3] if op in (M, N))

    def mate_of(r, kind):
        inner = int(rng.choice([150, 179, 180, 200, 220, 221, 239, 240, 300]))
        if kind == "far":                                       # a too-far mate: often over the next sites' junctions
            inner = int(rng.integers(500, 1500))
        ref = r[0]
        if kind == "contig":
            ref = 3 - ref
        left = end(r) + inner if kind != "upstream" else max(10, r[1] - 300)
        m = plain(left, 40, ref) if rng.integers(0, 3) else (ref, left, False, [(M, 20), (N, int(rng.integers(60, 90))), (M, 20)])
        if end(m) >= 19900:
            m = plain(19000, 40, ref)
        return m

    ins = []
    for _ in range(n_inserts):
        kind = int(rng.integers(0, 18))
        r = spliced()
        if kind <= 2:
            ins.append(([(r, int(-rng.integers(0, 4)))], [(mate_of(r, "near"), int(-rng.integers(0, 4)))]))
        elif kind == 3:
            ins.append(([(r, int(-rng.integers(0, 8))), (plain(r[1], 40, r[0]), int(-rng.integers(0, 8)))], [(mate_of(r, "near"), 0), (mate_of(r, "far"), 0)]))
        elif kind == 4:
            ins.append(([(r, 0)], [(mate_of(r, "far"), int(-rng.integers(0, 3))), (mate_of(r, "near"), int(-rng.integers(3, 9)))]))
        elif kind == 5:
            bad = mate_of(r, str(rng.choice(["contig", "upstream"])))
            ins.append(([(r, 0)], [(mate_of(r, "near"), int(-rng.integers(0, 12))), (bad, 0)][::int(rng.choice([1, -1]))]))
        elif kind == 6:                                          # equal strands, or a fusion op on the mate
            if rng.integers(0, 2) or not fusion_ops:
                ins.append(([(r, 0)], [(mate_of(r, "near"), int(-rng.integers(0, 9)), 0, False), (mate_of(r, "near"), int(-rng.integers(4, 12)))]))
            else:
                ins.append(([(r, 0)], [((r[0], end(r) + 200, False, [(M, 20), (FF, 3000), (M, 20)], r[0]), int(-rng.integers(0, 6))), (mate_of(r, "near"), int(-rng.integers(0, 12)))]))
        elif kind == 7:                                          # pair duplicates: equal under cmp_read_equal, different cigars
            left = end(r) + 200
            x = (r[0], left, False, [(M, 20), (N, 70), (M, 8), (I, 1), (M, 11)])
            y = (r[0], left, False, [(M, 20), (N, 70), (M, 9), (I, 1), (M, 10)])
            mid = (plain(left + 3, 40, r[0]), int(-rng.integers(0, 3)))
            ins.append(([(r, 0)], [(x, int(-rng.integers(0, 2))), mid, (y, int(-rng.integers(0, 2)))]))
        elif kind in (8, 12):                                    # many records a side, tied: a side is cut, the host sorts, the cap draws
            k1, k2 = int(rng.integers(1, 5)), int(rng.integers(2, 13))
            base = end(r) + 180
            ins.append(([(r, 0)] + [(plain(r[1] + 2 * j, 40 + j, r[0]), 0) for j in range(1, k1)], [(plain(base + 3 * int(j), 40, r[0]), int(-rng.integers(0, 2))) for j in rng.permutation(k2)]))
        elif kind == 9:
            ins.append(([(r, int(-rng.integers(0, 4)))], []) if rng.integers(0, 2) else ([], [(r, int(-rng.integers(0, 4)))]))
        elif kind == 13:                                         # a too-far pair around a junction site: rescued when the site's first-pass support is >= 10
            ref, at, gap, _anti = sites[int(rng.choice(len(sites), p=weight))]
            d1 = int(rng.integers(0, 230))
            ins.append(([(plain(at - d1 - 40, 40, ref), 0)], [(plain(at + gap + int(rng.choice([179, 180, 200, 220, 221])) - d1, 40, ref), int(-rng.integers(0, 3))),
                                                               (plain(at - d1 + 200, 40, ref), int(-rng.integers(2, 7)))]))
        elif kind == 14:                                         # the mate inside the left record's span
            ins.append(([(r, 0)], [(plain(r[1] + 2, 30, r[0]), int(-rng.integers(0, 3))), (mate_of(r, "near"), int(-rng.integers(0, 6)))]))
        elif kind == 15:                                         # A .. enter, F on the other contig raises the best and is skipped, B .. enter: two scores in one list
            e = end(r)
            a_ = [(plain(e + 200 + 2 * k, 40, r[0]), -10) for k in range(int(rng.integers(1, 5)))]
            b_ = [(plain(e + 190 + 2 * k, 40, r[0]), -6) for k in range(int(rng.integers(1, 4)))]
            ins.append(([(r, 0)], a_ + [(plain(e + 200, 40, 3 - r[0]), 0)] + b_))
        elif kind == 16 and fusion_ops:                          # fusion ops on both sides: the pair is not allowed
            fl = (r[0], r[1], False, [(M, 20), (FF, 5000), (M, 20)], r[0])
            fr = (r[0], end(r) + 200, False, [(M, 20), (FF, 3000), (M, 20)], r[0])
            ins.append(([(fl, 0), (r, int(-rng.integers(0, 6)))], [(fr, 0), (mate_of(r, "near"), int(-rng.integers(0, 6)))]))
        elif kind == 17:                                         # a left record with a deletion, often in two pairs; a mate with an insertion
            ld = (r[0], r[1], False, [(M, 20), (5, int(rng.integers(1, 3))), (M, 20)])
            ins.append(([(ld, 0)], [(plain(r[1] + 242 + int(rng.integers(0, 3)), 40, r[0]), 0), ((r[0], r[1] + 246, False, [(M, 20), (I, 1), (M, 19)]), int(-rng.integers(0, 2)))]))
        elif kind == 10:                                         # a mismatching record beside a clean one
            ins.append(([(r, -6, 1), (r, 0, 0)][::int(rng.choice([1, -1]))], [(mate_of(r, "near"), 0, int(rng.integers(0, 2)))]))
        else:
            ins.append(([(r, 0), (spliced(), 0)], [(mate_of(r, "near"), 0)]))
    return pcase("crowd", ins, best=(max_multihits, False, 6))
