"""Test infrastructure: hand-made record lists for the fusions.out tests (CPU and GPU), in fusionsout_ref's record form
(ref_id, left, antisense_splice, [(op, len) ...], ref_id2 or 0, read_idx, edit_dist).  The genome: two contigs of 3000 and 2000
bases, seeded, with a run of N in each."""
import numpy as np

M, m, I, i_, D, d, FF, FR, RF, RR, N, n, S = 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13
NAMES = ["chrA", "chrB"]


def _genome():
    rng = np.random.default_rng(41)
    a = "".join("ACGT"[k] for k in rng.integers(0, 4, 3000))
    b = "".join("ACGT"[k] for k in rng.integers(0, 4, 2000))
    return [a[:1180] + "NNNN" + a[1184:], b[:795] + "NN" + b[797:]]


GENOME = _genome()


def renumber(recs):
    """read_idx dense in [0, number of reads): the distinct values in order of first appearance"""
    ids = {}
    return [r[:5] + (ids.setdefault(r[5], len(ids)), r[6]) for r in recs]


def directions():
    """one fusion of every direction between the contigs and inside one, seen by one to three reads with different anchors, and
    contiguous reads over some of their ends"""
    recs = [
        (1, 1000, False, [(M, 60), (FF, 500), (M, 40)], 2, 0, 0),                          # FF: left 1059, right 500
        (1, 1020, False, [(M, 40), (FF, 500), (M, 55)], 2, 1, 1),
        (1, 1150, False, [(M, 50), (FR, 800), (m, 50)], 2, 2, 0),                          # FR: left 1199 (beside the N run), right 800
        (1, 700, False, [(m, 45), (RF, 900), (M, 55)], 2, 3, 0),                           # RF: left 656, right 900
        (1, 700, False, [(m, 30), (n, 100), (m, 25), (RF, 900), (M, 55)], 2, 4, 2),        # RF behind a junction: left 700 - 155 + 1 = 546, left_pos 155
        (1, 2000, False, [(m, 50), (RR, 1500), (m, 50)], 2, 5, 0),                         # RR: left 1951, right 1500
        (2, 300, False, [(M, 50), (FF, 2500), (M, 50)], 1, 6, 0),                          # its key swaps: (1, 2, 2500, 349)
        (1, 400, False, [(M, 30), (FF, 2200), (M, 70)], 1, 7, 0),                          # one contig, left 429 < right 2200
        (1, 2300, False, [(M, 30), (FF, 150), (M, 70)], 1, 8, 0),                          # one contig, swaps: (1, 1, 150, 2329)
        (1, 10, False, [(M, 25), (FF, 1000), (M, 75)], 2, 9, 0),                           # left 34: within 50 bases of the contig's start
        (1, 1500, False, [(M, 50), (FF, 1960), (M, 40)], 2, 10, 0),                        # right 1960: 1960 + 50 > 2000
        (1, 1500, False, [(M, 50), (FF, 1950), (M, 50)], 2, 11, 0),                        # right + 50 == the contig's length: the window ends one base past it
        # contiguous reads
        (1, 1000, False, [(M, 100)], 0, 12, 0),                                            # covers 1059 (chrA end of the FF fusion)
        (2, 450, False, [(M, 100)], 0, 13, 0),                                             # covers 500 (its chrB end: through the mirror)
        (1, 380, False, [(M, 100)], 0, 14, 1),                                             # covers 429
        (1, 100, False, [(M, 2250)], 0, 15, 0),                                            # covers 429 and 2200, 150 and 2329 ...: both ends of two fusions
    ]
    return recs


def walker_cases():
    """shapes for the walkers alone: lower-case pieces, a fusion op as the first and as the last op, positions that wrap below 0,
    indels and clips around the op"""
    return [
        (1, 5, False, [(m, 10), (FF, 500), (M, 40)], 2, 0, 0),                             # 5 - 10 - 1 wraps
        (1, 0, False, [(FF, 500), (M, 40)], 2, 1, 0),                                      # first op; 0 - 1 wraps
        (1, 100, False, [(M, 40), (RF, 500)], 2, 2, 0),                                    # last op
        (1, 0xFFFFFFF0 - (1 << 32), False, [(M, 10), (RR, 7), (m, 30)], 1, 3, 0),
        (2, 1000, False, [(S, 5), (M, 20), (I, 2), (M, 10), (D, 3), (M, 10), (FR, 900), (m, 15), (d, 2), (m, 10), (i_, 2), (m, 12), (S, 3)], 1, 4, 0),
        (2, 1000, False, [(m, 20), (n, 150), (m, 30), (RR, 700), (m, 30), (n, 90), (m, 20)], 2, 5, 0),
        (1, 700, False, [(M, 25), (N, 300), (M, 25), (FF, 700), (M, 50)], 1, 6, 0),        # one contig, position 1049 not below length 700: swaps
        (1, 651, False, [(M, 50), (FF, 700), (M, 50)], 1, 7, 0),                           # position 700 == length 700: its own mirror
        (1, 100, False, [(M, 39)], 0, 8, 0), (1, 100, False, [(M, 40)], 0, 9, 0),
        (1, 100, False, [(M, 20), (I, 2), (M, 18)], 0, 10, 0), (1, 100, False, [(S, 4), (M, 36)], 0, 11, 0),
        (1, 100, False, [(m, 40)], 0, 12, 0), (1, 100, False, [(M, 20), (N, 100), (M, 20)], 0, 13, 0),
        (1, 100, False, [(M, 20), (D, 5), (M, 20)], 0, 14, 0), (1, 10, False, [(m, 40)], 0, 15, 0),
    ]


def crowd(seed=9, n_reads=600):
    """reads with one to four alignments on a few break points: anchors around 20 and 50, edit distances 0..4, some fusion records
    behind junctions that the filter drops, contiguous and spliced reads over the break points"""
    rng = np.random.default_rng(seed)
    breaks = [(1, 1059, 2, 500, FF), (1, 1199, 2, 800, FR), (1, 656, 2, 900, RF), (1, 1951, 2, 1500, RR), (1, 429, 1, 2200, FF), (2, 600, 2, 1400, FF)]
    recs = []
    for read in range(n_reads):
        for _ in range(int(rng.choice([1, 1, 1, 2, 2, 3, 4]))):
            ed = int(rng.choice([0, 0, 1, 2, 3, 4]))
            kind = int(rng.integers(0, 10))
            r1, l, r2, r, dr = breaks[int(rng.integers(0, len(breaks)))]
            a, b = int(rng.choice([15, 19, 20, 21, 30, 49, 50, 51, 60])), int(rng.choice([15, 19, 20, 21, 30, 49, 50, 51, 60]))
            if kind < 5:
                first_up = dr in (FF, FR)
                second_up = dr in (FF, RF)
                left = l + 1 - a if first_up else l - 1 + a
                cig = [(M if first_up else m, a)]
                if kind == 0:                                     # a junction in front, its anchor sometimes too short for the filter
                    j = int(rng.choice([5, 9, 25]))
                    cig = [(M if first_up else m, j), (N if first_up else n, 80)] + cig
                    left = left - j - 80 if first_up else left + j + 80
                cig += [(dr, r), (M if second_up else m, b)]
                recs.append((r1, left, bool(rng.integers(0, 2)), cig, r2, read, ed))
            elif kind < 8:
                ref, at = (r1, l) if rng.integers(0, 2) else (r2, r)
                ln = int(rng.choice([39, 40, 60, 100]))
                off = int(rng.choice([19, 20, 21, ln - 21, ln - 20, ln - 19]))
                recs.append((ref, max(0, at - off), False, [(M, ln)], 0, read, ed))
            else:
                recs.append((r1, max(0, l - 30), False, [(M, 25), (N, 70), (M, int(rng.choice([5, 30])))], 0, read, ed))
    return recs


def sim_input(recs):
    """the records as tests/fusionsim reads them"""
    return "".join("%d %d %d %d %s\n" % (r[0], r[1], r[4], len(r[3]), " ".join("%d %d" % (op, ln) for op, ln in r[3])) for r in recs)


def sim_expected(recs, ref):
    """what tests/fusionsim prints for them, from the restatement's walkers (ref = the fusionsout_ref module)"""
    out = []
    for k, r in enumerate(recs):
        out.append("R %d" % k)
        f = ref.rec_fusion(r)
        if f:
            out.append("F %d %d %d %d %d %d %d %d" % (f[0] + (f[1], f[2], 1 if f[3] else 0)))
        u = ref.rec_unsplit(r)
        out.append("U %d %d %d" % (u[0], u[1], 1 if u[2] else 0))
    return "\n".join(out) + "\n"
