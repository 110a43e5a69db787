"""Test infrastructure: hand-made record lists for the indel consensus tests (CPU and GPU), in indelbed_ref's record form
(ref_id, left, antisense_splice, [(op, len) ...][, ref_id2]).  The genome they live on: two contigs of 20000 bases."""
import numpy as np

M, m, I, i_, D, d, FF, FR, RF, RR, N, n, S = 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13
GENOME = ["ACGT" * 5000, "TTGCA" * 4000]
NAMES = ["chrA", "chrB"]


def seq_len(rec):
    """bases of the record's SEQ: M, m, I, i and soft clips"""
    return sum(ln for op, ln in rec[3] if op in (M, m, I, i_, S))


def make_seqs(recs, seed, alphabet="ACGT"):
    rng = np.random.default_rng(seed)
    return ["".join(alphabet[k] for k in rng.integers(0, len(alphabet), seq_len(r))) for r in recs]


def _rec(left, a, gap, b, anti=False, ref=1):
    return (ref, left, anti, [(M, a), (N, gap), (M, b)])


def filter_cases():
    """the filter cases of test_juncbed_cpu / test_gpu_juncbed (copied, not imported: see there for what each one shows)"""
    cases = [
        [_rec(100, 20, 500, 7)],
        [_rec(100, 20, 500, 7), _rec(90, 30, 500, 12)],
        [_rec(100, 20, 60000, 20)], [_rec(100, 20, 60000, 20)] * 2, [_rec(100, 20, 60000, 12)] * 2,
        [_rec(100, 20, 500, 20, anti=False)] * 3 + [_rec(103, 20, 497, 20, anti=True)],
        [_rec(100, 20, 500, 20, anti=False)] * 2 + [_rec(103, 20, 497, 20, anti=True)] * 2,
        [(1, 100, False, [(M, 20), (N, 300), (M, 30), (N, 400), (M, 25)])],
        [(1, 100, False, [(M, 20), (N, 300), (M, 30), (N, 400), (M, 5)])],
        [(2, 1000, True, [(M, 10), (D, 3), (M, 10), (N, 100), (M, 15), (I, 2), (M, 9)])],
        [_rec(3, 9, 100, 30), _rec(5, 9, 98, 30, anti=True), _rec(5, 9, 98, 30, anti=True)],
        [],
    ]
    rng = np.random.default_rng(3)
    many = []
    for _ in range(3000):
        l0 = int(rng.integers(50, 400))
        many.append(_rec(l0, int(rng.integers(5, 40)), int(rng.integers(60, 90)), int(rng.integers(5, 40)), anti=bool(rng.integers(0, 2)), ref=int(rng.integers(1, 3))))
    cases.append(many)
    return cases


def fusion_cases():
    """the fusion list of test_gpu_juncbed._fusion_cases (copied)"""
    return [
        (1, 1000, False, [(M, 30), (N, 200), (M, 20), (FF, 5000), (M, 50)], 2),
        (1, 1000, False, [(M, 30), (N, 200), (M, 20), (FF, 5000), (M, 25), (N, 300), (M, 25)], 2),
        (1, 1000, True, [(M, 30), (N, 200), (M, 20), (FR, 9000), (m, 25), (n, 300), (m, 25)], 2),
        (2, 4000, False, [(m, 20), (n, 150), (m, 30), (RF, 700), (M, 30), (N, 90), (M, 20)], 1),
        (2, 4000, False, [(m, 20), (n, 150), (m, 30), (RR, 700), (m, 30), (n, 90), (m, 20)], 1),
        (1, 2000, False, [(M, 12), (D, 2), (M, 10), (N, 500), (M, 28), (FF, 3000), (M, 20), (I, 1), (M, 29)], 2),
        (1, 1000, False, [(M, 30), (N, 200), (M, 70)]), (1, 1000, False, [(M, 30), (N, 200), (M, 70)]),
        (2, 5025, False, [(M, 25), (N, 300), (M, 25)]),
        (2, 8675, True, [(M, 25), (N, 300), (M, 25)]),
    ]


def fusion_indel_cases():
    """that list's shape with d and i ops on both sides of every fusion direction: the dEL advance of the deletion walker (UP, unlike
    the other two walkers), iNS at pos + 1, ref_id2 behind FF / FR / RF, and RR, which no walker has a case for"""
    return fusion_cases() + [
        (1, 1000, False, [(M, 20), (I, 2), (M, 10), (D, 3), (M, 10), (FF, 5000), (M, 15), (I, 1), (M, 10), (D, 2), (M, 20)], 2),
        (1, 1500, False, [(M, 20), (D, 2), (M, 12), (I, 3), (M, 10), (FR, 9000), (m, 15), (d, 2), (m, 10), (i_, 2), (m, 12), (d, 1), (m, 9)], 2),
        (2, 4000, False, [(m, 20), (d, 3), (m, 10), (i_, 1), (m, 12), (d, 2), (m, 8), (RF, 700), (M, 30), (I, 2), (M, 10), (D, 1), (M, 12)], 1),
        (2, 6000, False, [(m, 20), (i_, 2), (m, 10), (d, 2), (m, 30), (RR, 700), (m, 30), (d, 3), (m, 5), (i_, 1), (m, 20)], 1),
        (1, 3000, False, [(M, 30), (N, 200), (M, 20), (D, 2), (M, 10), (FF, 5000), (M, 25), (N, 300), (M, 12), (I, 2), (M, 13)], 2),
        (1, 3000, True, [(M, 30), (N, 200), (M, 20), (D, 2), (M, 10), (FR, 5037), (m, 25), (n, 300), (m, 12), (i_, 2), (m, 13), (d, 4), (m, 11)], 2),
        (1, 700, False, [(S, 5), (M, 20), (I, 3), (M, 25), (S, 2)]),            # clips: the letters come from SEQ[20:23], not [25:28]
        (1, 700, False, [(M, 25), (I, 3), (M, 25)]),
    ]


def crowd(seed=5, n_recs=3000, n_places=40):
    """records on two contigs whose indels fall on about n_places places with lengths 1..3, half of them also carrying a junction
    close to the junctions of the same place's other records, on either strand, with anchors that are sometimes too short"""
    rng = np.random.default_rng(seed)
    places = [(int(rng.integers(1, 3)), 500 + 450 * k + int(rng.integers(0, 50))) for k in range(n_places)]
    recs = []
    for _ in range(n_recs):
        ref, pos = places[int(rng.integers(0, n_places))]
        a, ln = int(rng.integers(10, 30)), int(rng.integers(1, 4))
        op = (I, D, i_, d)[int(rng.integers(0, 4))] if rng.integers(0, 4) == 0 else (I, D)[int(rng.integers(0, 2))]
        up = op in (I, D)
        mt, nn = (M, N) if up else (m, n)
        left = pos - a if up else pos + a
        cig = [(mt, a), (op, ln)]
        if rng.integers(0, 2):
            # the junction 60 bases behind the place (+ 0..3), whatever the indel moved
            at = a + (ln if op in (D, d) else 0)
            b = 60 + int(rng.integers(0, 4)) - (at - a)
            cig += [(mt, b), (nn, int(rng.integers(60, 90))), (mt, int(rng.integers(5, 40)))]
        else:
            cig += [(mt, int(rng.integers(10, 40)))]
        recs.append((ref, left, bool(rng.integers(0, 2)), cig))
    return recs


def sim_input(recs):
    """the records as tests/indelsim reads them"""
    return "".join("%d %d %d %d %s\n" % (r[0], r[1], r[4] if len(r) > 4 else 0, len(r[3]), " ".join("%d %d" % (op, ln) for op, ln in r[3])) for r in recs)


def sim_expected(recs, ref):
    """what tests/indelsim prints for them, from the restatement's walkers (ref = the indelbed_ref module)"""
    out = []
    for k, r in enumerate(recs):
        out.append("R %d" % k)
        out += ["J %d %d %d %d %d" % (j[0], j[1], j[2], j[4], j[5]) for j in ref.rec_juncs(r)]
        out += ["D %d %d %d %d %d %d" % x for x in ref.rec_dels(r)]
        for (rf, l, s, le, re, c) in ref.rec_inss(r, range(seq_len(r))):         # a "SEQ" whose letters are their own offsets
            out.append("I %d %d %d %d %d %d %d" % (rf, l, len(s), s[0] if len(s) else 0, le, re, c))
    return "\n".join(out) + "\n"
