"""GPU: inserts are graded (thj_juncbed_pair_alignments, thj_juncbed_add_pairs) against the restatement (pair_ref.py): the hand-worked
cases and the crowd of pair_cases.py with and without the annotation, the read filter, mixed and discordant alignments; candidate lists of
the sizes at which the sort changes hands (16 / 17) and a side is cut; inserts across workgroup, grid-stride and add-call boundaries; the
contract."""
import numpy as np
import pytest

import best_cases as bc
import best_ref as br
import indelbed_ref as ir
import jbknown_ref as jr
import pair_cases as pc
import pair_ref as pr
from tophat_amd import host

pytestmark = pytest.mark.gpu


def side_alns(S, lo, hi):
    """the records of inserts lo .. hi - 1 of a side as an ALN_DTYPE array; read_idx = the insert's number inside the call"""
    idx = [k for k, num in enumerate(S["reads"]) if lo <= num < hi]
    a = host.aln_array_from_tuples([S["recs"][k] for k in idx]) if idx else np.zeros(0, dtype=host.ALN_DTYPE)
    if idx:
        a["mismatches"] = [S["mism"][k] for k in idx]
        a["AS"] = [S["AS"][k] for k in idx]
        a["flags"] |= np.array([1 if S["anti"][k] else 0 for k in idx], dtype=np.uint8)
        a["read_idx"] = np.array([S["reads"][k] for k in idx], dtype=np.int64) - lo
    return a


def n_inserts(c):
    return max(c["L"]["reads"] + c["R"]["reads"]) + 1


def ins_seqs(S, seqs, lo, hi):
    return [ir.ins_letters(S["recs"][k][:5], seqs[k]) for k, num in enumerate(S["reads"]) if lo <= num < hi]


def run(ctx, c, cuts=(), seqs=None, **over):
    """one paired consensus through the Context -> junction rows, or with seqs = {"L": .., "R": ..} (junction, insertion, deletion rows); cuts:
    the inserts go in as several add_pairs calls"""
    c = dict(c, **over)
    ctx.juncbed_reset()
    if seqs is not None:
        ctx.juncbed_collect_indels(True)
    if c["known"]:
        ctx.juncbed_known_junctions(c["known"])
    if c["limits"] is not None:
        ctx.juncbed_read_filter(True, *c["limits"])
    ctx.juncbed_best_alignments(True, *c["best"])
    ctx.juncbed_pair_alignments(True, *c["pair"])
    edges = [0] + list(cuts) + [n_inserts(c)]
    for lo, hi in zip(edges, edges[1:]):
        if seqs is None:
            ctx.juncbed_add_pairs(side_alns(c["L"], lo, hi), side_alns(c["R"], lo, hi))
        else:
            ctx.juncbed_add_pairs_seq(side_alns(c["L"], lo, hi), ins_seqs(c["L"], seqs["L"], lo, hi), side_alns(c["R"], lo, hi), ins_seqs(c["R"], seqs["R"], lo, hi))
    js = ir.junc_rows(ctx.juncbed_finish(c["anchor"]))
    if seqs is None:
        return js
    ins, dels = ctx.juncbed_indels()
    return js, ir.ins_rows(ins), ir.del_rows(dels)


def want(c, seqs=None, **over):
    c = dict(c, **over)
    return pr.consensus(c["L"], c["R"], c["best"], c["pair"], c["anchor"], c["known"], c["limits"], seqs)


def counts(c, **over):
    c = dict(c, **over)
    return pr.choose(c["L"], c["R"], c["best"], c["pair"], c["anchor"], c["known"], c["limits"])["counts"]


@pytest.fixture(scope="module")
def ctx():
    with host.Context(0) as c:
        c.upload_genome(host.pack_genome(pc.GENOME))
        yield c


@pytest.fixture(scope="module")
def crowd():
    return pc.crowd()


def test_cases_by_hand(ctx):
    for c in pc.cases():
        got = run(ctx, c)
        assert got == c["want_j"], c["label"]
        assert got == want(c), c["label"]
        assert ctx.juncbed_pair_counts() == counts(c), c["label"]
        sq = pc.seqs_of(c)
        j, i, d = run(ctx, c, seqs=sq)                          # and with the indel sets
        assert (j, d, len(i)) == (c["want_j"], c["want_d"], c["want_i"]) and (j, i, d) == want(c, sq), c["label"]
        assert c["want_ins"] is None or i == c["want_ins"], c["label"]


def test_crowd(ctx, crowd):
    c = crowd
    distinct = sorted({j[:4] for S in (c["L"], c["R"]) for r in S["recs"] for j in ir.rec_juncs(r)})
    mixed, disc, both = (200, 20, 10000000, True, False), (200, 20, 10000000, False, True), (150, 30, 900, True, True)
    seen = set()
    sq = pc.seqs_of(c, 3)
    for over in ({}, {"known": distinct[::3]}, {"limits": (0, 2, 2)}, {"pair": mixed}, {"pair": disc}, {"pair": both, "best": (2, False, 5)}, {"best": (2, True, 6), "pair": mixed},
                 {"known": distinct[1::4], "limits": (0, 2, 2), "anchor": 12, "pair": mixed}):
        got = run(ctx, c, **over)
        assert got == want(c, **over), over
        full = run(ctx, c, seqs=sq, **over)
        assert full == want(c, sq, **over) and full[0] == got and len(full[1]) > 3, over
        assert ctx.juncbed_pair_counts() == counts(c, **over), over
        seen.add(repr(got))
    assert len(seen) == 8
    # two add_pairs calls cut between inserts: same rows, the visit order and the draws go on
    assert run(ctx, c, cuts=(137,)) == run(ctx, c) and run(ctx, c, cuts=(1, 200, 399), pair=mixed) == want(c, pair=mixed)
    assert run(ctx, c, cuts=(1, 200, 399), seqs=sq, pair=mixed) == want(c, sq, pair=mixed)


def big_insert(nl, nr, seed):
    """an insert of nl x nr candidates, many of them tied: left records spliced at shifting places (their junction rows count the pairs they are
    in), right records unspliced behind them, every fifth a repeat of the one before (equal under cmp_read_equal: pair duplicates), AS 0 or -1"""
    rng = np.random.default_rng(seed)
    base = int(rng.integers(500, 3000))
    left = [(pc.rec(base + 3 * int(p), 20, 100 + int(p), 20), 0 if rng.integers(0, 3) else -1) for p in rng.permutation(nl)]
    places = [int(p) for p in rng.permutation(nr)]
    right = []
    for k, p in enumerate(places):
        p = places[k - 1] if k % 5 == 4 else p
        right.append((bc.plain(base + 340 + 2 * p, 40), 0 if rng.integers(0, 3) else -1))
    return (left, right)


SIZES = [(41, 41), (1, 1), (1, 2), (3, 5), (4, 4), (1, 17), (8, 8), (5, 13), (41, 41)]


@pytest.mark.parametrize("cap", (20, 2000))
def test_list_sizes(ctx, cap):
    """candidate lists of 1, 2, 15, 16 (the device's own sort), 17, 64, 65 and 1681 (the host's std::sort); the call's first and last inserts are
    the large ones; cap 20: the long lists are over --max-multihits and draw; cap 2000: every tied pair is reported and counted"""
    c = pc.pcase("sizes", [big_insert(nl, nr, 70 + k) for k, (nl, nr) in enumerate(SIZES)], best=(cap, False, 6))
    got = run(ctx, c)
    assert got == want(c) and len(got) > 10
    ch = pr.choose(c["L"], c["R"], c["best"], c["pair"])
    assert ctx.juncbed_pair_counts() == ch["counts"] and (ch["counts"][2] >= 2 if cap == 20 else ch["counts"][2] == 0)
    if cap == 2000:
        assert max(len(v) for v in ch["lists"].values()) > 16 and max(r[6] for r in got) > 10       # a record in many pairs counts that often
    assert run(ctx, c, cuts=(4,)) == got
    if cap == 20:
        assert run(ctx, c, best=(20, True, 6)) == want(c, best=(20, True, 6)) != got


def test_a_side_is_cut(ctx):
    """max_multihits 2: 6 x 6 records are cut to 5 x 5; the sixth records are the best ones and are not looked at"""
    left = [(pc.rec(1000 + 3 * k, 20, 100 + k, 20), 0 if k == 5 else -2) for k in range(6)]
    right = [(bc.plain(1340 + 2 * k, 40), 0 if k == 5 else -1) for k in range(6)]
    c = pc.pcase("cut", [big_insert(3, 3, 1), (left, right)], best=(2, False, 6))
    got = run(ctx, c)
    assert got == want(c)
    assert not any(r[1] == 1000 + 15 + 19 for r in got)


def test_an_insert_across_the_grid_stride(ctx):
    """the per-record kernels run 4096 workgroups of 256 threads: record 1048576 is the first of the second stride.  An insert of 1 x 130 records
    lies across it behind 524250 inserts of one unspliced record a side (each reports a pair: the generator has drawn 524250 times).  max_multihits 3:
    the right side is cut to 7 tied records, 4 of them are erased."""
    n_fill, n_big, cap = 524250, 130, 3
    left = np.zeros(n_fill + 1 + 20, dtype=host.ALN_DTYPE)
    left["ref_id"], left["left"], left["n_cigar"] = 1, 1000, 1
    left["cigar"][:, 0] = (bc.M << 28) | 40
    left["read_idx"] = np.arange(len(left))
    right = np.zeros(n_fill + n_big + 20, dtype=host.ALN_DTYPE)
    right["ref_id"], right["left"], right["n_cigar"] = 1, 1240, 1
    right["cigar"][:, 0] = (bc.M << 28) | 40
    right["flags"] = 1
    right["read_idx"] = np.concatenate([np.arange(n_fill), np.full(n_big, n_fill), n_fill + 1 + np.arange(20)])
    big = host.aln_array_from_tuples([pc.right_at(180 + (k % 40), 100 + k) for k in range(n_big)])
    big["flags"] |= 1
    big["read_idx"] = n_fill
    right[n_fill:n_fill + n_big] = big
    assert 2 * n_fill + 1 < 4096 * 256 < 2 * n_fill + 1 + n_big
    g = br.Mt19937(1)
    for _ in range(n_fill):
        g()
    tie = list(range(7))
    while len(tie) > cap:
        del tie[g() % len(tie)]
    ctx.juncbed_reset()
    ctx.juncbed_best_alignments(True, cap, False, 6)
    ctx.juncbed_pair_alignments(True)
    ctx.juncbed_add_pairs(left, right)
    got = ir.junc_rows(ctx.juncbed_finish(8))
    assert got == sorted(pc.jrow(180 + k, 100 + k) for k in tie)
    assert ctx.juncbed_pair_counts() == (n_fill + 1 + 20, n_fill + 1 + 20, 1, 0, 0)


def test_an_insert_across_a_workgroup(ctx):
    """120 inserts of one unspliced record a side, then an insert of 6 x 30 records that lies across record 256 -- the first of the second
    256-thread workgroup of the per-record kernels -- and a few more behind it; max_multihits 3: the list is over the cap and draws"""
    fill = ([(pc.L0, 0)], [(bc.plain(1240, 40), 0)])
    c = pc.pcase("workgroup", [fill] * 120 + [big_insert(6, 30, 5)] + [fill, big_insert(2, 3, 6), fill], best=(3, False, 6))
    assert 2 * 120 < 256 < 2 * 120 + 36
    sq = pc.seqs_of(c)
    got = run(ctx, c, seqs=sq)
    assert got == want(c, sq) and len(got[0]) >= 2
    st = counts(c)
    assert ctx.juncbed_pair_counts() == st and st[2] >= 1


def test_contract(ctx):
    c = [x for x in pc.cases() if x["label"] == "left_record_in_two_pairs"][0]
    L, R = side_alns(c["L"], 0, 99), side_alns(c["R"], 0, 99)
    # before thj_juncbed_best_alignments: THJ_ESTATE
    ctx.juncbed_reset()
    with pytest.raises(host.ThjError, match=r"\(-5\).*best alignments are not being chosen"):
        ctx.juncbed_pair_alignments(True)
    with pytest.raises(host.ThjError, match=r"\(-5\).*inserts are not being graded"):
        ctx.juncbed_add_pairs(L, R)
    # sd 0
    ctx.juncbed_best_alignments(True)
    with pytest.raises(host.ThjError, match=r"\(-1\).*inner_dist_std_dev"):
        ctx.juncbed_pair_alignments(True, 200, 0)
    # what is not built says so
    for other in (lambda: ctx.juncbed_collect_fusions(True), lambda: ctx.juncbed_collect_accepted(True, 0, "", [0, 1])):
        ctx.juncbed_reset()
        ctx.juncbed_best_alignments(True)
        ctx.juncbed_pair_alignments(True)
        with pytest.raises(host.ThjError, match=r"\(-1\).*not built"):
            other()
    # ... in the other call order too: fusions first rule out the single-end switch the pair switch needs; accepted hits first
    ctx.juncbed_reset()
    ctx.juncbed_collect_fusions(True)
    with pytest.raises(host.ThjError, match=r"\(-1\).*not built"):
        ctx.juncbed_best_alignments(True)
    with pytest.raises(host.ThjError, match=r"\(-5\).*best alignments are not being chosen"):
        ctx.juncbed_pair_alignments(True)
    ctx.juncbed_reset()
    ctx.juncbed_best_alignments(True)
    ctx.juncbed_collect_accepted(True, 0, "", [0, 1])
    with pytest.raises(host.ThjError, match=r"\(-1\).*not built"):
        ctx.juncbed_pair_alignments(True)
    # indels are collected beside pairs; a record with an insertion then needs its letters
    ctx.juncbed_reset()
    ctx.juncbed_collect_indels(True)
    ctx.juncbed_best_alignments(True)
    ctx.juncbed_pair_alignments(True)
    x = host.aln_array_from_tuples([pc.X])
    with pytest.raises(host.ThjError, match=r"\(-1\).*thj_juncbed_add_pairs_seq"):
        ctx.juncbed_add_pairs(x, x)
    with pytest.raises(host.ThjError, match=r"\(-1\).*inserted bases"):
        ctx.juncbed_add_pairs_seq(x, ["AC"], x, ["A"])
    assert len(ctx.juncbed_finish(8)) == 0
    ctx.juncbed_reset()
    ctx.juncbed_best_alignments(True)
    ctx.juncbed_pair_alignments(True)
    with pytest.raises(host.ThjError, match=r"\(-1\).*not built"):
        ctx.juncbed_add_span()
    # the other add calls: THJ_ESTATE, nothing counted
    with pytest.raises(host.ThjError, match=r"\(-5\).*thj_juncbed_add_pairs"):
        ctx.juncbed_add_records(L)
    assert len(ctx.juncbed_finish(8)) == 0
    # after the first add: THJ_ESTATE
    ctx.juncbed_add_pairs(L, R)
    with pytest.raises(host.ThjError, match=r"\(-5\).*records were added already"):
        ctx.juncbed_pair_alignments(True)
    assert ir.junc_rows(ctx.juncbed_finish(8)) == c["want_j"]
    # read_idx must not fall within a side and stays below the call's size; nothing is counted
    for bad in ("falls", "large"):
        ctx.juncbed_reset()
        ctx.juncbed_best_alignments(True)
        ctx.juncbed_pair_alignments(True)
        a = L.copy()
        if bad == "falls":
            a["read_idx"][2] = 0
        else:
            a["read_idx"][-1] = len(L) + len(R)
        with pytest.raises(host.ThjError, match=r"\(-1\).*read_idx"):
            ctx.juncbed_add_pairs(a, R)
        assert len(ctx.juncbed_finish(8)) == 0 and ctx.juncbed_pair_counts() == (0, 0, 0, 0, 0)
    # on, then a reset: off again, and a single-end consensus on the same context gives today's rows
    assert run(ctx, c) == c["want_j"]
    recs, reads, AS, mism, anti = pc.as_single(c)
    ctx.juncbed_reset()
    ctx.juncbed_best_alignments(True)
    a = host.aln_array_from_tuples(recs)
    a["AS"], a["read_idx"] = AS, reads
    a["flags"] |= np.array([1 if x else 0 for x in anti], dtype=np.uint8)
    ctx.juncbed_add_records(a)
    single = br.consensus(recs, None, 8, (), None, mism, (20, False, 6), reads, AS, anti)[0]
    assert ir.junc_rows(ctx.juncbed_finish(8)) == single != c["want_j"]
    assert ctx.juncbed_pair_counts() == (0, 0, 0, 0, 0)
    ctx.juncbed_reset()
    ctx.juncbed_add_records(a)
    assert ir.junc_rows(ctx.juncbed_finish(8)) == jr.consensus(recs, None, 8)[0]
    # taken back with the single-end switch
    ctx.juncbed_reset()
    ctx.juncbed_best_alignments(True)
    ctx.juncbed_pair_alignments(True)
    ctx.juncbed_best_alignments(True)
    ctx.juncbed_add_records(a)
    assert ir.junc_rows(ctx.juncbed_finish(8)) == single
