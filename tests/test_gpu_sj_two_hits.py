"""GPU: stage 1's reads of at most two hits a segment (class GEN_TWO of thj_k_sj_flat's list, the first pass of thj_k_sj_general's sliced
instance: flat2_read, a thread a read) against the oracle -- junctions, deletions, insertions with their letters, and the counters.
Planted batches: a workgroup's slice is what its tile of 256 consecutive reads lists, so the tiles hold 1, 255, 256 and no read of the
class, the same mixed with reads of the other classes in interleaved order, and (a batch of 2 048 tiles, all but two of them reads
without a hit: workgroup 0 takes the first and the last) 257.  Kinds of read: two abutting copies (nothing to do); a contiguous decoy
copy first and a spliced or a deletion copy second, so that the second hit of a segment alone gives the window or the indel pair; two
copies that take the mate-anchored rescue; one hit a segment with three mate hits; reads of three, twelve and forty hits a segment for
the other classes.  Batches of 2, 3 and 4 segments take the new pass, one of 5 segments today's.  The contested insertions are
tests/ins_conflicts.py's, sighted from the second of two hits."""
import numpy as np
import pytest

import ins_conflicts as ic
import orc
from tophat_amd import host
from tophat_amd.batch import HIT_DTYPE, SegBatch
from tophat_amd.params import Params, READ_LEFT
from util import assert_events_equal

pytestmark = pytest.mark.gpu
L = 25
SPAN = 1500            # genome bases a read has to itself
INTRON = 200


@pytest.fixture(scope="module")
def lib():
    return host.load_lib()   # fails loudly when the extension is missing


def make_batch(kinds, nseg, seed=7, empty_between=None):
    """kinds[r] = the kind of read r; empty_between = (at, count): that many reads without a hit behind read `at`"""
    rng = np.random.default_rng(seed)
    rl = nseg * L
    g = rng.choice(list("ACGT"), size=2000 + SPAN * len(kinds))
    hits, seg_off, reads, mate_off, mate_hits = [], [0], [], [0], []

    def end(s):
        return 2 if s == nseg - 1 else 0

    for r, kind in enumerate(kinds):
        A = 1000 + r * SPAN           # copy A: contiguous
        B = A + 600                   # copy B
        per_seg = [[] for _ in range(nseg)]
        seq = g[A:A + rl]
        mates = []
        if kind == "flat":
            for s in range(nseg):
                per_seg[s] = [(1, A + s * L, A + (s + 1) * L, end(s), 0, 0, L)]
        elif kind == "two":
            g[B:B + rl] = g[A:A + rl]
            for s in range(nseg):
                per_seg[s] = [(1, x + s * L, x + (s + 1) * L, end(s), 0, 0, L) for x in (A, B)]
        elif kind == "two_win":       # copy B is spliced behind its first segment: the window comes from the second hit of segment 0
            g[B + L:B + L + 2] = list("GT")
            g[B + L + INTRON - 2:B + L + INTRON] = list("AG")
            seq = np.concatenate([g[B:B + L], g[B + L + INTRON:B + INTRON + rl]])
            g[A:A + rl] = seq
            for s in range(nseg):
                b = B + s * L + (INTRON if s else 0)
                per_seg[s] = [(1, A + s * L, A + (s + 1) * L, end(s), 0, 0, L), (1, b, b + L, end(s), 0, 0, L)]
        elif kind == "two_del":       # copy B lacks two genome bases five bases into its second segment
            seq = np.concatenate([g[B:B + L + 5], g[B + L + 7:B + rl + 2]])
            g[A:A + rl] = seq
            for s in range(nseg):             # (the second segment stands on its longer side, its Hamming distance as edit_dist)
                b = B + s * L + (2 if s else 0)
                mm = int(np.sum(seq[s * L:(s + 1) * L] != g[b:b + L]))
                per_seg[s] = [(1, A + s * L, A + (s + 1) * L, end(s), 0, 0, L), (1, b, b + L, end(s), mm, mm, L)]
        elif kind in ("two_resc", "flat_m3"):      # the last segment lies behind an intron and has no hit: the mate hits anchor the rescue
            seq = np.concatenate([g[B:B + rl - L], g[B + rl - L + INTRON:B + rl + INTRON]])
            if kind == "two_resc":
                g[A:A + rl - L] = g[B:B + rl - L]
            for s in range(nseg - 1):
                per_seg[s] = [(1, x + s * L, x + (s + 1) * L, 0, 0, 0, L) for x in ((A, B) if kind == "two_resc" else (B,))]
            m = B + rl + INTRON + 30
            mates = [(1, m + 11 * k, m + 11 * k + 100, 1 | 2, 0, 0, 100) for k in range(2 if kind == "two_resc" else 3)]
        else:                         # "three", "mid", "many": several hits in the first two segments at intron distance, windows for every pair
            mh = {"three": 3, "mid": 12, "many": 40}[kind]
            per_seg[0] = [(1, A + 3 * k, A + 3 * k + L, 0, 0, 0, L) for k in range(mh)]
            per_seg[1] = [(1, A + 300 + 5 * k, A + 300 + 5 * k + L, end(1), 0, 0, L) for k in range(mh)]
        for s in range(nseg):
            hits += per_seg[s]
            seg_off.append(len(hits))
        mate_hits += mates
        mate_off.append(len(mate_hits))
        reads.append("".join(seq))
    seqg = "".join(g)
    n = len(kinds)
    seg_off = np.array(seg_off, dtype=np.uint32)
    mate_off = np.array(mate_off, dtype=np.uint32)
    lens = np.full(n, rl, dtype=np.int64)
    bases = np.frombuffer("".join(reads).encode(), dtype=np.uint8).copy()
    if empty_between:
        at, count = empty_between
        seg_off = np.concatenate([seg_off[:(at + 1) * nseg + 1], np.full(count * nseg, seg_off[(at + 1) * nseg], dtype=np.uint32), seg_off[(at + 1) * nseg + 1:]])
        mate_off = np.concatenate([mate_off[:at + 2], np.full(count, mate_off[at + 1], dtype=np.uint32), mate_off[at + 2:]])
        bases = np.concatenate([bases[:(at + 1) * rl], np.zeros(count * L, dtype=np.uint8) + ord("A"), bases[(at + 1) * rl:]])
        lens = np.concatenate([lens[:at + 1], np.full(count, L, dtype=np.int64), lens[at + 1:]])
        n += count
    read_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    b = SegBatch(nseg, np.arange(1, n + 1, dtype=np.uint32), read_off, bases, seg_off, np.array(hits, dtype=HIT_DTYPE),
                 mate_off, np.array(mate_hits, dtype=HIT_DTYPE))
    return seqg, b


def check(seqg, b, what, p=None):
    p = p or Params(read_side=READ_LEFT, inner_dist_mean=50, inner_dist_std_dev=20)
    want = orc.segjuncs(p, orc.Genome([seqg]), b)
    with host.Context(0) as ctx:
        ctx.upload_genome(host.pack_genome([seqg]))
        got = ctx.segjuncs([(p, ctx.upload_batch(b))])
    print(what, {k: got.stats[k] for k in ("windows", "indel_pairs", "rescue_pairs", "overflow_blocks")}, len(want.juncs), len(want.deletions), len(want.insertions))
    assert_events_equal(got, want, what)
    for k in ("windows", "indel_pairs", "rescue_pairs"):
        assert got.stats[k] == want.stats[k], (what, k)
    return want


TWO_KINDS = ("two", "two_win", "two_del", "two_resc", "flat_m3")


def tiles():
    """eight tiles of 256 reads: 1, 255, 256 and no read of the class among flat reads; the same counts of mixed kinds of the class
    among reads of the other classes, interleaved; a tile of the class alone, every kind in turn"""
    mixed = lambda k: TWO_KINDS[k % len(TWO_KINDS)]       # noqa: E731
    other = lambda k: ("flat", "three", "mid", "flat", "many", "three")[k % 6]      # noqa: E731
    t = [["two_win"] + ["flat"] * 255, ["two"] * 100 + ["flat"] + ["two_del"] * 155, ["two"] * 256, ["flat"] * 200 + ["three"] * 56]
    t.append([other(k) if k != 77 else "two_del" for k in range(256)])                          # 1 among the other classes
    t.append([mixed(k) if k != 130 else "mid" for k in range(256)])                             # 255
    t.append([mixed(k) for k in range(256)])                                                   # 256, every kind
    t.append([mixed(k) if k % 2 else other(k) for k in range(256)])                             # interleaved
    return [k for tile in t for k in tile]


def test_round_edges_and_mixed_classes(lib):
    kinds = tiles()
    seqg, b = make_batch(kinds, 4)
    assert b.n_reads == 2048
    want = check(seqg, b, "tiles")
    n_win, n_del, n_resc = kinds.count("two_win"), kinds.count("two_del"), kinds.count("two_resc") + kinds.count("flat_m3")
    assert n_win > 100 and n_del > 100 and n_resc > 100
    assert len(want.juncs) >= n_win and len(want.deletions) >= n_del and want.stats["rescue_pairs"] >= n_resc


def test_slice_of_257(lib):
    """2 048 tiles: workgroup 0 of 2 047 takes the first and the last -- 256 reads of the class and one more"""
    kinds = [TWO_KINDS[k % 3] for k in range(256)] + ["two_win"]
    seqg, b = make_batch(kinds, 4, seed=9, empty_between=(255, 2047 * 256 - 256))
    assert b.n_reads == 2047 * 256 + 1
    want = check(seqg, b, "slice of 257")
    assert len(want.juncs) >= 80 and len(want.deletions) >= 80


@pytest.mark.parametrize("nseg", [2, 3, 4, 5])
def test_segments_per_read(lib, nseg):
    """2, 3 and 4 segments take the first pass, 5 today's path"""
    kinds = [(TWO_KINDS + ("flat", "three"))[k % 7] for k in range(700)]
    seqg, b = make_batch(kinds, nseg, seed=10 + nseg)
    want = check(seqg, b, "nseg %d" % nseg)
    assert len(want.juncs) >= 100
    if nseg <= 4:                     # (with five segments the first and the fourth lie 2L = min_segment_intron apart: a partner, no rescue)
        assert want.stats["rescue_pairs"] > 0
    if nseg >= 3:
        assert len(want.deletions) >= 90


def contested():
    """ins_conflicts' contests with two hits in each of the piece's segments, the true one second: both contenders are reads of the
    class, and each contest is planted at two places with the letters in opposite order"""
    bd = ic.Builder("two_hits", 151, max_insertion_length=6)
    b = bd.batch(READ_LEFT, 1200, 7)
    lo, hi = iter(range(3, 400, 4)), iter(range(1190, 800, -4))
    two = dict(nhits=2, true_at=1)
    for k, (x, y) in enumerate((("A", "T"), ("AC", "TT"), ("ACA", "TCT"), ("AAAAAA", "TTTTTT"), ("CAC", "CNC"))):
        bd.contest([x, y], [ic.C(b, next(lo), pair=k & 1, d=k % 4, **two), ic.C(b, next(hi), anti=bool(k & 1), pair=(k >> 1) & 1, d=(k + 1) % 4, **two)], "two hits/k%d" % len(x))
        bd.contest([x, y], [ic.C(b, next(lo), anti=True, **two), ic.C(b, next(hi), where="first")], "two hits against flat")
    return bd.build(2 * 10)


def test_contested_insertions_from_the_second_hit(lib):
    sc = contested()
    assert len(sc.contests) >= sc.min_contests
    g = orc.Genome(sc.seqs)
    want = orc.segjuncs(sc.params(0), g, sc.batches[0].sb)
    ic.assert_first_wins(sc, want, "oracle")
    with host.Context(0) as ctx:
        ctx.upload_genome(host.pack_genome(sc.seqs))
        got = ctx.segjuncs([(sc.params(0), ctx.upload_batch(sc.batches[0].sb, ordinal_base=sc.batches[0].ordinal_base))])
    assert_events_equal(got, want, "contests")
    ic.assert_first_wins(sc, got, "two hits a segment")
    assert got.stats["indel_pairs"] == want.stats["indel_pairs"] and got.stats["windows"] == want.stats["windows"]
