"""Planted contests for stage 1's insertions: two or more reads that report different letters at one (contig, left, length), so that
which read's letters survive is decided by the visiting order alone (std::set<Insertion> compares only the length of the letters,
insertions.h:52-67: the first one inserted stays; all left reads are visited before the right reads).  Plain Python over numpy; it
does not use synth.make_case.  The oracle says what the events are (its insertions are numbered by a counter in visiting order,
batch.merge_events keeps the earlier batch's across batches); this module only says where the contests lie and who comes first.

A read is described in genome orientation ("F"): genome bases, k inserted letters X, genome bases.  An antisense read holds F's
reverse complement and its segment s lies at the far end of F.  The insertion sits inside one segment of a 2L piece (segments
`pair`, `pair + 1` of the read; find_insertions_and_deletions looks at pairs 0 .. nseg - 3 only, segment_juncs.cpp:2856), d bases
from the boundary between the two; that segment is placed ungapped on its longer side with its true Hamming distance as edit_dist,
the other segments lie where the genome says.  Then rh.right - lh.left == 2L - k, simpleSplitAlignment has no error at the true
place, and -- the genome holds G on either side of a contest's place and no contender's letters start or end with G -- an error
at every place before it and in the segment that holds the letters: every contender reports (ref, left of the place, k) with its
own letters, whatever they are.  self_check() asks the oracle, a read at a time.

Every contest is planted at two places with the letters in opposite order: in one the earlier read has the smaller letters (by
alphabet and as the packed 3-bit codes, which weigh the last letter most: the letters here are smaller both ways), in the other
the larger ones.  "The first one visited wins" is the only rule that gets both right.

A read's ordinal is its batch's ordinal_base plus its row, so inside one batch the winner is always the one earliest in memory;
the contests whose winner is neither first nor last in memory have their contenders in several batches, launched in another
order than their ordinals'."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field
from typing import Dict, List, Tuple

import numpy as np

from tophat_amd.batch import build_seg_batch, merge_events
from tophat_amd.params import Params, READ_LEFT, READ_RIGHT

_RC = str.maketrans("ACGTN", "TGCAN")
INS_CODE = "ACGTN"
RIGHT_ORDINAL_BASE = 1 << 28          # segment_juncs_main.cpp: the right side's ordinals start here in a paired run


def revcomp(s: str) -> str:
    return s.translate(_RC)[::-1]


def packed(letters: str) -> int:
    """the letters as the insertion table holds them: 3 bits each, the first one lowest"""
    return sum(INS_CODE.index(c) << (3 * i) for i, c in enumerate(letters))


def smaller(x: str, y: str) -> bool:
    """x before y by alphabet and as packed codes"""
    return x < y and packed(x) < packed(y)


@dataclass
class C:
    """one contender: where it sits (batch, read id) and how its read is laid out"""
    batch: int
    rid: int
    anti: bool = False
    pair: int = 0                   # the read's segments pair, pair + 1 hold the 2L piece
    d: int = 2                      # bases between the insertion and the boundary inside the piece
    where: str = "second"           # the piece's segment (in genome orientation) that holds the letters: "first" or "second"
    nhits: int = 1                  # hits in each of the piece's two segments: the true one and nhits - 1 decoys far off
    true_at: int = 0                # where the true hit stands among them
    dual: bool = False              # the segment that holds the letters is reported twice, placed on either of its sides: with the
                                    # segment behind it as a second piece the read sights its insertion twice (other pair, other hits)


@dataclass
class Contest:
    key: Tuple[int, int, int]                       # (ref_id, left, length)
    contenders: List[Tuple[int, int, str]]          # (batch, read id, letters) in visiting order: the first one wins
    note: str = ""

    @property
    def winner(self) -> str:
        return self.contenders[0][2]


@dataclass
class Batch:
    side: int
    ordinal_base: int
    n_reads: int
    rl: int
    rank: int = 0                                   # the context / rank that runs it
    ins_frac: float = 0.06
    del_frac: float = 0.06
    plan: Dict[int, tuple] = field(default_factory=dict)       # read id -> (sequence, [hits per segment])
    sb: object = None
    recs: list = None
    reads: dict = None


@dataclass
class Scenario:
    name: str
    seqs: List[str]
    L: int
    pkw: dict
    batches: List[Batch]
    contests: List[Contest]
    min_contests: int

    def params(self, bi: int) -> Params:
        return Params(segment_length=self.L, read_side=self.batches[bi].side, **self.pkw)

    def order(self) -> List[int]:
        """the batches in visiting order"""
        return sorted(range(len(self.batches)), key=lambda i: self.batches[i].ordinal_base)

    def one_read(self, bi: int, rid: int):
        b = self.batches[bi]
        return build_seg_batch([[h for h in seg if h[0] == rid] for seg in b.recs], {rid: b.reads[rid]})

    def ordinal(self, bi: int, rid: int) -> int:
        b = self.batches[bi]
        return b.ordinal_base + int(np.searchsorted(b.sb.read_id, rid))


class Builder:
    def __init__(self, name: str, seed: int, L: int = 25, contig_lens=(60000, 40000), **pkw):
        self.name, self.L, self.pkw = name, L, pkw
        self.rng = np.random.default_rng(seed)
        self.g = [[str(c) for c in self.rng.choice(list("ACGT"), size=n)] for n in contig_lens]
        self.at = [1000 for _ in contig_lens]       # the next free place of each contig
        self.turn = 0
        self.sealed = False                         # set by the first filler: the genome does not change any more
        self.batches: List[Batch] = []
        self.contests: List[Contest] = []

    # ---------------------------------------------------------------------------------------------- reads
    def batch(self, side: int, n_reads: int, ordinal_base: int, rl: int = 0, **kw) -> int:
        rl = rl or 4 * self.L
        assert rl % self.L == 0 and rl // self.L >= 3
        self.batches.append(Batch(side, ordinal_base, n_reads, rl, **kw))
        return len(self.batches) - 1

    def _place(self, span: int) -> Tuple[int, int]:
        c = self.turn
        self.turn = (self.turn + 1) % len(self.g)
        gi = self.at[c] + span
        self.at[c] = gi + span
        assert self.at[c] + 1000 < len(self.g[c]), "the genome is too small for the plants"
        return c + 1, gi

    def _segments(self, rl: int, anti: bool):
        L = self.L
        return [((rl - (s + 1) * L, rl - s * L) if anti else (s * L, (s + 1) * L)) for s in range(rl // L)]

    def _read(self, rid, ref, F, lefts, rl, anti, decoys=None):
        """-> (sequence, [hit records of segment s]): segment s of F at lefts[s], its Hamming distance as mismatches and edit_dist"""
        G, L, nseg = self.g[ref - 1], self.L, rl // self.L
        hits = []
        for s, (f0, f1) in enumerate(self._segments(rl, anti)):
            mm = sum(1 for a, b in zip(F[f0:f1], G[lefts[s]:lefts[s] + L]) if a != b or a == "N")
            mine = [(rid, ref, lefts[s], lefts[s] + L, anti, s == nseg - 1, mm, mm, L)]
            for at, extra in (decoys or {}).get(s, ()):
                ham = [sum(1 for a, b in zip(F[f0:f1], G[x:x + L]) if a != b or a == "N") for x in extra]
                mine[at:at] = [(rid, ref, x, x + L, anti, s == nseg - 1, m, m, L) for x, m in zip(extra, ham)]
            hits.append(mine)
        F = "".join(F)
        return (revcomp(F) if anti else F), hits

    def ins_read(self, rid, ref, gi, letters, rl, c: C):
        """the read of layout c whose letters lie between genome bases gi - 1 and gi"""
        G, L, k = self.g[ref - 1], self.L, len(letters)
        nseg = rl // L
        assert 0 <= c.pair <= nseg - 3 and c.d + k <= L
        P0 = (rl - (c.pair + 2) * L) if c.anti else c.pair * L
        p = P0 + L + c.d if c.where == "second" else P0 + L - c.d - k
        gs = gi - p
        F = G[gs:gs + p] + list(letters) + G[gi:gi + rl - p - k]
        lefts, decoys = [], {}
        for s, (f0, f1) in enumerate(self._segments(rl, c.anti)):
            if f1 <= p:
                lefts.append(gs + f0)
            elif f0 >= p + k:
                lefts.append(gs + f0 - k)
            else:
                assert f0 <= p and p + k <= f1
                lefts.append(gs + f0 - k if c.where == "second" else gs + f0)
                if c.dual:      # ... and on its short side, behind the true placement
                    assert c.where == "second" and c.d >= 1 and c.nhits == 1 and f1 + L <= rl and (s >= 1 if c.anti else s + 1 <= nseg - 2)
                    decoys[s] = [(1, [gs + f0])]
            if c.nhits > 1 and f0 in (P0, P0 + L):      # decoys: upstream of the piece's first segment, downstream of its second
                far = [lefts[s] - 300 - 3 * a for a in range(1, c.nhits)] if f0 == P0 else [lefts[s] + 300 + 5 * a for a in range(1, c.nhits)]
                at = min(c.true_at, c.nhits - 1)
                decoys[s] = [(0, far[:at]), (at + 1, far[at:])]
        return self._read(rid, ref, F, lefts, rl, c.anti, decoys)

    def del_read(self, rid, ref, gi, k, rl, anti, pair, d):
        """a read that lacks genome bases gi .. gi + k - 1, d bases into the piece's second segment"""
        G, L = self.g[ref - 1], self.L
        P0 = (rl - (pair + 2) * L) if anti else pair * L
        p = P0 + L + d
        gs = gi - p
        F = G[gs:gs + p] + G[gi + k:gi + k + rl - p]
        lefts = [gs + f0 if f1 <= p else gs + f0 + k for f0, f1 in self._segments(rl, anti)]
        return self._read(rid, ref, F, lefts, rl, anti)

    def plain_read(self, rid, ref, gs, rl, anti):
        G = self.g[ref - 1]
        return self._read(rid, ref, G[gs:gs + rl], [gs + f0 for f0, _ in self._segments(rl, anti)], rl, anti)

    # ---------------------------------------------------------------------------------------------- contests
    def contest(self, letters: List[str], cs: List[C], note: str = "", both_ways: bool = True):
        """cs[i] carries letters[i]; planted once more at another place with the letters in the opposite order, in the reads that
        follow the contenders (read id + 1)"""
        assert not self.sealed, "contests first: their places change the genome"
        k = len(letters[0])
        assert all(len(x) == k for x in letters) and len(set(letters)) == len(letters) == len(cs)
        assert all(x[0] != "G" and x[-1] != "G" for x in letters)
        for way in ((0, 1) if both_ways else (0,)):
            ls = letters[::-1] if way else letters
            rl = max(self.batches[c.batch].rl for c in cs)
            ref, gi = self._place(rl + 30)
            self.g[ref - 1][gi - 1] = self.g[ref - 1][gi] = "G"
            seen = []
            for c, x in zip(cs, ls):
                b = self.batches[c.batch]
                rid = c.rid + way
                assert 1 <= rid <= b.n_reads and rid not in b.plan, "read %d of batch %d is taken" % (rid, c.batch)
                b.plan[rid] = self.ins_read(rid, ref, gi, x, b.rl, c)
                seen.append((b.ordinal_base + rid - 1, c.batch, rid, x))      # (the batches hold read ids 1 .. n: row = id - 1)
            seen.sort()
            self.contests.append(Contest((ref, gi - 1, k), [(bi, rid, x) for _o, bi, rid, x in seen], note + ("/swapped" if way else "")))

    # ---------------------------------------------------------------------------------------------- fillers and the batches
    def build(self, min_contests: int) -> Scenario:
        self.sealed = True
        rng = self.rng
        for b in self.batches:
            nseg = b.rl // self.L
            for rid in range(1, b.n_reads + 1):
                if rid in b.plan:
                    continue
                u, anti = rng.random(), bool(rng.random() < 0.5)
                if u < b.ins_frac + b.del_frac:              # an uncontested indel at a place of its own
                    ref, gi = self._place(20)
                    G = self.g[ref - 1]
                    k, pair, d = int(rng.integers(1, 4)), int(rng.integers(0, nseg - 2)), int(rng.integers(0, 4))
                    if u < b.ins_frac:
                        x = [str(rng.choice([q for q in "ACGT" if q != G[gi]]))] + [str(q) for q in rng.choice(list("ACGT"), size=k - 1)]
                        if x[-1] == G[gi - 1]:
                            x[-1] = next(q for q in "ACGT" if q != G[gi - 1] and (k > 1 or q != G[gi]))
                        c = C(0, rid, anti=anti, pair=pair, d=d, where="second" if rng.random() < 0.5 else "first")
                        b.plan[rid] = self.ins_read(rid, ref, gi, "".join(x), b.rl, c)
                    else:
                        b.plan[rid] = self.del_read(rid, ref, gi, k, b.rl, anti, pair, d + 1)
                else:                                        # a plain exonic read
                    ref = 1 + int(rng.integers(0, len(self.g)))
                    b.plan[rid] = self.plain_read(rid, ref, int(rng.integers(500, len(self.g[ref - 1]) - b.rl - 500)), b.rl, anti)
            nseg = b.rl // self.L
            b.recs = [[h for rid in sorted(b.plan) for h in b.plan[rid][1][s]] for s in range(nseg)]
            b.reads = {rid: b.plan[rid][0] for rid in b.plan}
            b.sb = build_seg_batch(b.recs, b.reads)
            assert b.sb.n_reads == b.n_reads and b.sb.read_id.tolist() == list(range(1, b.n_reads + 1))
        return Scenario(self.name, ["".join(g) for g in self.g], self.L, self.pkw, self.batches, self.contests, min_contests)


def heavy_reads(bd: Builder, bi: int, rids, mh: int = 12):
    """reads with mh hits in their first two segments at intron distance, mh * mh windows each (test_queue_overflow_fallback's): side
    by side in the list of the reads with 9 .. 32 hits they fill a workgroup's task queue, which then runs its tasks un-queued"""
    b = bd.batches[bi]
    L = bd.L
    for rid in rids:
        ref = 1 + rid % len(bd.g)
        gs = int(bd.rng.integers(2000, len(bd.g[ref - 1]) - 3000))
        seq, hits = bd.plain_read(rid, ref, gs, b.rl, False)
        hits[0] = [(rid, ref, gs + 3 * k, gs + 3 * k + L, False, False, 0, 0, L) for k in range(mh)]
        hits[1] = [(rid, ref, gs + 300 + 5 * k, gs + 300 + 5 * k + L, False, False, 0, 0, L) for k in range(mh)]
        hits[2], hits[3] = [], []
        assert rid not in b.plan
        b.plan[rid] = (seq, hits)


# ------------------------------------------------------------------------------------------------ scenarios
def _paths() -> Scenario:
    """one batch of 2 400 reads, L = 25, insertions of up to six letters: every letter count, N, both strands, both segments of the
    piece, both pairs of a four-segment read, reads with one hit a segment (thj_k_sj_flat -> thj_k_sj_tasks) against reads with
    several (8 hits: thj_k_sj_general's first instance; 12 and 24: its second; 42: thj_k_segjuncs_shared), and one among reads that
    fill the task queue.  The contenders lie at both ends of the batch (tiles of 256 reads: other workgroups)."""
    bd = Builder("paths", 11, max_insertion_length=6)
    b = bd.batch(READ_LEFT, 2400, 7)
    lo, hi = iter(range(3, 400, 4)), iter(range(2390, 1900, -4))
    for k, (x, y) in enumerate((("A", "T"), ("AC", "TT"), ("ACA", "TCT"), ("AAAAAA", "TTTTTT"), ("CACTAC", "TTTTTT"), ("AATC", "CCTT"), ("ACTCA", "TATAT"))):
        assert smaller(x, y)
        bd.contest([x, y], [C(b, next(lo), pair=k & 1, d=k % 4, where="second" if k & 2 else "first"),
                            C(b, next(hi), pair=(k >> 1) & 1, d=(k + 1) % 4, where="first" if k & 2 else "second")], "flat/k%d" % len(x))
    for x, y in (("A", "N"), ("AAA", "CNC"), ("CA", "NC"), ("AACAAA", "CNCCNC")):          # (no T beside N: the alphabet has N < T, the codes T < N)
        assert smaller(x, y)
        bd.contest([x, y], [C(b, next(lo), d=1), C(b, next(hi), pair=1, d=3, where="first")], "flat/N")
    for x, y in (("AC", "CT"), ("CTA", "TAC")):
        bd.contest([x, y], [C(b, next(lo), anti=False, pair=1), C(b, next(hi), anti=True, pair=0, d=1)], "flat/forward-antisense")
        bd.contest([x, y], [C(b, next(lo), anti=True, pair=1, where="first"), C(b, next(hi), anti=False, d=0)], "flat/antisense-forward")
        bd.contest([x, y], [C(b, next(lo), anti=True, pair=1, d=3), C(b, next(hi), anti=True, pair=0, where="first")], "flat/antisense-antisense")
    for nh in (4, 6, 12, 21):           # 2 + 2 nh hits a read: 10, 14, 26, 44
        many = dict(nhits=nh, true_at=nh // 2)
        bd.contest(["AT", "CA"], [C(b, next(lo)), C(b, next(hi), pair=1, **many)], "flat-multihit/%d" % nh)
        bd.contest(["CCA", "TAT"], [C(b, next(lo), anti=True, **many), C(b, next(hi))], "multihit-flat/%d" % nh)
        bd.contest(["A", "C"], [C(b, next(lo), true_at=0, nhits=nh), C(b, next(hi), anti=True, true_at=nh, nhits=nh)], "multihit-multihit/%d" % nh)
    bd.contest(["CT", "TA"], [C(b, next(lo), nhits=3, true_at=2), C(b, next(hi), nhits=3, true_at=1)], "multihit-multihit/3")      # 8 hits: the first instance
    # among 70 reads of 144 windows each: the workgroups that take them run un-queued
    heavy_reads(bd, b, range(1000, 1070))
    bd.contest(["ACT", "TCA"], [C(b, 1070, nhits=12, true_at=11), C(b, 2395)], "overflow")
    bd.contest(["CAA", "TAC"], [C(b, 990), C(b, 1072, nhits=12, true_at=3, anti=True)], "overflow")
    # reads that sight their insertion twice, from two pairs of segments (five hits: thj_k_sj_general), first and second in their contests
    bd.contest(["AC", "TA"], [C(b, 800, dual=True), C(b, 1800, anti=True, pair=1, d=1, dual=True)], "sighted twice")
    bd.contest(["CAT", "TCA"], [C(b, 810, anti=True, pair=1, d=3, dual=True), C(b, 1810, where="first")], "sighted twice")
    bd.contest(["C", "T"], [C(b, 820), C(b, 1820, d=1, dual=True)], "sighted twice")
    # three and four reads: the winner's letters are neither the smallest nor the largest
    bd.contest(["CAC", "AAA", "TAT"], [C(b, 500), C(b, 1500, anti=True, pair=1), C(b, 2300, where="first")], "three")
    bd.contest(["CC", "TT", "AA", "AT"], [C(b, 600, nhits=5), C(b, 700), C(b, 1600, anti=True), C(b, 2200, pair=1)], "four")
    return bd.build(2 * 37)


def _wide(L: int) -> Scenario:
    """segment_length 50 and 64: the 2L piece and its letters on 128-bit plane words"""
    bd = Builder("wide%d" % L, 20 + L, L=L, max_insertion_length=6)
    b = bd.batch(READ_LEFT, 1100, 13, rl=4 * L)
    k = 0
    for x, y in (("A", "T"), ("AC", "TT"), ("ACA", "TCT"), ("AAAAAA", "TTTTTT"), ("AAA", "CNC")):
        for anti in ((False, False), (False, True), (True, True)):
            k += 1
            bd.contest([x, y], [C(b, 2 * k + 1, anti=anti[0], pair=k & 1, d=k % 5, where="first" if k & 2 else "second"),
                                C(b, 1100 - 2 * k, anti=anti[1], pair=(k >> 1) & 1, d=(k + 2) % 5, where="second" if k & 4 else "first")], "wide/k%d" % len(x))
    return bd.build(2 * 15)


def _long() -> Scenario:
    """reads of ten segments (250 bases at L = 25: flat_path<16>); the piece at the read's first, middle and last pairs"""
    bd = Builder("long", 31, contig_lens=(90000, 60000))
    b = bd.batch(READ_LEFT, 1000, 9, rl=250)
    k = 0
    for x, y in (("A", "T"), ("AC", "TT"), ("ACA", "TCT"), ("CAC", "CNC")):
        for pa, pb, anti in ((0, 7, False), (7, 3, True), (4, 0, False), (6, 7, True)):
            k += 1
            bd.contest([x, y], [C(b, 2 * k + 1, pair=pa, anti=anti, d=k % 4), C(b, 1000 - 2 * k, pair=pb, anti=bool(not anti and k & 1), where="first", nhits=1 + (k % 3 == 0))],
                       "long/k%d" % len(x))
    return bd.build(2 * 16)


def _sides() -> Scenario:
    """a left and a right batch as one pass: a right read at a low row of its batch against a left read at a high row of its own"""
    bd = Builder("sides", 41)
    le = bd.batch(READ_LEFT, 1500, 5)
    ri = bd.batch(READ_RIGHT, 1400, 5 + 1500)
    for k, (x, y) in enumerate((("A", "T"), ("AC", "TT"), ("ACA", "TCT"), ("CAC", "CNC"))):
        bd.contest([x, y], [C(ri, 2 + 2 * k, anti=bool(k & 1)), C(le, 1490 - 2 * k, pair=1, where="first")], "right-low/left-high")
        bd.contest([x, y], [C(le, 2 + 2 * k, d=k), C(ri, 1390 - 2 * k, anti=True, pair=k & 1)], "left-low/right-high")
    bd.contest(["CA", "AC", "TT"], [C(ri, 20), C(le, 700), C(ri, 1300)], "three")
    return bd.build(2 * 9)


def _shards() -> Scenario:
    """three batches of one side, ordinal_base running on: contenders in the first and the last, and three in an order that no
    launch order of the batches has"""
    bd = Builder("shards", 51)
    s = [bd.batch(READ_LEFT, 1000, 11 + 1000 * i) for i in range(3)]
    for k, (x, y) in enumerate((("A", "T"), ("AC", "TT"), ("ACA", "TCT"), ("AAA", "CNC"))):
        bd.contest([x, y], [C(s[0], 990 - 2 * k, anti=bool(k & 1)), C(s[2], 3 + 2 * k, pair=1)], "first-last")
        bd.contest([x, y], [C(s[2], 980 - 2 * k), C(s[0], 13 + 2 * k, where="first")], "last-first")
    bd.contest(["CAC", "AAA", "TAT"], [C(s[2], 40), C(s[1], 450, anti=True), C(s[2], 900)], "three")       # the winner sits in the middle batch
    bd.contest(["AA", "CC", "TT"], [C(s[1], 30), C(s[0], 450), C(s[2], 950)], "three")             # ... in the first, with the middle letters both times
    return bd.build(2 * 10)


def _growth(replay: bool) -> Scenario:
    """the insertion table (1 024 slots at the least) between two contenders: some 570 insertions in the batch between them -- the table
    passes 40 % and is rehashed into a larger one before the next batch or at the end of the pass -- or, `replay`, 1 000 in the
    second contender's own batch (1 350): the table runs full, the pass fails, and is run again on larger tables"""
    bd = Builder("replay" if replay else "growth", 61 + replay, contig_lens=(80000, 70000))
    if replay:
        bs = [bd.batch(READ_LEFT, 300, 17, ins_frac=0.05), bd.batch(READ_LEFT, 1500, 317, ins_frac=0.9, del_frac=0.02)]
    else:
        bs = [bd.batch(READ_LEFT, 300, 17, ins_frac=0.05), bd.batch(READ_LEFT, 800, 317, ins_frac=0.72, del_frac=0.02), bd.batch(READ_LEFT, 300, 1117, ins_frac=0.05)]
    for k, (x, y) in enumerate((("A", "T"), ("AC", "TT"), ("ACA", "TCT"), ("AAA", "CNC"))):
        bd.contest([x, y], [C(bs[0], 290 - 2 * k, anti=bool(k & 1)), C(bs[-1], (1400 if replay else 3) + 2 * k, pair=1)], "across growth")
        bd.contest([x, y], [C(bs[-1], 250 - 2 * k, where="first"), C(bs[0], 3 + 2 * k)], "across growth")
    return bd.build(2 * 8)


def _ranks() -> Scenario:
    """a paired run sharded by read id over two contexts: rank 0 has the first half of the left and of the right reads, rank 1 the
    second halves; the right side's ordinals start at 2^28"""
    bd = Builder("ranks", 71)
    n = 1000
    l0, l1 = bd.batch(READ_LEFT, n, 3, rank=0), bd.batch(READ_LEFT, n, 3 + n, rank=1)
    r0, r1 = bd.batch(READ_RIGHT, n, RIGHT_ORDINAL_BASE + 3, rank=0), bd.batch(READ_RIGHT, n, RIGHT_ORDINAL_BASE + 3 + n, rank=1)
    for k, (x, y) in enumerate((("A", "T"), ("AC", "TT"), ("ACA", "TCT"), ("CAC", "CNC"))):
        bd.contest([x, y], [C(r0, 4 + 2 * k, anti=bool(k & 1)), C(l1, 990 - 2 * k, pair=1)], "right on rank 0/left on rank 1")
        bd.contest([x, y], [C(l0, 980 - 2 * k), C(l1, 4 + 2 * k, where="first")], "left on rank 0/left on rank 1")
        bd.contest([x, y], [C(l0, 20 + 2 * k, anti=True), C(r1, 900 - 2 * k)], "left on rank 0/right on rank 1")
        bd.contest([x, y], [C(r1, 20 + 2 * k), C(r0, 950 - 2 * k, d=k)], "right on rank 1/right on rank 0")
    bd.contest(["CA", "AC", "TT"], [C(r0, 40), C(l1, 300), C(r1, 800)], "three")
    return bd.build(2 * 17)


def _range() -> Scenario:
    """ordinals just below 2^29 against ordinals from 0 on"""
    bd = Builder("range", 81)
    n = 1000
    lo, hi = bd.batch(READ_LEFT, n, 0), bd.batch(READ_RIGHT, n, (1 << 29) - n - 1)
    for k, (x, y) in enumerate((("A", "T"), ("AC", "TT"), ("ACA", "TCT"))):
        bd.contest([x, y], [C(hi, 2 + 2 * k), C(lo, 990 - 2 * k, anti=bool(k & 1))], "top of the range")
        bd.contest([x, y], [C(lo, 2 + 2 * k), C(hi, 990 - 2 * k, pair=1)], "top of the range")
    return bd.build(2 * 6)


def _stitch() -> Scenario:
    """for stage 2: the letters open the piece's second segment (d = 0), where long_spanning_reads joins two segment hits through
    an insertion of its set; parameters that let a loser's mismatches against the winner's letters through"""
    bd = Builder("stitch", 91, read_mismatches=8, read_edit_dist=10, read_gap_length=6, segment_mismatches=3)
    le, ri = bd.batch(READ_LEFT, 400, 5), bd.batch(READ_RIGHT, 400, 405)
    for k, (x, y) in enumerate((("A", "T"), ("AC", "TT"), ("ACA", "TCT"), ("CAC", "CNC"), ("AAC", "CAC"))):
        bd.contest([x, y], [C(le, 3 + 2 * k, pair=k & 1, d=0), C(le, 390 - 2 * k, anti=True, pair=(k >> 1) & 1, d=0)], "in one batch")
        bd.contest([x, y], [C(ri, 3 + 2 * k, anti=bool(k & 1), d=0), C(le, 370 - 2 * k, pair=1, d=0)], "right-low/left-high")
    return bd.build(2 * 10)


_SCENARIOS = {"paths": _paths, "stitch": _stitch, "wide50": lambda: _wide(50), "wide64": lambda: _wide(64), "long": _long, "sides": _sides, "shards": _shards,
              "growth": lambda: _growth(False), "replay": lambda: _growth(True), "ranks": _ranks, "range": _range}
NAMES = tuple(_SCENARIOS)


@functools.lru_cache(maxsize=None)
def scenario(name: str) -> Scenario:
    """built once a process, shared, never changed"""
    return _SCENARIOS[name]()


@functools.lru_cache(maxsize=None)
def expected(name: str):
    """the oracle's events of the scenario's batches, merged in visiting order (computed once a process)"""
    import orc
    sc = scenario(name)
    g = orc.Genome(sc.seqs)
    want = None
    for bi in sc.order():
        e = orc.segjuncs(sc.params(bi), g, sc.batches[bi].sb)
        want = e if want is None else merge_events(want, e)
    return want


def self_check(sc: Scenario):
    """with the reference alone: every contender, as a batch of one read, reports its contest's (ref, left, length) and nothing else,
    with its own letters; a contest's letters differ; the scenario holds the contests it promises"""
    import orc
    g = orc.Genome(sc.seqs)
    assert len(sc.contests) >= sc.min_contests, "%s: %d contests for %d" % (sc.name, len(sc.contests), sc.min_contests)
    for c in sc.contests:
        assert len(c.contenders) >= 2 and len({x for _b, _r, x in c.contenders}) == len(c.contenders), c
        ords = [sc.ordinal(bi, rid) for bi, rid, _x in c.contenders]
        assert ords == sorted(ords) and len(set(ords)) == len(ords), c
        for (bi, rid, x), o in zip(c.contenders, ords):
            assert o != int(np.searchsorted(sc.batches[bi].sb.read_id, rid)) or sc.batches[bi].ordinal_base == 0, c
            ev = orc.segjuncs(sc.params(bi), g, sc.one_read(bi, rid))
            assert ev.insertions == [(c.key[0], c.key[1], x)] and len(x) == c.key[2], "%s %s: read %d of batch %d reports %r" % (sc.name, c, rid, bi, ev.insertions)


def assert_first_wins(sc: Scenario, ev, what: str = ""):
    """every contest's place carries the letters of the contender visited first"""
    have = {(r, l, len(s)): s for r, l, s in ev.insertions}
    for c in sc.contests:
        assert have.get(c.key) == c.winner, "%s %s %s: %r at %r, the first contender has %r" % (what, sc.name, c.note, have.get(c.key), c.key, c.winner)


def losers_rules(sc: Scenario):
    """what the wrong rules would leave at the contests' places: {rule: number of contests it gets wrong}"""
    out = {"last": 0, "smallest": 0, "largest": 0}
    for c in sc.contests:
        xs = [x for _b, _r, x in c.contenders]
        out["last"] += xs[-1] != c.winner
        out["smallest"] += min(xs, key=packed) != c.winner
        out["largest"] += max(xs, key=packed) != c.winner
    return out


def span_batch(sc: Scenario, bi: int):
    """the batch's reads as long_spanning_reads takes them: the same segment hits, ungapped, with their mismatches"""
    from tophat_amd.batch import build_span_batch
    b = sc.batches[bi]
    return build_span_batch(b.recs, b.reads, {rid: "I" * len(s) for rid, s in b.reads.items()})


def write_files(sc: Scenario, d: str, left: int = 0, right: int = 1):
    """batches `left` and `right` as the files the executables take (synth.write_case's layout; the SAM lines as make_case's emit
    writes them); no full-read maps: the mate of a read is its partner's last segment"""
    from types import SimpleNamespace
    from tophat_amd.samtext import md_nm
    from tophat_amd.synth import write_case
    names = ["chr%d" % (i + 1) for i in range(len(sc.seqs))]
    case = SimpleNamespace(names=names, seqs=sc.seqs, reads={}, quals={}, seg_sam={}, full_sam={}, spliced_sam={}, juncdb={})
    for sd, bi in (("left", left), ("right", right)):
        b = sc.batches[bi]
        nseg = b.rl // sc.L
        case.reads[sd] = dict(b.reads)
        case.quals[sd] = {rid: "I" * len(s) for rid, s in b.reads.items()}
        case.full_sam[sd] = []
        case.seg_sam[sd] = [[] for _ in range(nseg)]
        for rid in sorted(b.plan):
            seq, hits = b.plan[rid]
            for s in range(nseg):
                for (_r, ref, lf, rt, anti, _e, _mm, _ed, _l) in hits[s]:
                    piece = (revcomp(seq) if anti else seq)[(b.rl - (s + 1) * sc.L if anti else s * sc.L):][:sc.L]
                    nm, md = md_nm(sc.seqs[ref - 1][lf:rt], piece)
                    case.seg_sam[sd][s].append("%d|%d:%d:%d\t%d\t%s\t%d\t255\t%dM\t*\t0\t0\t%s\t%s\tNM:i:%d\tMD:Z:%s\n" % (
                        rid, s * sc.L, s, nseg, 16 if anti else 0, names[ref - 1], lf + 1, rt - lf, piece, "I" * (rt - lf), nm, md))
    return write_case(case, d), names


def check_stage2(sc: Scenario, sbs, recs, p, g, juncs, ins) -> int:
    """recs[i] = the spanning records of sbs[i] (the batches in visiting order) with stage 1's sets.  long_spanning_reads joins two
    segments through an insertion of its set only where the read's bases equal the set's letters (long_spanning_reads.cpp:1010-1306;
    an N never equals): the winner of a contest has one alignment through the insertion, a loser has none -- and would have one had
    its own letters won, which the oracle is asked per loser.  -> the number of losers checked that way"""
    import orc
    through = lambda rs, row: [a for a in rs if a.read_idx == row and any((q >> 28) == 3 for q in a.cigar)]      # noqa: E731
    n_losers = 0
    for c in sc.contests:
        for k, (bi, rid, x) in enumerate(c.contenders):
            at = sc.order().index(bi)
            row = sbs[at].read_id.tolist().index(rid)
            if "N" in x:
                assert not through(recs[at], row), (c, rid)
            elif k == 0:
                assert len(through(recs[at], row)) == 1, (c, rid)
            else:
                own = [(r, l, x if (r, l, len(s)) == c.key else s) for r, l, s in ins]
                assert not through(recs[at], row), (c, rid)
                assert len(through(orc.spanning(p, g, sbs[at], juncs, own), row)) == 1, (c, rid)
                n_losers += 1
    return n_losers
