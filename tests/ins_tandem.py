"""Planted self-contests for stage 1's insertions: ONE read that reports the same (contig, left, length) twice with different
letters, so that which letters survive is decided by the order in which find_insertions_and_deletions visits the read's own hit
pairs (segment_juncs.cpp:2856-2940: the segment pair i outermost, then the hit li of segment i, then the hit ri of segment i + 1;
std::set<Insertion> keeps the first one inserted).  The device restates that order in the low 16 bits of ins_prio(ordinal, i, li,
ri); tests/ins_conflicts.py pins the ordinal above them, this module what lies below.  Plain Python over numpy beside
ins_conflicts.py, whose Builder, fillers and file writer it uses.

A *sighting* is one (segment pair, hit of its first segment, hit of its second) of a read that reports an insertion.  Two sightings
of one read bring different letters to one place only where its hits lie on different diagonals: inside a tandem repeat, where a
segment also aligns one period further on.  The raw material is found by a seeded search over periodic patches (`_candidate`: a
patch of period 1 .. 6 with one to three point mutations, a read piece G[a:a+q] + X + G[a+q:], diagonal A at the true place and
diagonal B one period off) that a restatement of simpleSplitAlignment / detect_small_insertion (`sightings`) sieves; the seeds that
passed are fixed below (RAW_SEEDS; `python tests/ins_tandem.py search`, with the repository's root on PYTHONPATH, prints them), so building a scenario searches nothing.  The
restatement only proposes: self_check() asks the oracle, a read at a time, whether each sighting alone reports what the plant
says, and whether the read with both reports the letters of the one visited first.

Everything is described in genome orientation: the piece P (2L bases, or 3L for a contest across two segment pairs), the hits of
its segments g0, g1 (, g2).  A forward read's segments i, i + 1 are g0, g1; an antisense read holds the reverse complement, its
segment i is the piece's LAST one, and the reference swaps lh / rh only after the indices are fixed (:2914-2920) -- li stays the
index in segment i's list, which then is the list of the genomic right hits.

  same pair     g0 has hits at a and a + s, g1 hits that end at e and e + s (s = one period, either way): the sightings are
                (a, e) and (a + s, e + s).  Where each hit stands in its list is the layout: ((li, ri) of the sighting visited first,
                (li, ri) of the other); "two diagonals" has the lists in step ((0,0) and (1,1)), "crossed" has them crossed ((0,1) and
                (1,0): li says one order, ri the other).
  across pairs  g1 has two hits; the pair (g0, g1) is on one diagonal and (g1, g2) on the other.

Two sightings of ONE pair that share a hit cannot contest: with the same hit of one segment the place and the length fix the other
hit.  So li always differs between them, ri never decides on its own, and what the ri field can spoil is li (a field too narrow
lets a high ri run into li's bits; li and ri swapped); the layouts are chosen for that."""
from __future__ import annotations

import functools
import random
import sys
from dataclasses import dataclass, field
from typing import Dict, List, Tuple

import ins_conflicts as ic
from ins_conflicts import Builder, packed, revcomp, smaller, write_files, span_batch      # noqa: F401  (write_files, span_batch: for the tests)
from tophat_amd.batch import build_seg_batch, merge_events
from tophat_amd.params import READ_LEFT, READ_RIGHT


# ------------------------------------------------------------------------------------------------ the restatement
def _split(shorter: str, left_ref: str, right_ref: str):
    """simpleSplitAlignment (segment_juncs.cpp:2390-2456): -> (first best position, its errors)"""
    n = len(shorter)
    before = [0] * (n + 1)
    for k in range(n - 1, -1, -1):
        before[k] = before[k + 1] + (right_ref[k] != shorter[k] or shorter[k] == "N")
    best, best_pos, after = n + 1, -1, 0
    for pos in range(1, n):
        after += (left_ref[pos - 1] != shorter[pos - 1] or shorter[pos - 1] == "N")
        if before[pos] + after < best:
            best, best_pos = before[pos] + after, pos
    return best_pos, best


def _insertion(G: str, mod: str, lh, rh):
    """detect_small_insertion (:2470-2543) for the piece `mod` in genome orientation; lh, rh = (left, right, edit_dist) of hits of L
    bases whose lengths sum to the piece's -> (left, letters) or None"""
    plen = len(mod)
    glen = rh[1] - lh[0]
    disc = plen - glen
    if lh[0] < 0 or glen < 2 or disc <= 0:
        return None
    pos, err = _split(G[lh[0]:rh[1]], mod[:glen], mod[plen - glen:])
    if pos < 0 or err > lh[2] + rh[2] - 1 or pos + disc > glen:
        return None
    return lh[0] + pos - 1, mod[pos:pos + disc]


def sightings(seqs, L: int, max_ins: int, seq: str, hits) -> List[tuple]:
    """find_insertions_and_deletions' visits of one read that report an insertion, in visiting order:
    [(i, li, ri, ref, left, letters)]; hits[s] = the hit records of segment s in list order"""
    out = []
    nseg = len(hits)
    for i in range(nseg - 2):
        if not hits[i] or not hits[i + 1]:
            break
        full = seq[i * L:i * L + 2 * L]
        for li, a in enumerate(hits[i]):
            for ri, b in enumerate(hits[i + 1]):
                if a[1] != b[1] or a[4] != b[4]:
                    continue
                lh, rh, mod = (b, a, revcomp(full)) if a[4] else (a, b, full)
                disc = rh[3] - lh[2] - len(full)
                if not (-max_ins <= disc < 0):
                    continue
                got = _insertion(seqs[a[1] - 1], mod, (lh[2], lh[3], lh[7]), (rh[2], rh[3], rh[7]))
                if got:
                    out.append((i, li, ri, a[1], got[0], got[1]))
    return out


def _ham(x, y) -> int:
    return sum(1 for p, q in zip(x, y) if p != q or p == "N")


# ------------------------------------------------------------------------------------------------ raw material
MAX_INS = 6                         # every scenario here runs with max_insertion_length = 6 (the default is 3)


@dataclass(frozen=True)
class Raw:
    """a piece and its hits in genome orientation, coordinates inside the patch T (random flanks of 2L + 10 bases around the
    periodic core, so that every hit of a read's neighbouring segments lies inside T too)"""
    kind: str                       # "same" or "across"
    k: int
    L: int
    T: str
    a: int                          # where the piece starts on diagonal A
    P: str
    A: Tuple[int, int]              # diagonal A's sighting: the lefts of its two hits
    B: Tuple[int, int]
    gA: int                         # the piece's segment that holds A's first hit (0; 1: the second pair of an across piece)
    gB: int
    left: int                       # the place both report
    XA: str
    XB: str

    def lists(self, only: str = ""):
        """the hits (lefts) of the piece's segments; `only` = "A" / "B": that sighting's two segments hold nothing but its hits"""
        out = [[] for _ in range(len(self.P) // self.L)]
        for name, (l, r), g in (("A", self.A, self.gA), ("B", self.B, self.gB)):
            out[g].append((name, l))
            out[g + 1].append((name, r))
        if only:
            g = self.gA if only == "A" else self.gB
            for s in (g, g + 1):
                out[s] = [x for x in out[s] if x[0] == only]
        return out


def _mini(raw: Raw, only: str = ""):
    """the piece with a segment before it and two behind as a forward read on T -> its sightings"""
    T, L, a = raw.T, raw.L, raw.a
    tail = a + len(raw.P) - raw.k
    seq = T[a - L:a] + raw.P + T[tail:tail + 2 * L]
    lefts = [[a - L]] + [[l for _n, l in x] for x in raw.lists(only)] + [[tail], [tail + L]]
    hits = []
    for s, ls in enumerate(lefts):
        hits.append([])
        for l in ls:
            m = _ham(seq[s * L:(s + 1) * L], T[l:l + L])
            hits[s].append((1, 1, l, l + L, False, False, m, m, L))
    return sightings([T], L, MAX_INS, seq, hits)


def _candidate(seed: int, kind: str, k: int, L: int):
    """one try of the search -> Raw or None"""
    rnd = random.Random("%s/%d/%d/%d" % (kind, k, L, seed))
    p = rnd.randint(1, 6)
    unit = "".join(rnd.choice("ACGT") for _ in range(p))
    nP = (3 if kind == "across" else 2) * L
    n, fl = nP + 44, 2 * L + 10
    T = list((unit * (n // p + 1))[:n])
    for _ in range(rnd.randint(1, 3)):
        at = rnd.randrange(n)
        T[at] = rnd.choice([c for c in "ACGT" if c != T[at]])
    T = "".join([rnd.choice("ACGT") for _ in range(fl)] + T + [rnd.choice("ACGT") for _ in range(fl)])
    a = fl + rnd.randint(p + 8, n - nP - p - 8 + k)
    q = rnd.randint(L, 2 * L - k) if kind == "across" else rnd.randint(1, 2 * L - k - 1)
    X = list(T[a + q - k:a + q] if rnd.random() < 0.5 else T[a + q:a + q + k])
    if rnd.random() < 0.75:
        at = rnd.randrange(k)
        X[at] = rnd.choice([c for c in "ACGT" if c != X[at]])
    P = T[a:a + q] + "".join(X) + T[a + q:a + nP - k]
    s = p if rnd.random() < 0.5 else -p
    swap = rnd.random() < 0.5               # across: which pair lies on diagonal A
    if kind == "same":
        A, B, gA, gB = (a, a + L - k), (a + s, a + L - k + s), 0, 0
    else:
        # the pair (g0, g1): g0 on its diagonal, g1 set to its right end; the pair (g1, g2): g1 on g0's diagonal, g2 behind the letters
        first, second = (a, a + L - k), (a + L, a + 2 * L - k)
        if swap:
            A, B, gA, gB = second, (first[0] + s, first[1] + s), 1, 0
        else:
            A, B, gA, gB = first, (second[0] + s, second[1] + s), 0, 1
    out = []
    for (l, r), g in ((A, gA), (B, gB)):            # the cheap sieve: each sighting on its own piece
        piece = P[g * L:g * L + 2 * L]
        hl, hr = _ham(piece[:L], T[l:l + L]), _ham(piece[L:], T[r:r + L])
        if hl > 2 or hr > 2:
            return None
        got = _insertion(T, piece, (l, l + L, hl), (r, r + L, hr))
        if not got or len(got[1]) != k:
            return None
        out.append(got)
    (left, XA), (leftB, XB) = out
    if left != leftB or not (smaller(XA, XB) or smaller(XB, XA)):
        return None
    raw = Raw(kind, k, L, T, a, P, A, B, gA, gB, left, XA, XB)
    # ... then the read around it: each sighting alone reports its letters at the place and nothing else, both together exactly two
    # sightings at the place
    if [x[4:] for x in _mini(raw, "A")] != [(left, XA)] or [x[4:] for x in _mini(raw, "B")] != [(left, XB)]:
        return None
    both = [x[5] for x in _mini(raw) if x[4] == left and len(x[5]) == k]
    if sorted(both) != sorted((XA, XB)):
        return None
    return raw


def first_smaller(raw: Raw) -> bool:
    """across pairs: has the sighting of the genomic first pair (a forward read's pair i) the smaller letters"""
    first, other = (raw.XA, raw.XB) if raw.gA <= raw.gB else (raw.XB, raw.XA)
    return smaller(first, other)


def search(kind: str, k: int, L: int, want: int, tries: int = 600000, ordered=None):
    """-> the seeds of the first `want` tries that pass (`ordered`: only those with that first_smaller)"""
    found = []
    for seed in range(tries):
        r = _candidate(seed, kind, k, L)
        if r is not None and (ordered is None or first_smaller(r) == ordered):
            found.append(seed)
            if len(found) == want:
                break
    return found


# (kind, k, L, first_smaller or None) -> seeds of _candidate that pass; printed by `python tests/ins_tandem.py search`
RAW_SEEDS: Dict[tuple, List[int]] = {
    ('same', 1, 25, None): [68493, 83177, 367350, 501323],
    ('same', 2, 25, None): [11459, 130957, 175491],
    ('same', 3, 25, None): [10868, 30677, 120620, 138822],
    ('same', 6, 25, None): [90835, 104222, 106551, 117185],
    ('same', 1, 50, None): [638964],
    ('same', 2, 50, None): [79987],
    ('same', 3, 50, None): [37297, 209471],
    ('same', 6, 50, None): [23029, 31799],
    ('across', 1, 25, True): [1985, 7253, 12727, 99404],
    ('across', 1, 25, False): [3025, 27584, 28859, 29430],
    ('across', 2, 25, True): [4461, 8283, 18891, 23000],
    ('across', 2, 25, False): [1987, 13528, 20598, 30095],
    ('across', 3, 25, True): [5489, 24662, 28176, 32386],
    ('across', 3, 25, False): [16884, 27459, 35491, 36189],
    ('across', 6, 25, True): [3161, 11116, 14550, 15564],
    ('across', 6, 25, False): [13267, 14665, 27207, 35277],
    ('across', 1, 50, True): [51700, 99937],
    ('across', 1, 50, False): [3903, 63486],
    ('across', 2, 50, True): [12070, 27244],
    ('across', 2, 50, False): [48743, 58100],
    ('across', 3, 50, True): [5530, 47559],
    ('across', 3, 50, False): [11977, 35701],
    ('across', 6, 50, True): [2669, 13433],
    ('across', 6, 50, False): [757, 1479],
}


@functools.lru_cache(maxsize=None)
def raw(kind: str, k: int, L: int, ordered, n: int) -> Raw:
    r = _candidate(RAW_SEEDS[(kind, k, L, ordered)][n], kind, k, L)
    assert r is not None and (ordered is None or first_smaller(r) == ordered), "seed %d of %r gives no contest any more" % (n, (kind, k, L, ordered))
    return r


# ------------------------------------------------------------------------------------------------ plants
@dataclass
class Contest:
    key: Tuple[int, int, int]                       # (ref_id, left, length)
    batch: int
    rid: int
    sights: List[Tuple[int, int, int, str]]         # the read's sightings at the key, (i, li, ri, letters), in visiting order
    note: str                                       # kind/layout/polarity/...
    others: List[Tuple[int, int, str]] = field(default_factory=list)       # (batch, read id, letters) of other reads at the key
    winner: str = ""                                # the letters that stay (the first sighting's, unless an earlier read claims the key)
    alone: list = field(default_factory=list)       # per sighting: (the hit records of the read with that sighting alone, letters)
    site: tuple = None                              # (ref_id, where the patch starts)

    @property
    def first(self) -> str:
        return self.sights[0][3]


class TBuilder(Builder):
    def site(self, r: Raw, rl: int, n_decoys: int = 0):
        """room for a read around r's patch and its decoys; the patch goes into the genome -> (ref, where T starts)"""
        assert not self.sealed
        c = self.turn
        self.turn = (self.turn + 1) % len(self.g)
        before, after = rl + (1100 + 3 * n_decoys if n_decoys else 0), len(r.T) - r.a + rl + (350 + 5 * n_decoys if n_decoys else 0)
        t0 = self.at[c] + before
        self.at[c] = t0 + r.a + after
        assert self.at[c] + 1000 < len(self.g[c]), "the genome is too small for the plants"
        self.g[c][t0:t0 + len(r.T)] = list(r.T)
        return c + 1, t0

    def tandem_read(self, bi: int, rid: int, r: Raw, anti: bool, pair: int, slots, first: str = "", pad: int = 0, only: str = "", site=None, note: str = ""):
        """the read of batch bi whose segments pair .. hold r's piece.  slots = ((li, ri) of the sighting visited first, (li, ri) of
        the other) in the read's own terms; `first` = "A" / "B" says which sighting is visited first in a same-pair contest (across
        pairs the strand says it).  The lists are filled up with decoys, `pad` more of them behind the piece's first segment's.
        only = "A" / "B": a read with that sighting's hits alone (no contest: another read of a mixed one), at an earlier read's `site`"""
        b = self.batches[bi]
        L, rl = self.L, b.rl
        nseg, nP = rl // L, len(r.P) // L
        assert r.L == L and 0 <= pair and pair + nP - 2 <= nseg - 3 and rid not in b.plan and 1 <= rid <= b.n_reads
        assert not only or r.kind == "same"
        rseg = lambda g: pair + (nP - 1 - g if anti else g)      # noqa: E731  the read's segment that is the piece's segment g
        if r.kind == "across":
            first = ("A" if r.gA == 0 else "B") if not anti else ("A" if r.gA == 1 else "B")
        order = [only] if only else [first, "B" if first == "A" else "A"]
        # where every planted hit stands: lists[g][index] = left inside T
        lists = [dict() for _ in range(nP)]
        expect = []
        for name, (li, ri) in zip(order, slots):
            (x0, x1), g = (r.A, r.gA) if name == "A" else (r.B, r.gB)
            for gg, x, at in ((g, x0, ri if anti else li), (g + 1, x1, li if anti else ri)):
                assert lists[gg].get(at, x) == x, "two hits for one place of a list"
                lists[gg][at] = x
            expect.append((rseg(g + 1) if anti else rseg(g), li, ri, r.XA if name == "A" else r.XB))
        sizes = [max(lists[g]) + 1 + (pad if g == 0 else 0) for g in range(nP)]
        ref, t0 = site or self.site(r, rl, sum(sizes) - sum(len(x) for x in lists))
        G = self.g[ref - 1]
        P0 = (rl - (pair + nP) * L) if anti else pair * L
        gi = t0 + r.a
        tail = gi + len(r.P) - r.k
        F = G[gi - P0:gi] + list(r.P) + G[tail:tail + rl - P0 - len(r.P)]
        assert len(F) == rl
        n_dec = 0
        hits = []
        for s, (f0, f1) in enumerate(self._segments(rl, anti)):
            if f1 <= P0:
                lefts = [(gi - P0 + f0, False)]
            elif f0 >= P0 + len(r.P):
                lefts = [(tail + f0 - P0 - len(r.P), False)]
            else:
                g = (f0 - P0) // L
                lefts = []
                for at in range(sizes[g]):
                    if at in lists[g]:
                        lefts.append((t0 + lists[g][at], True))
                    else:           # a decoy: far before the piece (its first segment; further off: a middle one), far behind it (its last)
                        n_dec += 1
                        lefts.append((gi - 300 - 3 * n_dec if g == 0 else tail + 300 + 5 * n_dec if g == nP - 1 else gi - 1100 - 3 * n_dec, False))
            hits.append([])
            for l, planted in lefts:
                m = _ham(F[f0:f1], G[l:l + L])
                assert m <= 2 or not planted
                hits[s].append((rid, ref, l, l + L, anti, s == nseg - 1, m, m, L))
        seq = "".join(F)
        seq = revcomp(seq) if anti else seq
        b.plan[rid] = (seq, hits)
        if only:
            return None
        key = (ref, t0 + r.left, r.k)
        got = [(i, li, ri, x) for i, li, ri, rf, left, x in sightings(_Lazy(self.g), L, MAX_INS, seq, hits) if (rf, left, len(x)) == key]
        assert got == expect == sorted(expect), "read %d: planted %r, the restatement sees %r" % (rid, expect, got)
        c = Contest(key, bi, rid, got, note, winner=got[0][3], site=(ref, t0))
        for i, li, ri, x in got:                # the read with that sighting alone: its two segments hold nothing but its two hits
            keep = {i: li, i + 1: ri}
            c.alone.append(([[h for n, h in enumerate(hs) if s not in keep or n == keep[s]] for s, hs in enumerate(hits)], x))
        self.contests.append(c)
        return c


class _Lazy:
    """the contigs as strings, joined when asked for (the genome is a list of letters while the plants go in)"""
    def __init__(self, g):
        self.g, self.s = g, {}

    def __getitem__(self, k):
        if k not in self.s:
            self.s[k] = "".join(self.g[k])
        return self.s[k]




# ------------------------------------------------------------------------------------------------ scenarios
@dataclass
class TScenario(ic.Scenario):
    min_counts: Dict[tuple, int] = None             # {tokens of a contest's note: the least number of contests that carry them all}


_TWO_DIAGONALS, _CROSSED = ((0, 0), (1, 1)), ((0, 1), (1, 0))
_ACROSS, _ACROSS_I = ((0, 0), (1, 0)), ((1, 1), (0, 0))      # the second: (li, ri) alone would put the pair i + 1 first -- i has to outrank them
KS = (1, 2, 3, 6)


def _name(slots) -> str:
    return "%d,%d-%d,%d" % (slots[0] + slots[1])


def _note(c: Contest, kind: str, slots, anti: bool, k: int, *more):
    pol = "first-smaller" if smaller(c.sights[0][3], c.sights[1][3]) else "first-larger"
    assert pol == "first-smaller" or smaller(c.sights[1][3], c.sights[0][3])
    c.note = "/".join((kind, _name(slots), pol, "antisense" if anti else "forward", "k%d" % k) + more)


def _same(bd: TBuilder, b: int, rids, r: Raw, anti: bool, pair: int, slots, pad: int = 0, *more):
    """a same-pair contest in both polarities: either sighting visited first"""
    for first in "AB":
        c = bd.tandem_read(b, next(rids), r, anti, pair, slots, first=first, pad=pad)
        _note(c, "same", slots, anti, r.k, *more)


def _across(bd: TBuilder, b: int, rids, k: int, n: int, anti: bool, pair: int, slots, pad: int = 0, *more):
    """an across-pairs contest in both polarities: a piece of either order (in an antisense read the genomic second pair is pair i)"""
    for ordered in (True, False):
        r = raw("across", k, bd.L, ordered, n)
        c = bd.tandem_read(b, next(rids), r, anti, pair, slots, pad=pad)
        _note(c, "across", slots, anti, k, "pairs%d,%d" % (pair, pair + 1), *more)


def _finish(bd: TBuilder, min_counts) -> TScenario:
    sc = bd.build(sum(1 for _ in bd.contests))
    return TScenario(min_counts=min_counts, **{f: getattr(sc, f) for f in ("name", "seqs", "L", "pkw", "batches", "contests", "min_contests")})


def _two() -> TScenario:
    """500 reads of four segments, at most two hits a segment: class GEN_TWO (flat2_read says "has a task", the second pass runs the
    loops).  Same-pair contests with the lists in step and crossed, either sighting first -- for the two-hit lists that IS the
    same read with both lists reversed --, across-pairs contests at the pairs (0, 1), the only two of such a read; both strands,
    k = 1, 2, 3, 6"""
    bd = TBuilder("two", 101, contig_lens=(90000, 60000), max_insertion_length=MAX_INS)
    b = bd.batch(READ_LEFT, 500, 7)
    rids = iter(range(2, 500, 5))
    n = 0
    for k in KS:
        for which in (0, 1):
            for anti in (False, True):
                for slots in (_TWO_DIAGONALS, _CROSSED):
                    n += 1
                    _same(bd, b, rids, raw("same", k, 25, None, which), anti, n & 1, slots)
    for k in KS:
        for anti in (False, True):
            for slots in (_ACROSS, _ACROSS_I):
                _across(bd, b, rids, k, 0, anti, 0, slots)
    bd.batch(READ_RIGHT, 300, 7 + 500)              # a plain right side: for the pair call and the executable
    return _finish(bd, {("same", _name(s), pol): 16 for s in (_TWO_DIAGONALS, _CROSSED) for pol in ("first-smaller", "first-larger")} |
                   {("across", _name(s), pol, strand): 4 for s in (_ACROSS, _ACROSS_I) for pol in ("first-smaller", "first-larger") for strand in ("forward", "antisense")} |
                   {("k%d" % k,): 24 for k in KS})


# the layouts with long lists: ((li, ri) of the sighting visited first, of the other) and what each tells.  (A layout such as (2, 31)
# against (2, 32) cannot exist -- one hit of segment i in both sightings --, so bit 5 of ri is crossed with li one apart; ri = 7 needs
# 2 + 8 hits in the pair's segments alone, so the read of exactly 8 hits has ri = 3.)
_LONG_LISTS = (
    (((3, 40), (4, 0)), "a high ri against a low one: ri must not run into li's bits"),
    (((31, 5), (32, 0)), "bit 5 of li"),
    (((2, 32), (3, 0)), "bit 5 of ri: in a field of 5 bits it is li's lowest, the two priorities tie and the smaller letters win"),
    (((39, 40), (40, 0)), "the top of the default cap of 40 hits a segment (indices up to 40: 41 hits, one past it)"),
    (((0, 7), (1, 0)), "ri = 7: twelve hits, the least such a read can have"),
    (((0, 3), (1, 0)), "exactly 8 hits in the read (2 + 4 + 1 + 1): the last class of thj_k_sj_general's first instance"),
)
_PADS = (1, 2, 3, 26, 27, 84)                       # decoys more in a read of 2 + 2 + 1 + 1 hits
_ACROSS_LI = ((34, 0), (1, 0))                      # li = 34 of pair i: in a field of 5 bits it would carry into i and pass pair i + 1's (1, 0)


def _paths() -> TScenario:
    """600 reads: the layouts with long lists, and the short ones padded with decoys to 7 - 8, 9 - 32 and 33 - 90 hits a read
    (thj_k_sj_general's two instances, thj_k_segjuncs_shared)"""
    bd = TBuilder("paths", 102, contig_lens=(90000, 90000), max_insertion_length=MAX_INS)
    b = bd.batch(READ_LEFT, 600, 11)
    rids = iter(range(3, 600, 5))
    n = 0
    for slots, _why in _LONG_LISTS:
        for anti in (False, True):
            n += 1
            _same(bd, b, rids, raw("same", KS[n % 4], 25, None, n & 1), anti, (n >> 1) & 1, slots, 0, "long-lists")
    for pad in _PADS:                               # 6 + pad hits: 7, 8 | 9, 32 | 33, 90
        for slots in (_TWO_DIAGONALS, _CROSSED):
            n += 1
            _same(bd, b, rids, raw("same", KS[n % 4], 25, None, (n >> 2) & 1), bool(n & 1), (n >> 1) & 1, slots, pad, "hits%d" % (6 + pad))
    for anti in (False, True):
        n += 1
        _across(bd, b, rids, KS[n % 4], 1, anti, 0, _ACROSS_LI, 0, "long-lists")
        for pad, slots in ((2, _ACROSS), (20, _ACROSS_I), (60, _ACROSS)):
            n += 1
            _across(bd, b, rids, KS[n % 4], 1, anti, 0, slots, pad, "padded")
    bd.batch(READ_RIGHT, 300, 11 + 600)             # a plain right side: for the executable
    return _finish(bd, {("same", _name(s), pol): 2 for s, _w in _LONG_LISTS for pol in ("first-smaller", "first-larger")} |
                   {("hits%d" % (6 + pad),): 4 for pad in _PADS} |
                   {("across", _name(_ACROSS_LI), pol): 2 for pol in ("first-smaller", "first-larger")} | {("across", "padded"): 12})


PATHS_HITS = {7, 8, 9, 12, 32, 33, 90}              # hits a read that _paths plants, of every class (6, the least: `two`)


def _overflow() -> TScenario:
    """self-contests of 12 + 12 hits among 66 reads of 144 windows each (ins_conflicts.heavy_reads): their workgroup's task queue runs
    full and the tasks take the un-queued push"""
    bd = TBuilder("overflow", 103, contig_lens=(90000, 60000), max_insertion_length=MAX_INS)
    b = bd.batch(READ_LEFT, 400, 5)
    mine = (118, 119, 140, 141, 170, 171, 172, 173)
    rids = iter(mine)
    for n, anti in enumerate((False, True)):
        _same(bd, b, rids, raw("same", KS[n], 25, None, 0), anti, n, ((5, 11), (6, 0)), 0, "overflow")
        _same(bd, b, rids, raw("same", KS[n + 2], 25, None, 1), not anti, 1 - n, ((0, 11), (11, 0)), 0, "overflow")
    ic.heavy_reads(bd, b, [r for r in range(100, 170) if r not in mine])
    return _finish(bd, {("overflow", pol): 4 for pol in ("first-smaller", "first-larger")})


def _long() -> TScenario:
    """reads of 16 segments (400 bases at L = 25): across-pairs contests at the pairs (12, 13) -- the i & 15 field holds 12 and 13 --
    and at (0, 1), same-pair contests at the pairs 13 (the last), 12 and 0"""
    bd = TBuilder("long", 104, contig_lens=(90000, 60000), max_insertion_length=MAX_INS)
    b = bd.batch(READ_LEFT, 300, 9, rl=400)
    rids = iter(range(2, 300, 6))
    n = 0
    for k in KS:
        for anti in (False, True):
            n += 1
            _across(bd, b, rids, k, n & 1, anti, 12, _ACROSS_I if n & 2 else _ACROSS)
    _across(bd, b, rids, 2, 0, False, 0, _ACROSS_I)
    _across(bd, b, rids, 3, 0, True, 0, _ACROSS)
    for n, pair in enumerate((13, 12, 0, 13)):
        _same(bd, b, rids, raw("same", KS[n], 25, None, 0), bool(n & 1), pair, _CROSSED if n & 2 else _TWO_DIAGONALS)
    return _finish(bd, {("across", "pairs12,13", pol, strand): 4 for pol in ("first-smaller", "first-larger") for strand in ("forward", "antisense")} |
                   {("across", "pairs0,1"): 4, ("same",): 8})


def _wide() -> TScenario:
    """segment_length 50: the 2L piece and its letters on 128-bit plane words"""
    bd = TBuilder("wide", 105, L=50, contig_lens=(90000, 60000), max_insertion_length=MAX_INS)
    b = bd.batch(READ_LEFT, 300, 13, rl=200)
    rids = iter(range(2, 300, 5))
    n = 0
    for k in KS:
        for anti in (False, True):
            n += 1
            _across(bd, b, rids, k, n & 1, anti, 0, _ACROSS_I if n & 2 else _ACROSS)
    for k in sorted(k for kind, k, L, _o in RAW_SEEDS if kind == "same" and L == 50):
        for anti in (False, True):
            n += 1
            _same(bd, b, rids, raw("same", k, 50, None, (n & 1) % len(RAW_SEEDS[("same", k, 50, None)])), anti, n & 1, _CROSSED if n & 2 else _TWO_DIAGONALS)
    return _finish(bd, {("across", pol): 8 for pol in ("first-smaller", "first-larger")} | {("same", pol): 4 for pol in ("first-smaller", "first-larger")})


def _mixed() -> TScenario:
    """a self-contest whose place other reads claim too: with an earlier read there (the letters of the read's SECOND sighting) that
    read wins, whatever the read's own sightings say; with a later one only, the read's own first sighting wins"""
    bd = TBuilder("mixed", 106, contig_lens=(90000, 60000), max_insertion_length=MAX_INS)
    b = bd.batch(READ_LEFT, 400, 21)
    n = 0
    for k in KS:
        for anti in (False, True):
            for earlier in (True, False):
                for first in "AB":
                    n += 1
                    r = raw("same", k, 25, None, n & 1)
                    slots = _CROSSED if n & 2 else _TWO_DIAGONALS
                    c = bd.tandem_read(b, 100 + 3 * n, r, anti, n & 1, slots, first=first)
                    _note(c, "same", slots, anti, k, "earlier" if earlier else "later-only")
                    second = "B" if first == "A" else "A"
                    for rid in ((n + 1, 300 + n) if earlier else (300 + n,)):
                        bd.tandem_read(b, rid, r, not anti if n & 4 else anti, (n >> 1) & 1, ((0, 0),), only=second, site=c.site)
                        c.others.append((b, rid, c.sights[1][3]))
                    if earlier:
                        c.winner = c.sights[1][3]
    return _finish(bd, {("earlier", pol): 8 for pol in ("first-smaller", "first-larger")} | {("later-only", pol): 8 for pol in ("first-smaller", "first-larger")})


_SCENARIOS = {"two": _two, "paths": _paths, "overflow": _overflow, "long": _long, "wide": _wide, "mixed": _mixed}
NAMES = tuple(_SCENARIOS)


@functools.lru_cache(maxsize=None)
def scenario(name: str) -> TScenario:
    """built once a process, shared, never changed"""
    return _SCENARIOS[name]()


@functools.lru_cache(maxsize=None)
def expected(name: str):
    """the oracle's events of the batch that holds the contests (computed once a process)"""
    import orc
    sc = scenario(name)
    return orc.segjuncs(sc.params(0), orc.Genome(sc.seqs), sc.batches[0].sb)


@functools.lru_cache(maxsize=None)
def expected_pair(name: str):
    """... of the scenario's left batch and its plain right batch, as one pass"""
    import orc
    sc = scenario(name)
    return merge_events(expected(name), orc.segjuncs(sc.params(1), orc.Genome(sc.seqs), sc.batches[1].sb))


def halves(sc: TScenario):
    """the contests' batch as two with ordinal_base running on: [(SegBatch, ordinal_base)] in visiting order"""
    b = sc.batches[0]
    mid = b.n_reads // 2
    out = []
    for lo, hi in ((1, mid), (mid + 1, b.n_reads)):
        sb = build_seg_batch([[h for h in seg if lo <= h[0] <= hi] for seg in b.recs], {rid: s for rid, s in b.reads.items() if lo <= rid <= hi})
        assert sb.n_reads == hi - lo + 1
        out.append((sb, b.ordinal_base + lo - 1))
    return out


def count(sc: TScenario, *tokens) -> int:
    return sum(1 for c in sc.contests if set(tokens) <= set(c.note.split("/")))


def self_check(sc: TScenario) -> Dict[tuple, int]:
    """with the reference alone, a read at a time: each of a contest's two sightings, its two segments holding nothing but its two
    hits, reports the contest's (ref, left, length) with its own letters and no other insertion; the letters differ; the read with
    all its hits reports the letters of the sighting visited first there -- and altogether what the restatement says it reports;
    every other read of a mixed contest reports its letters at the place and nothing else.  The scenario holds the contests it
    promises -> their counts"""
    import orc
    g = orc.Genome(sc.seqs)
    for c in sc.contests:
        b = sc.batches[c.batch]
        p = sc.params(c.batch)
        seq, hits = b.plan[c.rid]
        assert len(c.sights) == 2 and c.sights[0][:3] < c.sights[1][:3] and c.sights[0][3] != c.sights[1][3], c.note
        assert all(len(x) == c.key[2] for _i, _l, _r, x in c.sights)
        for alone, x in c.alone:
            ev = orc.segjuncs(p, g, build_seg_batch(alone, {c.rid: seq}))
            assert ev.insertions == [(c.key[0], c.key[1], x)], "%s %s: one sighting of read %d reports %r" % (sc.name, c.note, c.rid, ev.insertions)
        ev = orc.segjuncs(p, g, sc.one_read(c.batch, c.rid))
        have = {(r, l, len(s)): s for r, l, s in ev.insertions}
        assert have.get(c.key) == c.first, "%s %s: read %d reports %r, visits %r first" % (sc.name, c.note, c.rid, have.get(c.key), c.first)
        model = {}
        for _i, _li, _ri, r, l, s in sightings(sc.seqs, sc.L, p.max_insertion_length, seq, hits):
            model.setdefault((r, l, len(s)), s)
        assert model == have, "%s %s: the restatement and the reference differ on read %d" % (sc.name, c.note, c.rid)
        for bi, rid, x in c.others:
            ev = orc.segjuncs(sc.params(bi), g, sc.one_read(bi, rid))
            assert ev.insertions == [(c.key[0], c.key[1], x)], (sc.name, c.note, rid, ev.insertions)
        ords = [sc.ordinal(bi, rid) for bi, rid, _x in c.others] + [sc.ordinal(c.batch, c.rid)]
        assert c.winner == (c.first if min(ords) == ords[-1] else c.others[ords.index(min(ords))][2])
    counts = {k: count(sc, *k) for k in sc.min_counts}
    assert all(counts[k] >= n for k, n in sc.min_counts.items()), "%s: %r for %r" % (sc.name, counts, sc.min_counts)
    assert len(sc.contests) >= sc.min_contests
    return counts


def assert_first_wins(sc: TScenario, ev, what: str = ""):
    """every contest's place carries the letters of the sighting visited first (of the earliest read's, where several claim it)"""
    have = {(r, l, len(s)): s for r, l, s in ev.insertions}
    for c in sc.contests:
        assert have.get(c.key) == c.winner, "%s %s %s: %r at %r, read %d visits %r first" % (what, sc.name, c.note, have.get(c.key), c.key, c.rid, c.winner)


# ------------------------------------------------------------------------------------------------ the wrong rules
def _prio(i: int, li: int, ri: int, wl: int = 6, wr: int = 6, mask: bool = False) -> int:
    """ins_prio's low bits with fields of wl / wr bits for li / ri, values that do not fit cut off (`mask`) or carried on"""
    if mask:
        li, ri = li & ((1 << wl) - 1), ri & ((1 << wr) - 1)
    return ((i & 15) << (wl + wr)) + (li << wr) + ri


RULES = {
    "first visited": lambda i, li, ri: _prio(i, li, ri),
    "last visited": lambda i, li, ri: -_prio(i, li, ri),
    "li and ri swapped": lambda i, li, ri: _prio(i, ri, li),
    "i dropped": lambda i, li, ri: _prio(0, li, ri),
    "li in 5 bits, cut off": lambda i, li, ri: _prio(i, li, ri, wl=5, mask=True),
    "li in 5 bits, carried into i": lambda i, li, ri: _prio(i, li, ri, wl=5),
    "ri in 5 bits, carried into li": lambda i, li, ri: _prio(i, li, ri, wr=5),
    "smallest letters": lambda i, li, ri: 0,
}


def rule_winner(c: Contest, rule) -> str:
    """the letters the read's own sightings leave under `rule`: the smallest priority, among equal ones the smaller packed letters
    (the table keeps the minimum of priority << 18 | letters)"""
    return min(c.sights, key=lambda s: (rule(*s[:3]), packed(s[3])))[3]


def wrong_by_rule(sc: TScenario) -> Dict[str, List[str]]:
    """{rule: the notes of the contests whose read would keep other letters than those of its first sighting}"""
    out = {name: [c.note for c in sc.contests if rule_winner(c, rule) != c.first] for name, rule in RULES.items()}
    out["largest letters"] = [c.note for c in sc.contests if max(c.sights, key=lambda s: packed(s[3]))[3] != c.first]
    return out


if __name__ == "__main__" and sys.argv[1:2] == ["search"]:
    # python tests/ins_tandem.py search [kind L]: the lines of RAW_SEEDS
    for kind in ("same", "across"):
        for L in (25, 50):
            if sys.argv[2:] and (kind, str(L)) != tuple(sys.argv[2:4]):
                continue
            for k in (1, 2, 3, 6):
                for ordered in ((None,) if kind == "same" else (True, False)):
                    print("    %r: %r," % ((kind, k, L, ordered), search(kind, k, L, 4 if L == 25 else 2, 250000 if k > 1 else 700000, ordered)), flush=True)
