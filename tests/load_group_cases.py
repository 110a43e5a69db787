"""Planted reads for the loads that tier 0, the chain join and the finish of a joined hit issue unconditionally and in groups
(thj_span_core.h: contig_finish, join_compute, joined_extras): reads whose alignments touch the first and the last base of a contig,
whose length is on either side of a 64-base piece and of a plane word, whose junction lies INSIDE a segment hit (the junction-db
mapping's aM gN bM record, so that the chain abuts everywhere and thj_k_join_finish finishes it) or on a segment boundary (closure
kernel, thj_k_finish), and chain lists of exactly 1, 255, 256 and 257 entries.  Plain Python over numpy; the oracle says what the
records are.  Shared by test_gpu_load_groups.py and test_loadsim_cpu.py.

A read is described in genome orientation ("F", as in md_edges.py); `gaps` are (F offset, kind, length[, strand]) with kind "N"
(intron) or "D" (deletion): strictly inside a segment the gap becomes an op of that hit's cigar, on a segment boundary the two hits
do not abut and the chain is joined through the junction set."""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

import md_edges as me
from tophat_amd.batch import HIT_ANTISENSE_SPLICE, JUNC_DTYPE, SPAN_HIT_DTYPE, SpanBatch

_RC = str.maketrans("ACGTN", "TGCAN")
OP_M, OP_N, OP_D = 1, 11, 5         # cigar op codes of thj_span_core.h (MATCH, REF_SKIP, DEL)


@dataclass
class Read:
    tag: str
    rl: int = 100
    anti: bool = False
    subs: Tuple[int, ...] = ()
    read_n: Tuple[int, ...] = ()
    gen_n: Tuple[int, ...] = ()
    gaps: Tuple[tuple, ...] = ()
    quals: Optional[bytes] = None
    edge: str = ""                 # "start": the alignment begins at base 0 of a new contig; "end": it ends on the contig's last base


def _segments(rl: int, L: int, anti: bool):
    """F intervals of the read's segments, in F order (the last segment of the read takes the remainder)"""
    nseg = max(1, rl // L)
    cuts = sorted((rl - k * L) if anti else k * L for k in range(1, nseg))
    cuts = [0] + cuts + [rl]
    return list(zip(cuts[:-1], cuts[1:]))


class Genome:
    """contigs grown read by read; a read with edge "start" opens a new contig, one with edge "end" closes the current one"""
    def __init__(self, rng):
        self.rng, self.contigs, self.cur = rng, [], None

    def _rand(self, n):
        return [str(c) for c in self.rng.choice(list("ACGT"), size=n)]

    def open(self):
        self.cur = []
        self.contigs.append(self.cur)

    def place(self, sp: Read, L: int, juncs):
        if self.cur is None or sp.edge == "start":
            self.open()
        g = self.cur
        if sp.edge != "start":
            g.extend(self._rand(60))
        gap_at = {f: (gp[1], gp[2], gp[3] if len(gp) > 3 else 0) for gp in sp.gaps for f in [gp[0]]}
        pos = len(g)
        g.extend(self._rand(sp.rl + sum(n for _k, n, _s in gap_at.values())))
        ref = len(self.contigs)
        gmap = []
        for f in range(sp.rl):
            if f in gap_at:
                kind, n, strand = gap_at[f]
                juncs.append((ref, pos - 1, pos + n, int(strand)))        # (a deletion is looked up in the junction set too)
                pos += n
            gmap.append(pos); pos += 1
        assert pos == len(g)
        F = []
        for f in range(sp.rl):
            base = g[gmap[f]]
            if f in sp.gen_n:
                g[gmap[f]] = "N"
            if f in sp.read_n:
                base = "N"
            elif f in sp.subs:
                base = "ACGT"[("ACGT".index(base) + 1 + f % 3) % 4]
            F.append(base)
        hits = []
        for f0, f1 in _segments(sp.rl, L, sp.anti):
            cig, run, asplice = [], 0, 0
            for f in range(f0, f1):
                if f in gap_at and f > f0:
                    kind, n, strand = gap_at[f]
                    cig += [(OP_M << 28) | run, ((OP_N if kind == "N" else OP_D) << 28) | n]
                    run = 0
                    asplice |= HIT_ANTISENSE_SPLICE if (kind == "N" and strand) else 0
                run += 1
            cig.append((OP_M << 28) | run)
            assert len(cig) <= 5
            mm = sum(1 for f in range(f0, f1) if g[gmap[f]] != F[f] or g[gmap[f]] == "N")
            ed = mm + sum(c & 0x0FFFFFFF for c in cig if c >> 28 == OP_D)
            hits.append((ref, gmap[f0], asplice, mm, ed, len(cig), cig + [0] * (5 - len(cig))))
        if sp.edge == "end":
            self.cur = None
        return "".join(F), sp.quals if sp.quals is not None else me.default_quals(sp.rl), hits

    def close(self):
        if self.cur is not None:
            self.cur.extend(self._rand(200))
        return ["".join(c) for c in self.contigs]


def build(groups, seed: int):
    """groups: [(name, nseg of the batch, segment length, [Read])] over one genome -> {name: (seqs, SpanBatch, params, juncs, ins, tags)}"""
    rng = np.random.default_rng(seed)
    G, juncs, packed = Genome(rng), [], []
    for name, nseg, L, specs in groups:
        hits, seg_off, bases, quals, read_off = [], [0], bytearray(), bytearray(), [0]
        for sp in specs:
            F, fq, fh = G.place(sp, L, juncs)
            n = len(fh)
            assert n <= nseg and len(fq) == sp.rl
            for s in range(nseg):
                if s < n:
                    ref, left, fl, mm, ed, nc, cig = fh[n - 1 - s] if sp.anti else fh[s]
                    hits.append((ref, left, fl | (1 if sp.anti else 0) | (2 if s == n - 1 else 0), mm, ed, nc, cig))
                seg_off.append(len(hits))
            bases += (F.translate(_RC)[::-1] if sp.anti else F).encode()
            quals += fq[::-1] if sp.anti else fq
            read_off.append(len(bases))
        k = len(specs)
        sb = SpanBatch(nseg, np.arange(1, k + 1, dtype=np.uint32), np.array(read_off, dtype=np.int64),
                       np.frombuffer(bytes(bases), dtype=np.uint8).copy(), np.frombuffer(bytes(quals), dtype=np.uint8).copy(),
                       np.array(seg_off, dtype=np.uint32), np.array(hits, dtype=SPAN_HIT_DTYPE))
        packed.append((name, sb, me.params(segment_length=L), [sp.tag + ("/anti" if sp.anti else "/sense") for sp in specs]))
    seqs = G.close()
    j = np.array(sorted(set(juncs)), dtype=JUNC_DTYPE) if juncs else np.zeros(0, dtype=JUNC_DTYPE)
    return {name: (seqs, sb, p, j, [], tags) for name, sb, p, tags in packed}


# ------------------------------------------------------------------------------------------------ the planted reads
def _piece_sites(rl):
    return tuple(sorted({f for f in (0, 63, 64, rl - 1) if f < rl}))


def shapes(rl: int, tagp: str, spliced: bool):
    """the reads of one length: clean, mismatches on the piece edges, N in the read / the genome / both, seven quality-penalised
    mismatches (qq_add's overflow), both strands; `spliced`: the same walk with a junction inside the first, a middle and the last
    segment hit and with a junction and a deletion on a segment boundary (reads of 50 bases and more)"""
    out = []
    many = tuple(sorted({(11 * k + 3) % rl for k in range(9)}))
    for anti in (False, True):
        out.append(Read("%s/rl%d/clean" % (tagp, rl), rl=rl, anti=anti))
        out.append(Read("%s/rl%d/edges" % (tagp, rl), rl=rl, anti=anti, subs=_piece_sites(rl)))
        out.append(Read("%s/rl%d/n" % (tagp, rl), rl=rl, anti=anti, subs=(rl // 2,), read_n=(5,), gen_n=(9,)))
        out.append(Read("%s/rl%d/bothn" % (tagp, rl), rl=rl, anti=anti, read_n=(rl - 3,), gen_n=(rl - 3,)))
        out.append(Read("%s/rl%d/many" % (tagp, rl), rl=rl, anti=anti, subs=many))
        if spliced and rl >= 50:
            segs = _segments(rl, 25, anti)
            inside = sorted({(segs[0][0] + segs[0][1]) // 2, (segs[len(segs) // 2][0] + segs[len(segs) // 2][1]) // 2, (segs[-1][0] + segs[-1][1]) // 2})
            for k, f in enumerate(inside):
                out.append(Read("%s/rl%d/junction_in_hit%d" % (tagp, rl, k), rl=rl, anti=anti, subs=_piece_sites(rl) + (f, f - 1),
                                gaps=((f, "N", 70 + 13 * k + rl, anti),)))
            out.append(Read("%s/rl%d/junction_in_hit/many" % (tagp, rl), rl=rl, anti=anti, subs=many, read_n=(1,), gen_n=(rl - 2,),
                            gaps=((inside[0], "N", 150, 0),)))
            b = segs[1][0]
            out.append(Read("%s/rl%d/junction_on_boundary" % (tagp, rl), rl=rl, anti=anti, subs=_piece_sites(rl), gaps=((b, "N", 90 + rl, anti),)))
            out.append(Read("%s/rl%d/deletion" % (tagp, rl), rl=rl, anti=anti, subs=(0, b, rl - 1), gaps=((b, "D", 3),)))
    return out


def _edges(specs):
    """the first read of each strand opens a contig at its base 0, the last ones close it on its last base"""
    specs = list(specs)
    specs[0].edge = "start"
    specs[-1].edge = "end"
    return specs


def spliced_run(n: int, tagp: str):
    """n reads of 100 bases that travel as chain entries (a junction inside a hit), nothing else: a chain list of exactly n"""
    return [Read("%s/%d" % (tagp, k), anti=bool(k & 1), subs=((7 * k) % 100,), gaps=(((12, 37, 62, 88)[k % 4], "N", 64 + k % 50, k & 1),))
            for k in range(n)]


LIST_SIZES = (1, 255, 256, 257)


@functools.lru_cache(maxsize=None)
def cases():
    """{name: case}.  "seg4": lengths 25..100, at most four segments, two plane words: the register instances, chain entries.
    "seg5": 128 bases in five segments, two plane words.  "seg6": 129 and 150 bases, three plane words: the <8> tier-0 instance and the
    memory-read walks.  "long3": 129 and 150 bases at segment length 50 -- at most three segments, so spliced reads travel as chain
    entries with their planes in memory; a 150-base read with two junctions has four and five MATCH pieces.  "list<n>": chain lists."""
    seg4 = []
    for c, lens in enumerate(((25, 50, 64), (65, 100))):        # two contigs, a third with the other batches
        seg4 += _edges([r for rl in lens for r in shapes(rl, "seg4", True)])
    seg5 = _edges(shapes(128, "seg5", False) + shapes(65, "seg5", False) + shapes(25, "seg5", False))
    seg6 = _edges(shapes(129, "seg6", False) + shapes(150, "seg6", False) + shapes(64, "seg6", False) + shapes(100, "seg6", True))
    long3 = []
    for anti in (False, True):
        for rl in (129, 150):
            long3.append(Read("long3/rl%d/clean" % rl, rl=rl, anti=anti, subs=_piece_sites(rl)))
            long3.append(Read("long3/rl%d/one_junction" % rl, rl=rl, anti=anti, subs=_piece_sites(rl) + (70,), gaps=((70, "N", 120, anti),)))
            long3.append(Read("long3/rl%d/deletion" % rl, rl=rl, anti=anti, subs=(50, 128), gaps=((rl - 50 if anti else 50, "D", 4),)))
        long3.append(Read("long3/rl150/two_junctions", rl=150, anti=anti, subs=(0, 29, 30, 63, 64, 79, 80, 127, 128, 149), read_n=(100,), gen_n=(100, 140),
                          gaps=((30, "N", 200, anti), (80, "N", 333, anti))))
        long3.append(Read("long3/rl150/two_junctions/many", rl=150, anti=anti, subs=tuple(range(3, 150, 14)), gaps=((20, "N", 77, 0), (120, "N", 78, 0))))
    long3 = _edges(long3)
    groups = [("seg4", 4, 25, seg4), ("seg5", 5, 25, seg5), ("seg6", 6, 25, seg6), ("long3", 3, 50, long3)]
    groups += [("list%d" % n, 4, 25, spliced_run(n, "list%d" % n)) for n in LIST_SIZES]
    groups[-1][3][-1].edge = "end"              # the genome's last base is an alignment's last base
    return build(groups, 1407)


@functools.lru_cache(maxsize=None)
def two_copy_case():
    """reads on a two-fold repeat whose chains travel as a group of two (thj_k_chains: region B's dense list)"""
    specs = [me.Read("twocopy/%d" % k, anti=bool(k & 1), subs=s) for k, s in enumerate(((), (0,), (63, 64), (99,), (0, 13, 30, 49, 50, 88, 97)))]
    return me.build_repeat(specs, 2, 1408, me.params(max_report_intron=300, max_segment_intron=300))


NAMES = ("seg4", "seg5", "seg6", "long3") + tuple("list%d" % n for n in LIST_SIZES) + ("twocopy",)


def case(name: str):
    return two_copy_case() if name == "twocopy" else cases()[name]


@functools.lru_cache(maxsize=None)
def expected(name: str):
    """the oracle's records (computed once a process, shared, never changed)"""
    import orc
    seqs, sb, p, j, ins, _tags = case(name)
    return tuple(orc.spanning(p, orc.Genome(seqs), sb, j, ins))
