"""Planted edge cases for the spanning records' MD / AS walks (contig_finish, joined_extras, sam_extra, f_sam_extra) and for the
record slots: hand-built SpanBatch objects whose reads carry substitutions, N, deletions, insertions, introns and quality bytes at
chosen places, so that a test reaches a given MD offset, token size, quality slot or 64-base piece edge on purpose and not by the
luck of a random batch.  Plain Python over numpy; the oracle says what the records are, the families only say where to look.

A read is described in genome orientation ("F": what the genome strand reads at its placement, edits applied); an antisense read's
bases are F's reverse complement, its qualities F's reversed, and its segment s lies at the far end of the placement, as
build_span_batch lays it out.  Gaps (deletion, intron, insertion) sit on segment boundaries, where the one-hit-per-segment chain
is joined through the junction / insertion sets.

Every family returns a list of cases (seqs, sb, params, juncs, ins, tag_per_read); the tag names family and pattern."""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from tophat_amd.batch import JUNC_DTYPE, SPAN_HIT_DTYPE, SpanBatch
from tophat_amd.params import Params

_RC = str.maketrans("ACGTN", "TGCAN")
QCAP = 6            # thj_span_core.h: qualities noted per record before the one-by-one loads
QUAL_BYTES = (33, 34, 35, 73, 74, 75, 126)      # phred 0, 1, 2 and both sides of the clamp at 40


def params(**kw) -> Params:
    base = dict(read_mismatches=30, read_edit_dist=40, read_gap_length=10, segment_mismatches=10, max_deletion_length=10)
    base.update(kw)
    return Params(**base)


@dataclass
class Read:
    tag: str
    rl: int = 100
    L: int = 25
    anti: bool = False
    subs: Tuple[int, ...] = ()         # F offsets with a substituted base
    read_n: Tuple[int, ...] = ()       # F offsets where the read holds N
    gen_n: Tuple[int, ...] = ()        # F offsets whose genome base is N
    # (boundary number 1.., kind, length[, junction strand]); kinds: "D" deletion, "N" intron, "I" inserted bases that open the
    # segment behind the boundary, "i" inserted bases that close the segment before it
    gaps: Tuple[tuple, ...] = ()
    quals: Optional[bytes] = None      # in F orientation; default: a ramp that is no palindrome
    hide: bool = False                 # leave the read's junctions and insertions out of the sets: its chain does not join


def n_segments(rl: int, L: int) -> int:
    return max(1, rl // L)


def boundaries(rl: int, L: int, anti: bool):
    """F offsets of the segment boundaries"""
    nseg = n_segments(rl, L)
    return sorted((rl - k * L) if anti else k * L for k in range(1, nseg))


def default_quals(rl: int) -> bytes:
    return bytes(35 + (7 * i + i // 11) % 40 for i in range(rl))


def _place(rng, genome, sp: Read, juncs, ins):
    """append the read's stretch of genome; -> (F, quals in F orientation, [(f0, f1, left, mismatches)] per F interval)"""
    fb = boundaries(sp.rl, sp.L, sp.anti)
    gap_at, inserted, ins_after = {}, set(), []
    for gp in sp.gaps:
        b, kind, n = gp[0], gp[1], gp[2]
        pos = fb[b - 1]
        if kind in "DN":
            gap_at[pos] = (n, gp[3] if len(gp) > 3 else 0)
        elif kind == "I":
            inserted.update(range(pos, pos + n)); ins_after.append((pos - 1, pos, n))
        else:
            inserted.update(range(pos - n, pos)); ins_after.append((pos - n - 1, pos - n, n))
    genome.extend(rng.choice(list("ACGT"), size=60))
    g = len(genome)
    genome.extend(rng.choice(list("ACGT"), size=sp.rl + sum(n for n, _ in gap_at.values()) + 60))
    gmap, my_j = [], []
    for f in range(sp.rl):
        if f in gap_at:
            n, strand = gap_at[f]
            my_j.append((1, g - 1, g + n, strand))
            g += n
        if f in inserted:
            gmap.append(-1)
        else:
            gmap.append(g); g += 1
    F = []
    for f in range(sp.rl):
        if gmap[f] < 0:
            F.append(str(rng.choice(list("ACGT"))))
            continue
        base = genome[gmap[f]]
        if f in sp.gen_n:
            genome[gmap[f]] = "N"
        if f in sp.read_n:
            base = "N"
        elif f in sp.subs:
            base = "ACGT"[("ACGT".index(base) + 1 + f % 3) % 4]
        F.append(base)
    if not sp.hide:
        juncs.extend(my_j)
        for before, first, n in ins_after:
            ins.append((1, gmap[before], "".join(F[first:first + n])))
    cuts = [0] + fb + [sp.rl]
    hits = []
    for f0, f1 in zip(cuts[:-1], cuts[1:]):
        left = gmap[f0] if gmap[f0] >= 0 else gmap[f1 - 1] - (f1 - f0 - 1)
        mm = sum(1 for a, b in zip(genome[left:left + f1 - f0], F[f0:f1]) if a != b or a == "N")
        hits.append((f0, f1, left, mm))
    return "".join(F), sp.quals if sp.quals is not None else default_quals(sp.rl), hits


def build(groups, p: Optional[Params] = None, seed: int = 0):
    """groups: lists of Read, a batch each, over one genome -> (seqs, [SpanBatch], params, juncs, ins, [tags])"""
    rng = np.random.default_rng(seed)
    genome, juncs, ins = [], [], []
    sbs, tags = [], []
    for specs in groups:
        nsegs = {n_segments(sp.rl, sp.L) for sp in specs}
        assert len(nsegs) == 1, "one batch, one number of segments"
        nseg = nsegs.pop()
        hits, seg_off, bases, quals, read_off = [], [0], bytearray(), bytearray(), [0]
        for sp in specs:
            F, fq, fh = _place(rng, genome, sp, juncs, ins)
            assert len(fq) == sp.rl and len(fh) == nseg
            for s in range(nseg):
                f0, f1, left, mm = fh[nseg - 1 - s] if sp.anti else fh[s]
                flags = (1 if sp.anti else 0) | (2 if s == nseg - 1 else 0)
                hits.append((1, left, flags, mm, mm, 1, [(1 << 28) | (f1 - f0), 0, 0, 0, 0]))
                seg_off.append(len(hits))
            bases += (F.translate(_RC)[::-1] if sp.anti else F).encode()
            quals += fq[::-1] if sp.anti else fq
            read_off.append(len(bases))
        n = len(specs)
        sbs.append(SpanBatch(nseg, np.arange(1, n + 1, dtype=np.uint32), np.array(read_off, dtype=np.int64),
                             np.frombuffer(bytes(bases), dtype=np.uint8).copy(), np.frombuffer(bytes(quals), dtype=np.uint8).copy(),
                             np.array(seg_off, dtype=np.uint32), np.array(hits, dtype=SPAN_HIT_DTYPE)))
        tags.append([sp.tag + ("/anti" if sp.anti else "/sense") for sp in specs])
    genome.extend(rng.choice(list("ACGT"), size=200))
    j = np.array(sorted(set(juncs)), dtype=JUNC_DTYPE) if juncs else np.zeros(0, dtype=JUNC_DTYPE)
    return ["".join(genome)], sbs, p or params(), j, sorted(ins, key=lambda x: (x[0], x[1], len(x[2]))), tags


def build_one(specs, p: Optional[Params] = None, seed: int = 0):
    seqs, sbs, p, j, ins, tags = build([specs], p, seed)
    return seqs, sbs[0], p, j, ins, tags[0]


def build_repeat(specs, copies: int, seed: int, p: Optional[Params] = None):
    """the reads' patterns on a `copies`-fold tandem repeat, every copy changed at a few places of its own (as
    test_md_as_quals_cpu.mutated_repeat_batch does): every segment hits every copy, the read has a record per copy, each with its
    own mismatches.  Reads of 100 bases in four segments, substitutions and read N only."""
    rng = np.random.default_rng(seed)
    unit = [str(c) for c in rng.choice(list("ACGT"), size=400)]
    flank = [str(c) for c in rng.choice(list("ACGT"), size=3000)]
    genome = flank + unit * copies + flank
    for c in range(copies):
        for k in rng.choice(400, size=int(rng.integers(0, 9)), replace=False):
            i = 3000 + c * 400 + int(k)
            genome[i] = "N" if rng.random() < 0.1 else "ACGT"[("ACGT".index(genome[i]) + 1) % 4]
    L, nseg, rl = 25, 4, 100
    hits, seg_off, bases, quals, read_off, tags = [], [0], bytearray(), bytearray(), [0], []
    for sp in specs:
        assert sp.rl == rl and sp.L == L and not sp.gaps and not sp.gen_n
        off = int(rng.integers(0, 400 - rl))
        F = list(unit[off:off + rl])
        for f in sp.subs:
            F[f] = "ACGT"[("ACGT".index(F[f]) + 1 + f % 3) % 4]
        for f in sp.read_n:
            F[f] = "N"
        for s in range(nseg):
            f0, f1 = (rl - (s + 1) * L, rl - s * L) if sp.anti else (s * L, (s + 1) * L)
            for c in range(copies):
                left = 3000 + c * 400 + off + f0
                mm = sum(1 for a, b in zip(genome[left:left + L], F[f0:f1]) if a != b or a == "N")
                hits.append((1, left, (1 if sp.anti else 0) | (2 if s == nseg - 1 else 0), mm, mm, 1, [(1 << 28) | L, 0, 0, 0, 0]))
            seg_off.append(len(hits))
        F = "".join(F)
        fq = sp.quals if sp.quals is not None else default_quals(rl)
        bases += (F.translate(_RC)[::-1] if sp.anti else F).encode()
        quals += fq[::-1] if sp.anti else fq
        read_off.append(len(bases))
        tags.append("%s/x%d%s" % (sp.tag, copies, "/anti" if sp.anti else "/sense"))
    n = len(specs)
    sb = SpanBatch(nseg, np.arange(1, n + 1, dtype=np.uint32), np.array(read_off, dtype=np.int64),
                   np.frombuffer(bytes(bases), dtype=np.uint8).copy(), np.frombuffer(bytes(quals), dtype=np.uint8).copy(),
                   np.array(seg_off, dtype=np.uint32), np.array(hits, dtype=SPAN_HIT_DTYPE))
    return ["".join(genome)], sb, p or params(), np.zeros(0, dtype=JUNC_DTYPE), [], tags


# ------------------------------------------------------------------------------------------------ MD arithmetic
def md_tokens(md: str):
    """(offset, size) of the tokens md_append is called with for this string: <run><letter> of a mismatch, <run>^ of a deletion,
    the deletion's letters four a token, the final run"""
    out, i, n = [], 0, len(md)
    while i < n:
        j = i
        while j < n and md[j].isdigit():
            j += 1
        if j == n:
            out.append((i, j - i))
            break
        out.append((i, j + 1 - i))
        if md[j] == "^":
            k = j + 1
            while k < n and md[k].isalpha():
                k += 1
            out.extend((q, min(4, k - q)) for q in range(j + 1, k, 4))
            i = k
        else:
            i = j + 1
    return out


_LO = {1: 0, 2: 10, 3: 100}
_HI = {1: 9, 2: 99, 3: 999}


def fit_runs(sizes, final_digits: int, cover: int, final: Optional[int] = None):
    """match runs in front of mismatch tokens of `sizes` characters (digits + letter) and a final run of `final_digits` digits that
    cover `cover` bases -> (runs, final run) or None"""
    runs = [_LO[s - 1] for s in sizes]
    fin = _LO[final_digits] if final is None else final
    need = cover - (sum(runs) + len(runs) + fin)
    if need < 0 or not _LO[final_digits] <= fin <= _HI[final_digits]:
        return None
    if final is None:
        add = min(need, _HI[final_digits] - fin); fin += add; need -= add
    for i, s in enumerate(sizes):
        add = min(need, _HI[s - 1] - runs[i]); runs[i] += add; need -= add
    return (runs, fin) if need == 0 else None


def sites(runs, start: int = 0):
    out, pos = [], start - 1
    for r in runs:
        pos += r + 1
        out.append(pos)
    return tuple(out)


def compositions(o: int):
    """ways to fill o characters with 2- and 3-character tokens, most 3s first"""
    for a in range(o // 3, -1, -1):
        if (o - 3 * a) % 2 == 0:
            yield [3] * a + [2] * ((o - 3 * a) // 2)
            if a and o - 3 * a:
                yield [2] * ((o - 3 * a) // 2) + [3] * a


# ------------------------------------------------------------------------------------------------ families
def ladder_patterns(per_length: int = 2):
    """{MD length: [substitution sites]} on 100-base reads, one- and two-digit runs mixed"""
    out = {}
    for T in range(3, 45):
        found = []
        for fd in (2, 1, 3):
            for sizes in compositions(T - fd) if T - fd > 0 else [[]]:
                fit = fit_runs(sizes, fd, 100)
                if fit and sites(fit[0]) not in found:
                    found.append(sites(fit[0]))
        out[T] = found[:per_length]
    return out


def ladder(p: Optional[Params] = None, seed: int = 101):
    """every MD length 3..44 of a 100-base read, sense and antisense, as a contig read (contig_finish) and with an intron on the second
    boundary (joined_extras; the intron leaves MD as it is)"""
    specs = []
    for T, pats in ladder_patterns().items():
        for v, subs in enumerate(pats):
            for anti in (False, True):
                specs.append(Read("ladder/md%d/v%d/plain" % (T, v), anti=anti, subs=subs))
                specs.append(Read("ladder/md%d/v%d/spliced" % (T, v), anti=anti, subs=subs, gaps=((2, "N", 70 + T, anti),)))
    return [build_one(specs, p, seed)]


def _mismatch_target(o, n, rls):
    for rl in rls:
        for fd in (1, 2, 3):
            if o + n + fd > 40:
                continue
            for pre in compositions(o) if o else [[]]:
                fit = fit_runs(pre + [n], fd, rl)
                if fit:
                    return rl, sites(fit[0])
    return None


def _final_target(o, n, rls):
    for rl in rls:
        for pre in compositions(o) if o else [[]]:
            fit = fit_runs(pre, n, rl)
            if fit:
                return rl, sites(fit[0])
    return None


def _deletion_target(o, d, after=False):
    """a 100-base read whose `<run>^` token starts at MD offset o: -> Read fields or None"""
    for b, P in ((1, 25), (2, 50), (3, 75)):
        for cs in (2, 3):
            for pre in compositions(o) if o else [[]]:
                fit = fit_runs(pre, cs - 1, P)
                if fit:
                    subs = sites(fit[0]) + ((P,) if after else ())
                    return dict(subs=subs, gaps=((b, "D", d),))
    return None


def sweep(p: Optional[Params] = None, seed: int = 202):
    """a token of every size at every offset of the MD buffer that a read can reach: filler mismatches in front of a mismatch token of
    2, 3 and 4 characters (the last needs a run of 100 or more: reads of 150 and 250 bases), of a final run of 1, 2 and 3 digits,
    and of deletions (the `^` token, 4-letter groups, a 1-letter rest)"""
    by_rl = {100: [], 150: [], 250: []}
    k = 0
    for o in range(40):
        for n in (2, 3, 4):
            for rls in ((100,),) if n < 4 else ((150,), (250,)):
                t = _mismatch_target(o, n, rls)
                if t:
                    by_rl[t[0]].append(Read("sweep/o%d/n%d/mismatch" % (o, n), rl=t[0], anti=bool(k & 1), subs=t[1])); k += 1
                    if n == 4:      # the same through a join: an intron leaves MD as it is
                        by_rl[t[0]].append(Read("sweep/o%d/n%d/mismatch/spliced" % (o, n), rl=t[0], anti=bool(k & 1), subs=t[1], gaps=((2, "N", 77, k & 1),))); k += 1
        for n in (1, 2, 3):
            for rls in ((100,), (150,), (250,)):
                t = _final_target(o, n, rls)
                if t:
                    by_rl[t[0]].append(Read("sweep/o%d/n%d/final" % (o, n), rl=t[0], anti=bool(k & 1), subs=t[1])); k += 1
        for d in (1, 4, 5, 8):
            t = _deletion_target(o, d)
            if t:
                by_rl[100].append(Read("sweep/o%d/del%d" % (o, d), anti=bool(k & 1), **t)); k += 1
    return [build_one(specs, p, seed + rl) for rl, specs in by_rl.items()]


def indels(p: Optional[Params] = None, seed: int = 303):
    """deletions of 1, 3, 4, 5, 8 and 10 bases whose `^` token lands on every offset mod 8 (so do their 4-letter groups), a mismatch on
    the base before and on the base behind (`...0^AC0T...`), MD strings that pass 24 and 40 characters inside the deletion, and
    insertions of 1..3 bases on either side of a boundary with mismatches next to them"""
    specs, k = [], 0
    for d in (1, 3, 4, 5, 8, 10):
        for o in list(range(3, 19)) + [20, 22, 23, 30, 33, 36, 37]:
            for b, P in ((1, 25), (2, 50), (3, 75)):
                fit = None
                for pre in compositions(o):
                    fit = fit_runs(pre, 1, P, final=0)      # no run behind the filler: its last mismatch is the base before the deletion
                    if fit:
                        break
                if fit:
                    # `0^` starts at MD offset o; the base behind the deletion is a mismatch too
                    specs.append(Read("indel/del%d/o%d" % (d, o), anti=bool(k & 1), subs=sites(fit[0]) + (P,), gaps=((b, "D", d),)))
                    k += 1
                    break
    for n in (1, 2, 3):
        for kind in "Ii":
            for b in (1, 2, 3):
                for anti in (False, True):
                    P = 25 * b
                    lo, hi = (P - 1, P + n) if kind == "I" else (P - n - 1, P)
                    specs.append(Read("indel/ins%d%s/b%d" % (n, kind, b), anti=anti, subs=(3, lo, hi, 97), gaps=((b, kind, n),)))
    return [build_one(specs, p, seed)]


def _qual_bytes(rl, at, values):
    q = bytearray(default_quals(rl))
    for f, v in zip(at, values):
        q[f] = v
    return bytes(q)


def qualities(p: Optional[Params] = None, seed: int = 404):
    """records with 5, 6, 7 and 12 mismatches that take a quality penalty, their quality bytes from QUAL_BYTES so that the sixth and the
    seventh differ; N in the read, in the genome and in both among them; contig reads, spliced and deleted ones, both strands"""
    lay = {5: (2, 24, 25, 61, 99), 6: (0, 13, 30, 49, 50, 88), 7: (1, 12, 26, 47, 63, 64, 98),
           12: (0, 5, 11, 24, 25, 33, 48, 62, 65, 74, 75, 99)}
    orders = ((33, 73, 34, 74, 35, 34, 126, 75, 33, 126, 35, 73), (126, 35, 75, 33, 74, 75, 34, 73, 126, 33, 74, 34))
    specs = []
    for k, at in lay.items():
        for v, vals in enumerate(orders):
            fq = _qual_bytes(100, at, vals)
            for gaps, gname in (((), "plain"), (((2, "N", 90),), "spliced"), (((1, "D", 3),), "deleted")):
                for anti in (False, True):
                    specs.append(Read("qual/k%d/q%d/%s" % (k, v, gname), anti=anti, subs=at, gaps=gaps, quals=fq))
                    # N among them, in front of the sixth: none of the three may take a quality slot
                    extra = dict(read_n=(at[3] + 2,), gen_n=(at[3] + 4, at[3] + 6), subs=at)
                    specs.append(Read("qual/k%d/q%d/%s/n" % (k, v, gname), anti=anti, gaps=gaps, quals=fq, **extra))
                    specs.append(Read("qual/k%d/q%d/%s/bothn" % (k, v, gname), anti=anti, gaps=gaps, quals=fq, subs=at,
                                      read_n=(at[2] + 3,), gen_n=(at[2] + 3,)))
    steep = params(bowtie2_min_penalty=2, bowtie2_max_penalty=42) if p is None else p      # a point of penalty per phred: 33, 34, 35 differ
    return [build_one(specs, p, seed), build_one(specs, steep, seed)]


PIECE_READ_LENGTHS = (64, 65, 100, 128, 129, 150, 192, 193, 250, 256, 257, 512)
PIECE_OFFSETS = (0, 63, 64, 127, 128, 191, 192)


def piece_edges_specs(rl: int):
    L = 32 if rl == 512 else 25
    edge = [f for f in PIECE_OFFSETS + (255, 256, 447, 448, 510) if f < rl - 1] + [rl - 1]
    specs = []
    for anti in (False, True):
        specs.append(Read("piece/rl%d/clean" % rl, rl=rl, L=L, anti=anti))
        for f in edge:
            specs.append(Read("piece/rl%d/at%d" % (rl, f), rl=rl, L=L, anti=anti, subs=(f,)))
        for f in edge:
            if f % 64 == 63 and f + 1 < rl:
                specs.append(Read("piece/rl%d/pair%d" % (rl, f), rl=rl, L=L, anti=anti, subs=(f, f + 1)))
        specs.append(Read("piece/rl%d/all" % rl, rl=rl, L=L, anti=anti, subs=tuple(edge)))
        # a junction / a deletion inside each 64-base piece of the read that holds a boundary
        seen = set()
        for b, pos in enumerate(boundaries(rl, L, anti), 1):
            if pos // 64 in seen or pos // 64 > 4:
                continue
            seen.add(pos // 64)
            around = tuple(sorted(set(f for f in (0, pos - 1, pos, pos + 63, pos + 64, rl - 1) + tuple(edge) if 0 <= f < rl)))
            specs.append(Read("piece/rl%d/spliced_in_piece%d" % (rl, pos // 64), rl=rl, L=L, anti=anti, subs=around, gaps=((b, "N", 80 + b, anti),)))
            specs.append(Read("piece/rl%d/deleted_in_piece%d" % (rl, pos // 64), rl=rl, L=L, anti=anti, subs=around[:12], gaps=((b, "D", 3),)))
    return specs


def piece_edges(rl: int, p: Optional[Params] = None):
    return build_one(piece_edges_specs(rl), p, 500 + rl)


def multihit(copies: int, p: Optional[Params] = None, seed: int = 606):
    """every third ladder pattern and the ones around the tail line's and the record's limits, on a tandem repeat"""
    if p is None and copies <= 4:
        # the copies lie 400 bases apart: with introns of up to 300 a hit chains with its own copy's next hit only and the read's chains
        # travel as chain entries (thj_k_chains); with the default 500 kb the read stays with the packed tier
        p = params(max_report_intron=300, max_segment_intron=300)
    specs = []
    for T, pats in ladder_patterns(1).items():
        if T % 3 == 0 or T in (23, 24, 25, 26, 39, 40, 41, 42):
            for anti in (False, True):
                specs.append(Read("multihit/md%d" % T, anti=anti, subs=pats[0]))
    return [build_repeat(specs, copies, seed + copies, p)]


# ------------------------------------------------------------------------------------------------ shared by the CPU and the GPU tests
# (offset, size) pairs of the MD buffer that no read reaches:
#   offset + size > 40     the string would pass the record's 40 characters (the host formats it: thj_md_string);
#   (36, 4)                a 4-character token is never the last one (the final run has at most three digits), so one more character follows;
#   offset 1               the first token is <run><letter>, two characters or more, or the string is the final run alone;
#   (0, 1), (2, 1)         a one-character token here ends a string of one or three characters: a read of under 20 bases.
MD_UNREACHABLE = {(o, n) for o in range(40) for n in (1, 2, 3, 4) if o + n > 40 or o == 1} | {(36, 4), (0, 1), (2, 1)}


@functools.lru_cache(maxsize=None)
def family(name: str):
    """the cases of a family by name (built once a process): "ladder", "sweep", "indels", "qualities", "piece<rl>", "multihit<copies>" """
    if name.startswith("piece"):
        return [piece_edges(int(name[5:]))]
    if name.startswith("multihit"):
        return multihit(int(name[8:]))
    return {"ladder": ladder, "sweep": sweep, "indels": indels, "qualities": qualities}[name]()


@functools.lru_cache(maxsize=None)
def expected(name: str):
    """the oracle's records of every case of the family (computed once a process, shared, never changed)"""
    import orc
    return tuple(tuple(orc.spanning(p, orc.Genome(seqs), sb, j, ins)) for seqs, sb, p, j, ins, _tags in family(name))


def explain(got, want, tags) -> str:
    """which planted read differs first"""
    if len(got) != len(want):
        have = {}
        for a in got:
            have[a.read_idx] = have.get(a.read_idx, 0) + 1
        for a in want:
            have[a.read_idx] = have.get(a.read_idx, 0) - 1
        bad = [tags[r] for r, d in sorted(have.items()) if d]
        return "%d records for %d: %s" % (len(got), len(want), bad[:6])
    for a, b in zip(got, want):
        if a != b:
            return "%s\n got  %r\n want %r" % (tags[b.read_idx], a, b)
    return "equal"
