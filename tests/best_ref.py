"""Test infrastructure: a plain-Python restatement of tophat_reports' choice among the alignments of a read, the single-end half --
read_best_alignments in both of its modes, the AlignStatus score and the --max-multihits cap with the reference's generator -- and of
the whole consensus with that choice made, as an extension of jbknown_ref.consensus / indelbed_ref.  Written from reading the reference,
each step citing its lines; nothing here runs on a GPU or calls the product.

A record is indelbed_ref's (ref_id, left, antisense_splice, [(op, len) ...][, ref_id2]).  What the choice reads beside it comes in
lists of the records' length: reads[i] = the number of record i's read (a read's records follow each other; numbers do not fall),
AS[i] = its AS:i, mism[i] = BowtieHit::mismatches() (jbknown_ref.mismatches), anti[i] = antisense_align().
best = (max_multihits, suppress_hits, bowtie2_max_penalty)."""
from __future__ import annotations

import indelbed_ref as ir
import jbknown_ref as jr

U32 = ir.U32
FUSION_OPS = (7, 8, 9, 10)


# ---- BowtieHit's own quantities
def ref_id2(rec):
    """HitFactory::create_hit, bwt_map.cpp:284-288: the first contig again unless the alignment names a second one"""
    return rec[4] if any(op in FUSION_OPS for op, _ in rec[3]) else rec[0]


def right(rec):
    """BowtieHit::right(), bwt_map.h:213-243 (all four fusion ops jump)"""
    r = ir._i32(rec[1])
    for op, ln in rec[3]:
        if op in (1, 11, 5):
            r += ln
        elif op in (2, 12, 6):
            r -= ln
        elif op in FUSION_OPS:
            r = ln
    return ir._i32(r)


def read_len(cig):
    """BowtieHit::read_len(), bwt_map.h:145-165: MATCH, mATCH, INS, iNS, SOFT_CLIP"""
    return sum(ln for op, ln in cig if op in (1, 2, 3, 4, 13))


def min_extent(cig):
    return min(read_len(cig) // 4, 10)                          # align_status.cpp:55-56


def order_key(rec, mism, anti):
    """BowtieHit::operator<, bwt_map.h:180-207 (the read id is equal within a read): tuples compare the way it does"""
    cig = [tuple(x) for x in rec[3]]
    return (rec[0], ref_id2(rec), ir._i32(rec[1]), 1 if anti else 0, mism, jr.edit_dist(mism, cig), len(cig), cig)


def equal_key(rec, mism, anti):
    """cmp_read_equal, tophat_reports.cpp:94-111: right instead of the cigar, no score"""
    return (rec[0], ref_id2(rec), ir._i32(rec[1]), right(rec), 1 if anti else 0, mism, jr.edit_dist(mism, rec[3]), len(rec[3]))


def sort_unique(idx, recs, mism, anti):
    """std::sort and std::unique(cmp_read_equal) (tophat_reports.cpp:161-163) over record numbers -> (sorted, survivors); records
    that compare equal under operator< are identical in everything the statistics read, their order does not show"""
    srt = sorted(idx, key=lambda k: order_key(recs[k], mism[k], anti[k]))
    out = []
    for k in srt:
        if not out or equal_key(recs[out[-1]], mism[out[-1]], anti[out[-1]]) != equal_key(recs[k], mism[k], anti[k]):
            out.append(k)
    return srt, out


# ---- the score
def score_juncs(rec):
    """the junctions AlignStatus asks about, align_status.cpp:59-85, :144-172, :271-278: the contig is always the alignment's first
    (junc.refid = bh.ref_id()), and every fusion op -- FUSION_RR too -- sets the position to its length"""
    ref, left, anti, cig = rec[:4]
    j, out = ir._i32(left), []
    for op, ln in cig:
        if op == 11:
            out.append((ref, (j - 1) & U32, (j + ln) & U32, 1 if anti else 0)); j += ln
        elif op == 12:
            out.append((ref, (j - ln) & U32, (j + 1) & U32, 1 if anti else 0)); j -= ln
        elif op in (1, 5):
            j += ln
        elif op in (2, 6):
            j -= ln
        elif op in FUSION_OPS:
            j = ln
    return out


def penalty(mp, support, le, re, me):
    """align_status.cpp:99-122 with avg_cov = 0 (the consensus worker's update_coverage calls are commented out,
    tophat_reports.cpp:2015, :2037): int penalty = mp + 2; penalty *= min(0 / support + extent_penalty, 1.f) when support >= 5"""
    p = mp + 2
    if support >= 5:
        p = int(p * min(0.0 + (0.5 if le < me or re < me else 0.0), 1.0))
    return p


def score(rec, AS, js1, known, mp):
    """AlignStatus::AlignStatus, align_status.cpp:40-284.  js1 = the first-pass JunctionSet {junction: [le, re, support]} with the
    annotation merged in; known = the annotation.  recalculate_indel_score is false: the indel branches are dead."""
    sc = AS
    if not js1:                                                 # :57 recalculate_score = !junctions.empty()
        return sc
    me = min_extent(rec[3])
    for j in score_juncs(rec):
        if j in known:
            sc += 2                                             # :136-139
        elif j not in js1:
            sc -= mp                                            # :93-96
        else:
            le, re, sup = js1[j]
            sc -= penalty(mp, sup, le, re, me)                  # (gtf_match, :118-119, is set only for junctions of the annotation: they took + 2)
    return sc


# ---- boost::mt19937 (the standard MT19937), written out
class Mt19937:
    def __init__(self, seed=1):
        s = [seed & U32]
        for i in range(1, 624):
            s.append((1812433253 * (s[-1] ^ (s[-1] >> 30)) + i) & U32)
        self.s, self.at = s, 624
        self.drawn = 0

    def __call__(self):
        s = self.s
        if self.at >= 624:
            for i in range(624):
                y = (s[i] & 0x80000000) | (s[(i + 1) % 624] & 0x7FFFFFFF)
                s[i] = s[(i + 397) % 624] ^ (y >> 1) ^ (0x9908B0DF if y & 1 else 0)
            self.at = 0
        y = s[self.at]
        self.at += 1
        self.drawn += 1
        y ^= y >> 11
        y ^= (y << 7) & 0x9D2C5680
        y ^= (y << 15) & 0xEFC60000
        y ^= y >> 18
        return y & U32


def groups(reads):
    """[(first, end)] of the runs of equal read numbers"""
    out, s = [], 0
    for i in range(1, len(reads) + 1):
        if i == len(reads) or reads[i] != reads[s]:
            out.append((s, i)); s = i
    return out


def choose(recs, reads, AS, mism, anti, best, min_anchor=8, known=(), limits=None):
    """both passes over all reads -> dict: rank[i] (place under operator< among the read's records under the limits, None for a
    dropped one), dup1[i] (the first pass's unique drops it), score[i] (None: filtered or excluded), keep[i] (reported), draws[(first
    record of a read over the cap)] = (number of the read's first draw in the generator's stream, survivors' places), stats = (reads,
    reads that lost records to the choice, reads over the cap, first-pass duplicates), accepted, js1"""
    n = len(recs)
    max_multihits, suppress, mp = best
    known = set(known)
    live = [not jr.dropped(mism[i], recs[i][3], limits) for i in range(n)]
    rank, dup1 = [None] * n, [False] * n
    grp = groups(reads)
    # pass 1 (final_report == false, tophat_reports.cpp:113-168): limits, sort, unique; no score is involved
    first = []
    for s, e in grp:
        idx = [i for i in range(s, e) if live[i]]
        srt, surv = sort_unique(idx, recs, mism, anti)
        for place, k in enumerate(srt):
            rank[k] = place
        for k in idx:
            dup1[k] = k not in surv
        first += sorted(surv)
    js1 = {}
    for k in first:
        for (ref, l, rt, a, le, re) in ir.rec_juncs(recs[k]):
            ir._merge(js1, (ref, l, rt, a), le, re)
    for k in known:
        js1.setdefault(k, [0, 0, 0])                            # merge_with(junctions, gtf_junctions), tophat_reports.cpp:2814
    _state, accepted = jr.first_pass([recs[k] for k in first], min_anchor, known)
    # pass 2 (:2283-2313), from the raw records
    rng = Mt19937(1)                                            # rng.seed(1) per worker, :2325
    sc, keep, draws = [None] * n, [False] * n, {}
    n_lost = n_over = 0
    for s, e in grp:
        cand = [i for i in range(s, e) if live[i] and ir.kept(recs[i], accepted)]      # :133-136, :1194-1229
        for i in cand:
            sc[i] = score(recs[i], AS[i], js1, known, mp)
        top = max((sc[i] for i in cand), default=None)
        ties = [i for i in cand if sc[i] == top]                # :141-157, in input order
        _srt, left = sort_unique(ties, recs, mism, anti)        # :161-163
        if any(live[i] and i not in left for i in range(s, e)):
            n_lost += 1
        if len(left) > max_multihits:                           # :170-208
            n_over += 1
            if suppress:
                left = []
            else:
                at = rng.drawn
                tie = list(range(len(left)))
                while len(tie) > max_multihits:
                    del tie[rng() % len(tie)]
                draws[s] = (at, tie)
                left = [left[t] for t in tie]
        if left:
            rng()                                               # print_sam_for_single, :1005-1007: rng() % hits.size()
        for i in left:
            keep[i] = True
    return {"rank": rank, "dup1": dup1, "score": sc, "keep": keep, "draws": draws, "stats": (len(grp), n_lost, n_over, sum(dup1)),
            "accepted": accepted, "js1": js1}


def consensus(recs, seqs=None, min_anchor=8, known=(), limits=None, mism=None, best=None, reads=None, AS=None, anti=None):
    """jbknown_ref.consensus with the choice made: -> (junctions, insertions, deletions) in indelbed_ref.consensus's forms.  best =
    None: jbknown_ref.consensus itself."""
    mism = [0] * len(recs) if mism is None else mism
    if best is None:
        return jr.consensus(recs, seqs, min_anchor, known, limits, mism)
    anti = [False] * len(recs) if anti is None else anti
    ch = choose(recs, reads, AS, mism, anti, best, min_anchor, known, limits)
    js, ins, dels, letters = {}, {}, {}, {}
    for k, r in enumerate(recs):
        if not ch["keep"][k]:
            continue
        for (ref, l, rt, a, le, re) in ir.rec_juncs(r):        # update_junctions, update_insertions_and_deletions, :2286-2313
            ir._merge(js, (ref, l, rt, a), le, re)
        if seqs is not None:
            for (ref, l, s, le, re, _c) in ir.rec_inss(r, seqs[k]):
                key = (ref, l, len(s))
                letters.setdefault(key, s)
                ir._merge(ins, key, le, re)
        for (ref, l, rt, le, re, _c) in ir.rec_dels(r):
            ir._merge(dels, (ref, l, rt), le, re)
    jout = [k + tuple(js[k]) for k in sorted(js) if js[k][2] > 0 and js[k][0] >= 8 and js[k][1] >= 8]          # :2974-2984
    iout = [(k[0], k[1], letters[k]) + tuple(ins[k]) for k in sorted(ins)]
    dout = [k + tuple(dels[k]) for k in sorted(dels)]
    return jout, iout, dout
