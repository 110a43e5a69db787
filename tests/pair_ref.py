"""Test infrastructure: a plain-Python restatement of tophat_reports' choice among the alignments of an INSERT -- pair_best_alignments in
both of its modes (tophat_reports.cpp:358-576), the InsertAlignmentGrade score with its too_far rescue (inserts.h:72-184), the visit
order of its two callers (:2002-2097, :2388-2594), the cap over pairs and the generator's draws -- and of the junction consensus with
that choice made, on top of best_ref.py.  Written from reading the reference, each step citing its lines; nothing here runs on a GPU
or calls the product.

A side is best_cases' form: recs, reads (the INSERT's number of every record; a read's records follow each other, numbers do not
fall), AS, mism, anti.  pair = (inner_dist_mean, inner_dist_std_dev, fusion_min_dist, report_mixed, report_discordant); best =
(max_multihits, suppress_hits, bowtie2_max_penalty).  fusion_search is false, report_secondary_alignments is false.

std::sort of a list of more than 16 pairs is not restated: tests/pairsim prints the order libstdc++ gives for a sequence of scores."""
from __future__ import annotations

import bisect
import os
import subprocess

import best_ref as br
import indelbed_ref as ir
import jbknown_ref as jr

HERE = os.path.dirname(os.path.abspath(__file__))
PAIRSIM = os.path.join(HERE, "pairsim", "pairsim")
TRACE = None                                                    # a list: pair_best appends what tests/pairsim needs to redo every insert
SEEN = None                                                     # a dict: mechanism -> the inserts it acted on (the crowd's self-check)
_built, _cur = [], [None]


def _saw(what):
    if SEEN is not None:
        SEEN.setdefault(what, set()).add(_cur[0])


def cdiv(a, b):
    """C++ integer division (truncation toward zero)"""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b >= 0) else -q


def sort_order(scores):
    """std::sort(best_hits, cmp_pair_alignment): -> order[place] = entry.  Up to 16 entries libstdc++ runs an insertion sort: ties stand
    in generation order.  A longer list: the order pairsim's std::sort gives on the same scores with the same comparator."""
    n = len(scores)
    if n <= 16:
        return sorted(range(n), key=lambda k: -scores[k])
    if not _built:
        from locked_make import locked_make
        locked_make(os.path.dirname(PAIRSIM))
        _built.append(True)
    out = subprocess.run([PAIRSIM, "order"], input=" ".join(str(s) for s in scores), capture_output=True, text=True, check=True).stdout
    order = [int(x) for x in out.split()]
    assert sorted(order) == list(range(n))
    return order


class Hit:
    """what the grade reads of an alignment"""

    def __init__(self, side, k, score):
        rec = side["recs"][k]
        self.k, self.ref, self.left, self.right = k, rec[0], ir._i32(rec[1]), br.right(rec)
        self.anti, self.fused, self.score = bool(side["anti"][k]), any(op in br.FUSION_OPS for op, _ in rec[3]), score
        self.eq = br.equal_key(rec, side["mism"][k], side["anti"][k])


def inner_dist(h1, h2):
    """pair_distances().second, inserts.cpp:105-132"""
    if h1.left <= h2.left and h1.right >= h2.right:
        return 0
    if h2.left <= h1.left and h2.right >= h1.right:
        return 0
    return h2.left - h1.right if h1.left < h2.left else h1.left - h2.right


def is_fusion(lh, rh, fusion_min_dist):
    """is_fusion_insert_alignment, tophat_reports.cpp:217-247"""
    if lh.fused or rh.fused:
        return True
    if lh.ref != rh.ref:
        return True
    if lh.anti == rh.anti:
        return True
    d = lh.left - rh.left if lh.anti else rh.left - lh.left   # left() on purpose (:235-236)
    return d < 0 or d > fusion_min_dist


def rescued(h1, h2, junctions, keys, lo, hi):
    """inserts.h:111-150 over the JunctionSet handed in ({junction: [le, re, support]}, keys = sorted(junctions))"""
    if h1.left < h2.left:
        inner1, inner2 = h1.right, h2.left
    else:
        inner1, inner2 = h2.right, h1.left
    lb = bisect.bisect_right(keys, (h1.ref, inner1 & ir.U32, inner1 & ir.U32, 1))
    ub = bisect.bisect_left(keys, (h1.ref, inner2 & ir.U32, inner2 & ir.U32, 0))
    while lb != ub and lb != len(keys):
        j = keys[lb]
        if inner1 <= ir._i32(j[1]) and inner2 >= ir._i32(j[2]) and junctions[j][2] >= 10:
            if lo <= ir._i32(j[1]) - inner1 + inner2 - ir._i32(j[2]) <= hi:
                return True
        lb += 1
    return False


def grade(lh, rh, junctions, keys, pair, mp):
    """set_insert_alignment_grade + InsertAlignmentGrade(h1, h2, junctions, fusion) -> None (not allowed) or (score, fusion)"""
    mean, sd, fmd = pair[:3]
    if lh.fused and rh.fused:                                   # :251-254
        _saw("not_allowed")
        return None
    fusion = is_fusion(lh, rh, fmd)
    if fusion:
        _saw("fusion_op" if lh.fused or rh.fused else "fusion_contig" if lh.ref != rh.ref else "fusion_strand" if lh.anti == rh.anti else "fusion_distance")
    lo, hi = mean - sd, mean + sd                               # inserts.h:87-88
    inner = inner_dist(lh, rh)
    too_far, too_close = inner > hi, inner < lo                 # :100-101
    if too_far and not fusion and rescued(lh, rh, junctions, keys, lo, hi):
        too_far = False
        _saw("rescued")
    if not fusion:
        _saw("contained" if inner == 0 else "too_far_half" if too_far and inner - hi < sd else "too_far_full" if too_far else "too_close" if too_close else "in_window")
    sc = lh.score + rh.score                                    # :155
    if not fusion:
        if too_far:
            sc -= mp // 2 if inner - hi < sd else mp            # :158-167
        elif too_close:
            sc -= min(mp // 2, cdiv(lo - inner, sd) + 1)        # :168-173
        if lh.anti == rh.anti:
            sc -= mp                                            # :175-177
    else:
        sc -= mp                                                # :179-183, fusion_search false
    return sc, fusion


def pair_best(L, R, lidx, ridx, lscore, rscore, junctions, keys, pair, best, final_report, rng):
    """pair_best_alignments over the records lidx / ridx (the hit groups as handed in, under the limits already), their scores ->
    (best_hits [(li, ri, score)], best grade is a fusion grade, over the cap).  tophat_reports.cpp:385-576"""
    max_multihits, suppress, mp = best
    discordant = pair[4]
    rhits = [Hit(R, k, rscore[k]) for k in ridx[:2 * max_multihits + 1]]      # (nhits >> 1) > max_multihits breaks at the 2M + 2nd
    hits, best_score, best_fusion = [], None, False
    drawn0 = rng.drawn if rng else 0
    cands = []
    for k in lidx[:2 * max_multihits + 1]:
        lh = Hit(L, k, lscore[k])
        for rh in rhits:
            g = grade(lh, rh, junctions, keys, pair, mp)
            cands.append((lh, rh, g))
            if g is None:
                continue
            sc, fusion = g
            new_best = best_score is None or best_score < sc    # :443-447 (a default grade has num_mapped 0: below every pair)
            if new_best:
                best_score, best_fusion = sc, fusion
            if fusion and not discordant:                       # :449
                continue
            if not final_report:
                hits.append((lh, rh, sc, len(cands) - 1))
            elif new_best:
                hits = [(lh, rh, sc, len(cands) - 1)]
            elif not sc < best_score:
                hits.append((lh, rh, sc, len(cands) - 1))
    order = sort_order([h[2] for h in hits])                    # :472-475
    hits = [hits[k] for k in order]
    uniq = []
    for h in hits:                                              # :496-497 cmp_pair_equal
        if uniq and uniq[-1][0].eq == h[0].eq and uniq[-1][1].eq == h[1].eq:
            continue
        uniq.append(h)
    if len(lidx) > 2 * max_multihits + 1 or len(ridx) > 2 * max_multihits + 1:
        _saw("side_cut")
    if len(uniq) < len(hits):
        _saw("pair_duplicates")
    if len(hits) > 16:
        _saw("host_sort")
    if final_report and len({h[2] for h in uniq}) > 1:
        _saw("two_scores")
    hits = uniq                                                 # (the first pass sorts again, :519-524: the statistics do not read the order)
    over = False
    if final_report:
        over = len(hits) > max_multihits
        if over and suppress:
            hits = []
        if len(hits) > max_multihits:                           # :538-571
            tie_score = hits[max_multihits - 1][2]
            ties, better = [], 0
            for i, h in enumerate(hits):
                if h[2] == tie_score:
                    ties.append(i)
                elif h[2] < tie_score:
                    break
                else:
                    better += 1
            _saw("cap_draws")
            if better:
                _saw("cap_pairs_above_the_ties")
            while better + len(ties) > max_multihits:
                del ties[rng() % len(ties)]
            hits = hits[:better] + [hits[i] for i in ties]
            hits = hits[:max_multihits]
    if TRACE is not None:
        TRACE.append(dict(final=final_report, juncs=[k[:3] + (junctions[k][2],) for k in keys if junctions[k][2] >= 10], drawn=drawn0, cands=cands,
                          kept=[h[3] for h in hits], best_fusion=best_fusion, over=over, used=(rng.drawn if rng else 0) - drawn0))
    return [(h[0].k, h[1].k, h[2]) for h in hits], best_fusion, over


def inserts(L, R):
    """the merge of :2002-2097 / :2388-2594 -> [(number, left records, right records)] in visit order"""
    gl = {L["reads"][s]: list(range(s, e)) for s, e in br.groups(L["reads"])}
    gr = {R["reads"][s]: list(range(s, e)) for s, e in br.groups(R["reads"])}
    return [(k, gl.get(k, []), gr.get(k, [])) for k in sorted(set(gl) | set(gr))]


def single_first(S, idx):
    """read_best_alignments, first pass (best_ref.choose's): limits applied by the caller, sort, unique"""
    return br.sort_unique(idx, S["recs"], S["mism"], S["anti"])[1]


def choose(L, R, best, pair, min_anchor=8, known=(), limits=None):
    """both passes -> dict: first = [(side, record)] with multiplicity (what feeds the first-pass statistics), final = the same for the
    final sets, lists = {insert number: [(left record, right record, score)]} of the second pass, counts = the five of
    thj_juncbed_pair_counts, drawn = the generator's outputs used"""
    max_multihits, suppress, mp = best
    mixed, discordant = pair[3], pair[4]
    known = set(known)
    sides = {"L": L, "R": R}
    live = {s: [not jr.dropped(S["mism"][i], S["recs"][i][3], limits) for i in range(len(S["recs"]))] for s, S in sides.items()}
    ins = inserts(L, R)
    # ---- first pass: the annotation is the set the grade searches; its entries have support 0
    gtf = {k: [0, 0, 0] for k in known}
    gkeys = sorted(gtf)
    first = []
    for _num, li, ri in ins:
        _cur[0] = ("first", _num)
        if li and ri:
            lid, rid = [k for k in li if live["L"][k]], [k for k in ri if live["R"][k]]
            hits, _bf, _ov = pair_best(L, R, lid, rid, L["AS"], R["AS"], gtf, gkeys, pair, best, False, None)
            if hits:
                first += [("L", h[0]) for h in hits] + [("R", h[1]) for h in hits]
                if len(hits) > len({h[0] for h in hits}) or len(hits) > len({h[1] for h in hits}):
                    _saw("record_in_several_pairs")
            else:                                               # :2075-2079: the hit groups as they came
                first += [("L", k) for k in li] + [("R", k) for k in ri]
                _saw("no_pair_in_the_first_pass")
                if len(lid) < len(li) or len(rid) < len(ri):
                    _saw("no_pair_unfiltered")
        else:
            s, idx = ("L", li) if li else ("R", ri)
            first += [(s, k) for k in sorted(single_first(sides[s], [k for k in idx if live[s][k]]))]
    first_recs = [sides[s]["recs"][k] for s, k in first]
    js1 = {}
    for r in first_recs:
        for (ref, l, rt, a, le, re) in ir.rec_juncs(r):
            ir._merge(js1, (ref, l, rt, a), le, re)
    for k in known:
        js1.setdefault(k, [0, 0, 0])                            # merge_with(junctions, gtf_junctions), :2814
    keys1 = sorted(js1)
    _state, accepted = jr.first_pass(first_recs, min_anchor, known)
    # ---- second pass
    rng = br.Mt19937(1)
    final, lists = [], {}
    n_both = n_rep = n_over = n_single = n_dropped = 0

    def left_of(s, idx):                                        # exclude_hits_on_filtered_junctions (:1194-1229) and the limits
        S = sides[s]
        return [k for k in idx if live[s][k] and ir.kept(S["recs"][k], accepted)]

    def single(s, idx):
        """write_singleton_alignments (:2229-2322) -> the read_best_alignments of best_ref.choose's second pass, one read"""
        nonlocal final
        S = sides[s]
        cand = left_of(s, idx)
        sc = {k: br.score(S["recs"][k], S["AS"][k], js1, known, mp) for k in cand}
        top = max(sc.values(), default=None)
        ties = [k for k in cand if sc[k] == top]
        _srt, left = br.sort_unique(ties, S["recs"], S["mism"], S["anti"])
        if len(left) > max_multihits:
            if suppress:
                left = []
            else:
                tie = list(range(len(left)))
                while len(tie) > max_multihits:
                    del tie[rng() % len(tie)]
                left = [left[t] for t in tie]
        if left:
            rng()                                               # print_sam_for_single
        final += [(s, k) for k in left]

    for num, li, ri in ins:
        _cur[0] = ("second", num)
        if not (li and ri):
            n_single += 1
            s, idx = ("L", li) if li else ("R", ri)
            if mixed:
                single(s, idx)
            elif left_of(s, idx):                               # :2266-2280: the user only wants paired alignments reported
                n_dropped += 1
            continue
        n_both += 1
        lid, rid = left_of("L", li), left_of("R", ri)
        paired = bool(lid) and bool(rid)                        # :2434-2435 (the limits: see thj.h -- the same ways out)
        hits = []
        if paired:
            lsc = {k: br.score(L["recs"][k], L["AS"][k], js1, known, mp) for k in lid}
            rsc = {k: br.score(R["recs"][k], R["AS"][k], js1, known, mp) for k in rid}
            hits, best_fusion, over = pair_best(L, R, lid, rid, lsc, rsc, js1, keys1, pair, best, True, rng)
            n_over += over
            if over:
                _saw("over_the_cap")
            if mixed and (not hits or (best_fusion and not discordant)):      # :2488-2493
                paired = False
                _saw("mixed_fusion_grade" if hits else "mixed_empty_list")
        elif not mixed:
            n_dropped += bool(lid) + bool(rid)
            if lid or rid:
                _saw("mate_has_nothing_left")
        if paired:
            if hits:
                lists[num] = hits
                n_rep += 1
                final += [("L", h[0]) for h in hits] + [("R", h[1]) for h in hits]      # :2509-2519
                rng()                                           # print_sam_for_pair, :1055-1056
        elif mixed:
            if lid:
                single("L", li)
            if rid:
                single("R", ri)
    return {"first": first, "final": final, "lists": lists, "counts": (n_both, n_rep, n_over, n_single, n_dropped), "drawn": rng.drawn, "js1": js1,
            "accepted": accepted}


def consensus(L, R, best, pair, min_anchor=8, known=(), limits=None, seqs=None):
    """-> the junction rows of junctions.bed (indelbed_ref.consensus's form) with the choice among pairs made; with seqs = {"L": [SEQ of every
    left record], "R": [...]}: (junction rows, insertion rows, deletion rows).  choose()'s final list is the reference's order of observation
    (inserts in visit order; per insert the left records in pair-list order, then the right ones, :2502-2519): the first insertion seen at a
    place with a length keeps its letters."""
    ch = choose(L, R, best, pair, min_anchor, known, limits)
    sides = {"L": L, "R": R}
    js, ins, dels, letters = {}, {}, {}, {}
    for s, k in ch["final"]:
        r = sides[s]["recs"][k]
        for (ref, l, rt, a, le, re) in ir.rec_juncs(r):
            ir._merge(js, (ref, l, rt, a), le, re)
        if seqs is not None:
            for (ref, l, sq, le, re, _c) in ir.rec_inss(r, seqs[s][k]):
                key = (ref, l, len(sq))
                letters.setdefault(key, sq)
                ir._merge(ins, key, le, re)
            for (ref, l, rt, le, re, _c) in ir.rec_dels(r):
                ir._merge(dels, (ref, l, rt), le, re)
    jout = [k + tuple(js[k]) for k in sorted(js) if js[k][2] > 0 and js[k][0] >= 8 and js[k][1] >= 8]          # :2974-2984
    if seqs is None:
        return jout
    return jout, [(k[0], k[1], letters[k]) + tuple(ins[k]) for k in sorted(ins)], [k + tuple(dels[k]) for k in sorted(dels)]
