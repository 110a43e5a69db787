"""Test infrastructure: a plain-Python restatement of how tophat_reports writes the reported alignments of an INSERT into
accepted_hits.bam -- print_sam_for_pair (tophat_reports.cpp:1027-1089), rewrite_sam_record's paired overload (:783-960), its unpaired
overload with FRAG_LEFT / FRAG_RIGHT for the sides --report-mixed-alignments sends down the single-end way (:656-781, :2565-2585),
add_auxData's side rule (:580-654) and InsertAlignmentGrade::happy() of the best grade (inserts.h:72-221) -- THROUGH THE SAM TEXT, on
accepted_ref.py's tokens and records and pair_ref.py's choice.  Written from reading the reference; nothing here runs on a GPU or
calls the product.

pair_ref.choose hands out the junction rows' records only.  watched_choose() runs it unchanged and watches it from outside: the
generator it seeds (every draw with the insert it was drawn for), best_ref.sort_unique (once per side that goes the single-end way)
and pair_ref.TRACE (the graded candidates of every second-pass pair_best).

A side of a case is best_cases' form (a record is (contig, left, antisense_splice, cigar ops[, ...])); raw = {"L": [...], "R": [...]}: the
BAM record of every record, WITH its block_size field.  cfg as accepted_ref's: library_type, rg, names, header."""
from __future__ import annotations

import struct

import accepted_ref as ar
import best_ref as br
import pair_ref as pr
from accepted_ref import Loud  # noqa: F401
from best_cases import M

UNPAIRED, LEFT, RIGHT = 0, 1, 2


# ---- the decisions the device shares with this file
def spliced(rec):
    """not BowtieHit::contiguous() (bwt_map.h:496-499)"""
    return not (len(rec[3]) == 1 and rec[3][0][0] == M)


def happy(lrec, lanti, rrec, ranti, too_far):
    """inserts.h:93-103, :218-221 with num_mapped == 2"""
    num_spliced = int(spliced(lrec)) + int(spliced(rrec))
    consistent = num_spliced == 2 and bool(lrec[2]) == bool(rrec[2])
    return (bool(lanti) != bool(ranti)) and (num_spliced != 2 or consistent) and not too_far


def tlen(left, right, p_left, p_right):
    """:864-875, same contig"""
    if left <= p_left and right >= p_right and right - left > p_right - p_left:
        return right - left
    if p_left <= left and p_right >= right and p_right - p_left > right - left:
        return p_left - p_right
    return p_right - left if left < p_left else p_left - right


def xs_sign(library_type, anti, side):
    """add_auxData, :615-647 -> '+', '-' or None"""
    if library_type == ar.FR_FIRSTSTRAND:
        plus = anti
    elif library_type == ar.FR_SECONDSTRAND:
        plus = not anti
    else:
        return None
    if side == RIGHT:
        plus = not plus
    return "+" if plus else "-"


# ---- one record
def rewrite(d, cfg, hit, n, nxt, primary, hit_index, side, partner, is_happy):
    """both rewrite_sam_record overloads + add_auxData.  d: the input record without its block_size field; hit / partner / nxt: dicts
    with ref, left, right, anti, score (partner None: the unpaired overload)"""
    names = cfg["names"]
    toks = ar.sam_tokens(d, names[hit["ref"] - 1])
    for i in range(11, len(toks)):
        if toks[i].startswith("XF"):
            raise Loud("fusion")
        if toks[i].startswith("AS"):
            toks[i] = "AS:i:%d" % min(0, hit["score"])
    qname = toks[0]
    sl = qname.rfind("/")
    if sl >= 0 and len(qname) - sl < 4:
        qname = qname[:sl]
    if names[hit["ref"] - 1] not in cfg["header"]:
        raise Loud("contig")
    tid = cfg["header"].index(names[hit["ref"] - 1])
    flag = int(toks[1])
    mtid, mate_pos, tl = -1, int(toks[7]), int(toks[8])
    if partner is None:
        if side != UNPAIRED:                                 # :717-729
            flag |= 0x1 | (0x40 if side == LEFT else 0x80) | 0x8
        if not primary:
            flag |= 0x100
    else:
        flag |= 0x1 | (0x40 if side == LEFT else 0x80)       # :805-814
        if not primary:
            flag |= 0x100
        tl = 0
        if partner["ref"] == hit["ref"]:
            mtid = tid                                        # "="
            tl = tlen(hit["left"], hit["right"], partner["left"], partner["right"])
        else:
            pname = names[partner["ref"] - 1]
            mtid = cfg["header"].index(pname) if pname in cfg["header"] else -1
        mate_pos = partner["left"] + 1
        if is_happy:
            flag |= 0x2
        if partner["anti"]:
            flag |= 0x20
    aux, xs_found = [], False
    for t in toks[11:]:
        if "NH:i:" not in t and "XS:i:" not in t:
            aux.append(t)
        if "XS:A:" in t:
            xs_found = True
    aux.append("NH:i:%d" % n)
    if nxt is not None:
        aux.append("CC:Z:" + ("=" if nxt["ref"] == hit["ref"] else names[nxt["ref"] - 1]))
        aux.append("CP:i:%d" % (nxt["left"] + 1))
    if not xs_found:
        sign = xs_sign(cfg["library_type"], hit["anti"], side)
        if sign:
            aux.append("XS:A:" + sign)
    if hit_index >= 0:
        aux.append("HI:i:%d" % hit_index)
    if cfg.get("rg"):
        aux.append("RG:Z:" + cfg["rg"])
    out = bytearray(ar.new_record(qname, flag, tid, int(toks[3]), ar.mapq(n), toks[5], mate_pos, tl, toks[9], toks[10], aux))
    struct.pack_into("<i", out, 4 + 20, mtid)
    if len(out) > 65536:
        raise Loud("big")
    return bytes(out)


def hit_of(S, raw, k, score):
    rec = S["recs"][k]
    d = raw[k][4:]
    return dict(ref=rec[0], left=pr.ir._i32(rec[1]), right=br.right(rec), anti=bool(struct.unpack_from("<H", d, 14)[0] & 0x10), score=score, d=d)


def print_sam_for_pair(pairs, draw, is_happy, cfg, big_order=None):
    """pairs = [(left hit, right hit)] = best_hits -> the records: per pair in index_vector order its right record, then its left one"""
    n = len(pairs)
    iv = ar.index_vector([(r["ref"], r["left"]) for _l, r in pairs], big_order)
    primary = draw % n
    out = []
    for p, k in enumerate(iv):
        lh, rh = pairs[k]
        nl, nr = pairs[iv[p + 1]] if p + 1 < n else (None, None)
        hi = p if n > 1 else -1
        out.append(rewrite(rh["d"], cfg, rh, n, nr, k == primary, hi, RIGHT, lh, is_happy))
        out.append(rewrite(lh["d"], cfg, lh, n, nl, k == primary, hi, LEFT, rh, is_happy))
    return out


def print_sam_for_single(hits, draw, side, cfg, big_order=None):
    n = len(hits)
    iv = ar.index_vector([(h["ref"], h["left"]) for h in hits], big_order)
    primary = draw % n
    return [rewrite(hits[k]["d"], cfg, hits[k], n, hits[iv[p + 1]] if p + 1 < n else None, k == primary, p if n > 1 else -1, side, None, False) for p, k in enumerate(iv)]


# ---- pair_ref.choose, watched
def watched_choose(L, R, best, pair, min_anchor=8, known=(), limits=None):
    """-> (pair_ref.choose's dict, plan): plan = per insert that writes anything, in visit order, ("pairs", number, [(left record, right
    record)], primary draw, happy of the best grade) or ("side", number, "L" | "R", [records in hits order], primary draw)"""
    events, traces = [], []
    real_rng, real_su, real_trace = br.Mt19937, br.sort_unique, pr.TRACE

    class Rng(real_rng):
        def __call__(self):
            v = real_rng.__call__(self)
            events.append((pr._cur[0], "draw", v))
            return v

    def su(idx, recs, mism, anti):
        out = real_su(idx, recs, mism, anti)
        events.append((pr._cur[0], "side", None))
        return out

    class Trace(list):
        def append(self, t):
            if t["final"]:
                traces.append((pr._cur[0], t))

    br.Mt19937, br.sort_unique, pr.TRACE = Rng, su, Trace()
    try:
        ch = pr.choose(L, R, best, pair, min_anchor, known, limits)
    finally:
        br.Mt19937, br.sort_unique, pr.TRACE = real_rng, real_su, real_trace
    mean, sd = pair[0], pair[1]
    keys1 = sorted(ch["js1"])
    grades = {}
    for cur, t in traces:
        top, is_happy = None, False
        for lh, rh, g in t["cands"]:                           # :441-447: the first candidate that raises the running best is best_grade
            if g is None:
                continue
            sc, fusion = g
            if top is None or top < sc:
                top = sc
                too_far = pr.inner_dist(lh, rh) > mean + sd
                if too_far and not fusion and pr.rescued(lh, rh, ch["js1"], keys1, mean - sd, mean + sd):
                    too_far = False
                is_happy = happy(L["recs"][lh.k], lh.anti, R["recs"][rh.k], rh.anti, too_far)
        grades[cur[1]] = is_happy
    # the final records by insert (an insert's left records, then its right records; inserts in visit order)
    sides = {"L": L, "R": R}
    by_ins = {}
    for s, k in ch["final"]:
        by_ins.setdefault(sides[s]["reads"][k], {"L": [], "R": []})[s].append(k)
    ev_of = {}
    for cur, kind, v in events:
        if cur[0] == "second":
            ev_of.setdefault(cur[1], []).append((kind, v))
    plan = []
    for num, _li, _ri in pr.inserts(L, R):
        evs = ev_of.get(num, [])
        if num in ch["lists"]:
            draws = [v for kind, v in evs if kind == "draw"]
            plan.append(("pairs", num, [(h[0], h[1]) for h in ch["lists"][num]], draws[-1], grades[num]))
            continue
        if num not in by_ins:
            continue
        # the sides that went the single-end way: every call of single() is a "side" event, then its cap draws, then its own draw
        segs, cur_seg = [], None
        for kind, v in evs:
            if kind == "side":
                cur_seg = []
                segs.append(cur_seg)
            elif cur_seg is not None:
                cur_seg.append(v)
        reporting = [s for s in ("L", "R") if by_ins[num][s]]
        with_draws = [sg for sg in segs if sg]
        assert len(with_draws) == len(reporting), (num, segs, reporting)
        for s, sg in zip(reporting, with_draws):
            plan.append(("side", num, s, by_ins[num][s], sg[-1]))
    return ch, plan


def accepted(c, raw, cfg, big_order=None):
    """c: a pair_cases-style case -> (the output records in order, what was seen: {"pairs", "sides", "big", "happy"})"""
    L, R = c["L"], c["R"]
    ch, plan = watched_choose(L, R, c["best"], c["pair"], c.get("anchor", 8), c.get("known", ()), c.get("limits"))
    mp = c["best"][2]
    known = set(c.get("known", ()))
    sides = {"L": L, "R": R}

    def hit(s, k):
        S = sides[s]
        return hit_of(S, raw[s], k, br.score(S["recs"][k], S["AS"][k], ch["js1"], known, mp))

    out, seen = [], {"pairs": 0, "sides": 0, "big": 0, "happy": 0}
    for item in plan:
        if item[0] == "pairs":
            _kind, _num, hits, draw, is_happy = item
            seen["pairs"] += 1
            seen["happy"] += bool(is_happy)
            seen["big"] += len(hits) > ar.SORT_THRESHOLD
            out += print_sam_for_pair([(hit("L", a), hit("R", b)) for a, b in hits], draw, is_happy, cfg, big_order)
        else:
            _kind, _num, s, ks, draw = item
            seen["sides"] += 1
            seen["big"] += len(ks) > ar.SORT_THRESHOLD
            out += print_sam_for_single([hit(s, k) for k in ks], draw, LEFT if s == "L" else RIGHT, cfg, big_order)
    return out, seen
