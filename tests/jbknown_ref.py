"""Test infrastructure: a plain-Python restatement of tophat_reports' consensus with its two further inputs -- the annotated
junctions (--gtf-juncs) and the read filter (--read-mismatches / --read-gap-length / --read-edit-dist) -- written from reading the
reference, each step citing its lines; nothing here runs on a GPU or calls the product.  The record walks are indelbed_ref's.

A record is indelbed_ref's (ref_id, left, antisense_splice, [(op, len) ...][, ref_id2]); a junction is (ref, left, right, antisense).
What the filter reads of a record is its `mismatches` (BowtieHit::mismatches()) and its cigar; mismatches() itself comes from
(NM, cigar) the way the BAM factory makes it."""
from __future__ import annotations

import bisect

import indelbed_ref as ir

U32 = ir.U32
REJECTED, VALID, KNOWN = 0, 1, 2                                # the three states filter_junctions' loop leaves a junction in


def mismatches(nm, cig):
    """BAMHitFactory::get_hit_from_buf: unsigned char num_mismatches = 0 (bwt_map.cpp:1175); = bam_aux2i(NM) when the tag is there
    (:1185-1188); -= length for every INS and every DEL of the cigar it builds (:1362-1365; a fusion alignment's, rebuilt from
    XF:Z: :1282-1285) -- upper case only, modulo 256"""
    v = (0 if nm is None else nm) & 0xFF
    for op, ln in cig:
        if op in (3, 5):
            v = (v - ln) & 0xFF
    return v


def gap_length(cig):
    """bwt_map.cpp:32-43: INS, iNS, DEL, dEL"""
    return sum(ln for op, ln in cig if op in (3, 4, 5, 6))


def edit_dist(mism, cig):
    """num_mismatches + gap_length(cigar) into BowtieHit's unsigned char (bwt_map.cpp:1429-1430)"""
    return (mism + gap_length(cig)) & 0xFF


def dropped(mism, cig, limits):
    """tophat_reports.cpp:133-136 (read_best_alignments) and :1202-1205 (exclude_hits_on_filtered_junctions); limits =
    (read_mismatches, read_gap_length, read_edit_dist) or None: no filter"""
    if limits is None:
        return False
    return mism > limits[0] or gap_length(cig) > limits[1] or edit_dist(mism, cig) > limits[2]


def first_pass(recs, min_anchor=8, known=()):
    """the first-pass JunctionSet of the records, merge_with(junctions, gtf_junctions) (tophat_reports.cpp:2814) and filter_junctions
    (junctions.cpp:305-318) -> ({junction: REJECTED | VALID | KNOWN} after the loop, {junction: accepted} after the knockout).
    Junctions of the annotation nobody shows are in both, with support 0, as in the reference."""
    known = set(known)
    js = {}
    for r in recs:
        for (ref, l, rt, a, le, re) in ir.rec_juncs(r):
            ir._merge(js, (ref, l, rt, a), le, re)
    for k in known:                                             # JunctionStats(): extents 0, supporting_hits 0 (junctions.h:83-84)
        js.setdefault(k, [0, 0, 0])
    state = {}
    for k, (le, re, sup) in js.items():
        if k in known:                                          # :311-314: accepted = gtf_match = true, accept_if_valid is not asked
            state[k] = KNOWN
            continue
        mn = min(le, re)                                        # accept_if_valid, :192-240
        if mn < min_anchor:
            state[k] = REJECTED
        elif ir._i32(k[2]) - ir._i32(k[1]) > 50000:
            state[k] = VALID if sup >= 2 and mn > 12 else REJECTED
        else:
            state[k] = VALID
    keys = sorted(js)
    out = {k: state[k] != REJECTED for k in keys}
    for k in keys:                                              # knockout_shadow_junctions, :242-303
        if state[k] != VALID:                                   # :270: accepted && !gtf_match
            continue
        ref, l, rt, a = k
        lo = (ref, (l - min_anchor) & U32, rt, 1 - a)           # fuzzy_left / fuzzy_right, :272-277 (unsigned: see indelbed_ref.first_pass)
        hi = (ref, l, (rt + min_anchor) & U32, 1 - a)
        for k2 in keys[bisect.bisect_left(keys, lo):bisect.bisect_right(keys, hi)]:      # [lower_bound(fuzzy_left), upper_bound(fuzzy_right)), :280-281
            if k2 == k or k2[3] == a:
                continue
            left_diff, right_diff = ir._i32(l) - ir._i32(k2[1]), ir._i32(rt) - ir._i32(k2[2])        # :288-289
            if (left_diff < min_anchor or right_diff < min_anchor) and js[k][2] < js[k2][2]:         # :290-295
                out[k] = False
    return state, out


def consensus(recs, seqs=None, min_anchor=8, known=(), limits=None, mism=None):
    """both passes -> (junctions, insertions, deletions) in indelbed_ref.consensus's forms.  mism[i] = mismatches() of record i (all 0
    when not given).  A record the filter drops is in neither pass (single-end input: tophat_reports.cpp:133-136 feeds the first pass,
    :1202-1205 the second)."""
    mism = [0] * len(recs) if mism is None else mism
    live = [k for k, r in enumerate(recs) if not dropped(mism[k], r[3], limits)]
    _state, accepted = first_pass([recs[k] for k in live], min_anchor, known)
    js, ins, dels, letters = {}, {}, {}, {}
    for k in live:
        r = recs[k]
        if not ir.kept(r, accepted):                            # exclude_hits_on_filtered_junctions, :1207-1226
            continue
        for (ref, l, rt, a, le, re) in ir.rec_juncs(r):
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


def parse_gtf_juncs(text, name_id):
    """tophat_reports.cpp:2675-2711 on the text of a --gtf-juncs file: fgets lines of at most 4095 bytes, cut at TABs (get_token,
    common.cpp:242-263), atoi, antisense exactly when the orientation begins with '-' -> sorted distinct junctions, or None where the
    reference ends the run (a line of fewer than four fields).  name_id(name) = contig number, 0: the run does not know it (such a
    line can match no record and is passed over)."""
    def atoi(s):
        s = s.lstrip(" \t\n\v\f\r")
        k = 1 if s[:1] in "+-" and s[:1] else 0
        e = k
        while e < len(s) and s[e].isdigit():
            e += 1
        return (int(s[:e]) if e > k else 0) & U32
    out = set()
    data = text
    while data:
        nl = data.find("\n")
        line, data = (data[:nl + 1], data[nl + 1:]) if 0 <= nl < 4095 else (data[:4095], data[4095:])
        line = line[:-1] if line.endswith("\n") else line
        f = line.split("\t")
        if len(f) < 4:
            return None
        ref = name_id(f[0])
        if ref:
            out.add((ref, atoi(f[1]), atoi(f[2]), 1 if f[3][:1] == "-" else 0))
    return sorted(out)
