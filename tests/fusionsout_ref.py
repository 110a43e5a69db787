"""Test infrastructure: a plain-Python restatement of how tophat_reports gets fusions.out from the alignments it reports --
written from reading the reference (fusions.cpp, fusions.h, tophat_reports.cpp:1156-1180), each function citing its lines; nothing
here runs on a GPU or calls the product.

A record is indelbed_ref's (ref_id, left, antisense_splice, [(op, len) ...], ref_id2 or 0) plus (read_idx, edit_dist): read_idx
numbers the reads of one record list from 0; the records of one read are its alignments (HitsForRead).  A fusion alignment is one
record.  32-bit unsigned arithmetic where the reference has it.  Contigs are ordered by their number (the reference orders them by
a hash of their names).  Not restated: pair_support -- the two pair columns are 0 and the pair list is empty, which is what the
reference prints for single-end input."""
from __future__ import annotations

import bisect

import numpy as np

import indelbed_ref as ir

U32 = 0xFFFFFFFF
UP, DOWN, FUSION = (1, 11, 5), (2, 12, 6), (7, 8, 9, 10)
_RC = str.maketrans("ACGTN", "TGCAN")


def _fields(rec):
    ref, left, _anti, cig = rec[:4]
    return ref, left, cig, (rec[4] if len(rec) > 4 else 0), (rec[5] if len(rec) > 5 else 0), (rec[6] if len(rec) > 6 else 0)


def rec_fusion(rec):
    """fusions_from_spliced_hit with auto_sort (fusions.cpp:441-495) and the anchor sums of fusions_from_alignment (:141-194), for
    the first fusion op -> None or ((ref1, ref2, left, right, dir), left_pos, right_pos, inner)"""
    ref, left, cig, ref2, _ri, _ed = _fields(rec)
    pos = left & U32
    for c, (op, ln) in enumerate(cig):
        if op in UP:
            pos = (pos + ln) & U32                                                                # :451-455
        elif op in DOWN:
            pos = (pos - ln) & U32                                                                # :456-460
        elif op in FUSION:
            p = (pos + 1) & U32 if op in (9, 10) else (pos - 1) & U32                             # :466-469
            if ref < ref2 or (ref == ref2 and p < ln):                                            # :471-473
                key = (ref, ref2, p, ln, op)
            else:
                key = (ref2, ref, ln, p, op)                                                      # :480-487
            left_pos = sum(l for o, l in cig[:c] if o in UP + DOWN)                               # :153-171
            right_pos = sum(l for o, l in cig[c + 1:] if o in UP + DOWN)                          # :173-191
            return key, left_pos, right_pos, (c > 0 and c + 1 < len(cig))                         # :150
    return None


def rec_unsplit(rec):
    """read_len() (bwt_map.h:145-165), right() (:213-243), qualifies = the test of unsupport_fusions (fusions.cpp:289)"""
    _ref, left, cig, _r2, _ri, _ed = _fields(rec)
    rl = sum(l for o, l in cig if o in (1, 2, 3, 4, 13))
    r = left & U32
    plain = True
    for op, ln in cig:
        if op in UP:
            r = (r + ln) & U32
        elif op in DOWN:
            r = (r - ln) & U32
        elif op in FUSION:
            r = ln
        if op in FUSION or op in (11, 12):
            plain = False
    return rl, r, plain and rl >= 40


def difference(first, second):
    """difference(), fusions.cpp:44-100"""
    n = len(first)
    if n != len(second):
        return 0
    min_value = 10000
    curr, prev = [0] * 1024, [0] * 1024
    for j in range(n):
        for i in range(n):
            value = 10000
            match = 0 if first[i] == second[j] else 1
            if i == 0:
                value = j * 2 + match
            elif j > 0:
                value = prev[i] + 2
            temp = 10000
            if j == 0:
                temp = i * 2 + match
            elif i > 0:
                temp = curr[i - 1] + 2
            if temp < value:
                value = temp
            if i > 0 and j > 0:
                temp = prev[i - 1] + match
            if temp < value:
                value = temp
            curr[i] = value
            if (i == n - 1 or j == n - 1) and value < min_value:
                min_value = value
        curr, prev = prev, curr
    return min_value


def _window(seq, lo, hi):
    """seq[lo:hi); a base past the contig's end reads as N (the reference's window may end one base past it, :234-256)"""
    return "".join(seq[k] if k < len(seq) else "N" for k in range(lo, hi))


def strings_and_diffs(key, genome):
    """fusions.cpp:228-267 -> (chr1_seq, chr2_seq, diffs); ("", "", []) near a contig end"""
    ref1, ref2, left, right, d = key
    s1, s2 = genome[ref1 - 1], genome[ref2 - 1]
    if not (left >= 50 and left + 50 <= len(s1) and right >= 50 and right + 50 <= len(s2)):       # :234-235
        return "", "", []
    if d in (9, 10):
        a = _window(s1, left - 50, left + 50).translate(_RC)[::-1]                                # :239-243
    else:
        a = _window(s1, left - 49, left + 51)                                                     # :245
    if d in (8, 10):
        b = _window(s2, right - 49, right + 51).translate(_RC)[::-1]                              # :247-251
    else:
        b = _window(s2, right - 50, right + 50)                                                   # :253
    diffs = []
    for j in range(5):                                                                            # :258-265
        pos = (5 - j - 1) * 20 // 2
        diffs.append(difference(a[pos:pos + (j + 1) * 20], b[pos:pos + (j + 1) * 20]))
    return a, b, diffs


def _groups(recs, mask):
    n = {}
    for r, m in zip(recs, mask):
        if m:
            n[_fields(r)[4]] = n.get(_fields(r)[4], 0) + 1
    return n


def _passes(rec, anchor, mism):
    """the fusion of a record that update_fusions / fusions_from_alignment let through: edit distance (tophat_reports.cpp:1172), the
    op neither first nor last, both anchors (fusions.cpp:150, :193)"""
    if _fields(rec)[5] > mism:
        return None
    f = rec_fusion(rec)
    if f is None or not f[3] or f[1] < anchor or f[2] < anchor:
        return None
    return f


def fusions(recs, genome, anchor=20, mism=2, multi=2, min_anchor=8):
    """both passes -> rows [(key, count, unsupport, left_ext, right_ext, left_bases, right_bases, chr1_seq, chr2_seq, diffs)] in
    Fusion::operator< order (fusions.h:39-67), count > 0 only (print_fusions, fusions.cpp:362)"""
    # pass 1 (tophat_reports.cpp:2018-2090): every record; the reference set with its mirror entries (fusions.cpp:210-223)
    g1 = _groups(recs, [True] * len(recs))
    ref_set = {}                                              # (ref1, ref2, left, right, dir) -> the un-mirrored key
    for r in recs:
        if g1[_fields(r)[4]] > multi:                                                             # tophat_reports.cpp:1164
            continue
        f = _passes(r, anchor, mism)
        if f:
            k = f[0]
            ref_set.setdefault(k, k)
            ref_set[(k[1], k[0], k[3], k[2], k[4])] = k
    order = sorted(ref_set, key=lambda k: (k[2], k[3], k[0], k[1], k[4]))                         # fusion_comparison, fusions.h:199-220
    lefts = [(k[2], k[3], k[0], k[1], k[4]) for k in order]
    # pass 2 (:2286-2318): the records exclude_hits_on_filtered_junctions keeps, group sizes among those
    accepted = ir.first_pass([r[:5] for r in recs], min_anchor)
    keep = [ir.kept(r[:5], accepted) for r in recs]
    g2 = _groups(recs, keep)
    stat = {}

    def entry(k):
        return stat.setdefault(k, dict(count=0, unsupport=0, le=0, re=0, lb=[0] * 50, rb=[0] * 50))
    update_stat = len(ref_set) > 0                                                                # tophat_reports.cpp:1167
    for r, kp in zip(recs, keep):
        if not kp or g2[_fields(r)[4]] > multi or _fields(r)[5] > mism:
            continue
        f = _passes(r, anchor, mism)
        if f:
            k, lp, rp, _ = f
            e = entry(k)
            e["count"] += 1                                                                       # fusions.cpp:196-207
            if update_stat:
                e["le"], e["re"] = max(e["le"], lp), max(e["re"], rp)                             # :271-272
                for i in range(min(lp, 50)):
                    e["lb"][i] += 1                                                               # :274-277
                for i in range(min(rp, 50)):
                    e["rb"][i] += 1
        if update_stat:
            rl, right, ok = rec_unsplit(r)                                                        # unsupport_fusions, :287-343
            if ok:
                lo, hi = (_fields(r)[1] + 20) & U32, (right - 20) & U32
                a = bisect.bisect_right(lefts, (lo, 0, 0, 0, 7))                                  # upper_bound(Fusion(0, 0, left, 0)), :297
                b = bisect.bisect_left(lefts, (hi, U32, U32, U32, 7))                             # lower_bound(Fusion(max, max, right, max)), :298
                for q in range(a, b):                         # (an interval that ends before it starts holds nothing here)
                    if order[q][0] == _fields(r)[0]:
                        entry(ref_set[order[q]])["unsupport"] += 1
    rows = []
    for k in sorted(stat):
        e = stat[k]
        if e["count"] <= 0:
            continue
        a, b, diffs = strings_and_diffs(k, genome) if update_stat else ("", "", [])
        rows.append((k, e["count"], e["unsupport"], e["le"], e["re"], tuple(e["lb"]), tuple(e["rb"]), a, b, tuple(diffs)))
    return rows


def fusions_out(rows, names):
    """print_fusions, fusions.cpp:347-433"""
    out = []
    for (k, count, unsup, le, re, lb, rb, a, b, diffs) in rows:
        symm = np.float32(0.0)
        for x, y in zip(lb, rb):                                                                  # :377-382, in float
            term = np.float32(x - y) / np.float32(count)
            symm = np.float32(symm + np.float32(term * term))
        line = "%s-%s\t%d\t%d\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%.6f" % (names[k[0] - 1], names[k[1] - 1], ir._i32(k[2]), ir._i32(k[3]),
                                                                 {7: "ff", 8: "fr", 9: "rf"}.get(k[4], "rr"), count, 0, 0, unsup, le, re, float(symm))
        line += "\t@\t" + "".join("%d " % d for d in diffs)
        line += "\t@\t%s %s\t@\t%s %s\t@\t" % (a[:len(a) // 2], a[len(a) // 2:], b[:len(b) // 2], b[len(b) // 2:])
        line += "".join("%d " % x for x in lb) + "\t@\t" + "".join("%d " % x for x in rb) + "\t@\t\n"
        out.append(line)
    return "".join(out)


def stat_rows(a):
    """FUSSTAT_DTYPE array -> the rows of fusions()"""
    return [((int(x["ref_id1"]), int(x["ref_id2"]), int(x["left"]), int(x["right"]), int(x["dir"])), int(x["count"]), int(x["unsupport"]), int(x["left_ext"]),
             int(x["right_ext"]), tuple(int(v) for v in x["left_bases"]), tuple(int(v) for v in x["right_bases"]), bytes(x["seq1"]).decode(), bytes(x["seq2"]).decode(),
             tuple(int(v) for v in x["diffs"][:int(x["n_diffs"])])) for x in a]
