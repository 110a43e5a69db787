"""Test infrastructure: a plain-Python restatement of how tophat_reports gets junctions.bed, insertions.bed and deletions.bed
from the alignments it reports -- written from reading the reference, each function citing its lines; nothing here runs on a GPU
or calls the product.

A record is (ref_id, left, antisense_splice, [(op, len) ...][, ref_id2]) with op = CigarOpCode (bwt_map.h:36-55):
1 MATCH 2 mATCH 3 INS 4 iNS 5 DEL 6 dEL 7 FUSION_FF 8 FUSION_FR 9 FUSION_RF 10 FUSION_RR 11 REF_SKIP 12 rEF_SKIP 13 SOFT_CLIP;
`seq` is the record's SEQ as BAMHitFactory::get_hit_from_buf hands it to BowtieHit::seq() (bwt_map.cpp:1158-1165: all l_qseq
bases of the record, soft-clipped ones included; for a fusion record the bases field of its XF:Z tag, :1231-1232).
32-bit unsigned arithmetic where the reference has it."""
from __future__ import annotations

import os

U32 = 0xFFFFFFFF
FUSION_JUMP = (7, 8, 9)                  # FUSION_RR (10) has no case in any of the three walkers


def _i32(x):
    x &= U32
    return x - (1 << 32) if x & 0x80000000 else x


def rec_juncs(rec):
    """junctions_from_spliced_hit, junctions.cpp:19-96 -> [(ref, left, right, antisense, left_extent, right_extent)]"""
    ref, left, anti, cig = rec[:4]
    ref2 = rec[4] if len(rec) > 4 else 0
    j, out, cur = left, [], ref
    for c, (op, ln) in enumerate(cig):
        if op in (11, 12):
            prev = cig[c - 1][1] if c > 0 else 0
            nxt = cig[c + 1][1] if c + 1 < len(cig) else 0
            if op == 11:
                out.append((cur, (j - 1) & U32, (j + ln) & U32, 1 if anti else 0, prev, nxt))       # :49-56
                j += ln
            else:
                out.append((cur, (j - ln) & U32, (j + 1) & U32, 1 if anti else 0, nxt, prev))       # :57-64
                j -= ln
        elif op in (1, 5):
            j += ln                                                                                   # :78-81
        elif op in (2, 6):
            j -= ln                                                                                   # :82-85
        elif op in FUSION_JUMP:
            j, cur = ln, ref2                                                                         # :86-91
    return out


def rec_dels(rec):
    """deletions_from_spliced_hit, deletions.cpp:83-151 -> [(ref, left, right, left_extent, right_extent, op index)].  Its own walk:
    after a dEL the position goes UP by the length (:133), unlike the junction and insertion walkers."""
    ref, left, _anti, cig = rec[:4]
    ref2 = rec[4] if len(rec) > 4 else 0
    pos, out, cur = left & U32, [], ref
    for c, (op, ln) in enumerate(cig):
        if op == 11:
            pos = (pos + ln) & U32                                                                    # :91-93
        elif op == 12:
            pos = (pos - ln) & U32                                                                    # :94-96
        elif op == 1:
            pos = (pos + ln) & U32                                                                    # :97-104
        elif op == 2:
            pos = (pos - ln) & U32
        elif op in (5, 6):
            prev = cig[c - 1][1] if c > 0 else 0                                                      # :127-130
            nxt = cig[c + 1][1] if c + 1 < len(cig) else 0
            if op == 5:
                out.append((cur, (pos - 1) & U32, (pos + ln) & U32, prev, nxt, c))                    # :115-119
            else:
                out.append((cur, (pos - ln) & U32, (pos + 1) & U32, prev, nxt, c))                    # :120-124
            pos = (pos + ln) & U32                                                                    # :133, DEL and dEL alike
        elif op in FUSION_JUMP:
            pos, cur = ln, ref2                                                                       # :140-145
    return out


def rec_inss(rec, seq):
    """insertions_from_spliced_hit, insertions.cpp:109-180 -> [(ref, left, letters, left_extent, right_extent, op index)].
    positionInRead advances on MATCH, mATCH, INS and iNS only (:129, :166): clips fall into `default`."""
    ref, left, _anti, cig = rec[:4]
    ref2 = rec[4] if len(rec) > 4 else 0
    pos, rpos, out, cur = left & U32, 0, [], ref
    for c, (op, ln) in enumerate(cig):
        if op in (11, 5):
            pos = (pos + ln) & U32                                                                    # :117-119, :131-133
        elif op in (12, 6):
            pos = (pos - ln) & U32                                                                    # :120-122, :134-136
        elif op == 1:
            pos = (pos + ln) & U32; rpos += ln                                                        # :123-130
        elif op == 2:
            pos = (pos - ln) & U32; rpos += ln
        elif op in (3, 4):
            prev = cig[c - 1][1] if c > 0 else 0                                                      # :160-163
            nxt = cig[c + 1][1] if c + 1 < len(cig) else 0
            out.append((cur, (pos - 1) & U32 if op == 3 else (pos + 1) & U32, seq[rpos:rpos + ln], prev, nxt, c))     # :153-158
            rpos += ln                                                                                # :166
        elif op in FUSION_JUMP:
            pos, cur = ln, ref2                                                                       # :169-174
    return out


def ins_letters(rec, seq):
    """the letters of a record's I / i ops in cigar order, one string (what thj_juncbed_add_records_seq is handed)"""
    return "".join(x[2] for x in rec_inss(rec, seq))


def _merge(table, key, le, re):
    """JunctionStats::merge_with (junctions.h:87-101) / deletions.cpp:61-66 / insertions.cpp:58-63: support adds up, extents take the maximum"""
    s = table.get(key)
    if s is None:
        table[key] = [le, re, 1]
    else:
        s[0], s[1], s[2] = max(s[0], le), max(s[1], re), s[2] + 1


def first_pass(recs, min_anchor=8):
    """the first-pass JunctionSet of all records with filter_junctions applied (junctions.cpp:305-318; no GTF) -> {junction: accepted}.
    Junction = (ref, left, right, antisense), ordered like Junction::operator< (junctions.h:39-57)."""
    js = {}
    for r in recs:
        for (ref, l, rt, a, le, re) in rec_juncs(r):
            _merge(js, (ref, l, rt, a), le, re)
    acc = {}
    for k, (le, re, sup) in js.items():                       # accept_if_valid, junctions.cpp:192-240 (no splice mismatches recorded)
        mn = min(le, re)
        if mn < min_anchor:
            acc[k] = False
        elif _i32(k[2]) - _i32(k[1]) > 50000:
            acc[k] = sup >= 2 and mn > 12
        else:
            acc[k] = True
    keys = sorted(js)
    out = dict(acc)
    for k in keys:                                            # knockout_shadow_junctions, junctions.cpp:242-303
        if not acc[k]:
            continue
        ref, l, rt, a = k
        lo = (ref, (l - min_anchor) & U32, rt, 1 - a)         # fuzzy_left :272-277 (left is unsigned: below the anchor it wraps and the
        hi = (ref, l, (rt + min_anchor) & U32, 1 - a)         # range [lower_bound, upper_bound) holds nothing of this contig)
        for k2 in keys:
            if k2 == k or k2[0] != ref or k2[3] == a or k2 < lo or k2 > hi:
                continue
            left_diff, right_diff = _i32(l) - _i32(k2[1]), _i32(rt) - _i32(k2[2])                     # :288-289
            if (left_diff < min_anchor or right_diff < min_anchor) and js[k][2] < js[k2][2]:          # :290-295
                out[k] = False
    return out


def kept(rec, accepted):
    """exclude_hits_on_filtered_junctions, tophat_reports.cpp:1194-1229, without the read_mismatches / gap / edit-distance limits: a
    contiguous record always stays; another one when each of its junctions is in the first-pass set and accepted"""
    return all(accepted.get(j[:4], False) for j in rec_juncs(rec))


def consensus(recs, seqs=None, min_anchor=8):
    """the second pass (tophat_reports.cpp:2286-2313): update_junctions and update_insertions_and_deletions on the records kept, in
    record order -> (junctions, insertions, deletions)
      junctions  [(ref, left, right, antisense, left_extent, right_extent, support)] after the extent filter (:2974-2984), set order
      insertions [(ref, left, letters, left_extent, right_extent, support)] in Insertion::operator< order (insertions.h:52-67:
                 contig, left, LENGTH -- two insertions of one length at one place are one entry and the first keeps its letters)
      deletions  [(ref, left, right, left_extent, right_extent, support)] in Junction::operator< order (Deletion = Junction, antisense false)"""
    accepted = first_pass(recs, min_anchor)
    js, ins, dels, letters = {}, {}, {}, {}
    for k, r in enumerate(recs):
        if not kept(r, accepted):
            continue
        for (ref, l, rt, a, le, re) in rec_juncs(r):
            _merge(js, (ref, l, rt, a), le, re)
        if seqs is not None:
            for (ref, l, s, le, re, _c) in rec_inss(r, seqs[k]):
                key = (ref, l, len(s))
                letters.setdefault(key, s)                                                            # std::map::find under operator<: the first stays
                _merge(ins, key, le, re)
        for (ref, l, rt, le, re, _c) in rec_dels(r):
            _merge(dels, (ref, l, rt), le, re)
    jout = [k + tuple(js[k]) for k in sorted(js) if js[k][2] > 0 and js[k][0] >= 8 and js[k][1] >= 8]
    iout = [(k[0], k[1], letters[k]) + tuple(ins[k]) for k in sorted(ins)]
    dout = [k + tuple(dels[k]) for k in sorted(dels)]
    return jout, iout, dout


def insertions_bed(ins, names):
    """print_insertions, insertions.cpp:87-101"""
    out = ['track name=insertions description="TopHat insertions"\n']
    for (ref, l, s, _le, _re, sup) in ins:
        out.append("%s\t%d\t%d\t%s\t%d\n" % (names[ref - 1], _i32(l), _i32(l), s, min(sup, 1000)))
    return "".join(out)


def deletions_bed(dels, names):
    """print_deletions, deletions.cpp:36-45"""
    out = ['track name=deletions description="TopHat deletions"\n']
    for (ref, l, rt, _le, _re, sup) in dels:
        out.append("%s\t%d\t%d\t-\t%d\n" % (names[ref - 1], _i32(l + 1), _i32(rt), sup))
    return "".join(out)


def junctions_bed(js, names):
    """print_junctions / print_junction, junctions.cpp:98-118, :330-350"""
    out = ['track name=junctions description="TopHat junctions"\n']
    for k, (ref, l, rt, a, le, re, sup) in enumerate(js):
        start, end = _i32(l) + 1 - le, _i32(rt) + re
        out.append("%s\t%d\t%d\tJUNC%08d\t%d\t%s\t%d\t%d\t255,0,0\t2\t%d,%d\t0,%d\n" % (names[ref - 1], start, end, k + 1, sup, "-" if a else "+", start, end,
                                                                                   le, re, _i32(rt) - start))
    return "".join(out)


_RC = str.maketrans("ACGTN", "TGCAN")


def recorded_seqs(gold_dir, case):
    """SEQ of every record of the case's accepted_hits.tsv, in file order: the read (reads.tsv; the right mate, flag 0x80, from
    reads_right.tsv) upper-cased as prep_reads does, reverse-complemented for flag 0x10"""
    d = os.path.join(gold_dir, case)
    reads = {}
    for side, fn in ((0, "reads.tsv"), (0x80, "reads_right.tsv")):
        if os.path.exists(os.path.join(d, fn)):
            for l in open(os.path.join(d, fn)):
                nm, s = l.rstrip("\n").split("\t")
                reads[(nm, side)] = s.upper()
    out = []
    for l in open(os.path.join(d, "accepted_hits.tsv")):
        t = l.rstrip("\n").split("\t")
        s = reads[(t[0], int(t[1]) & 0x80)]
        out.append(s.translate(_RC)[::-1] if int(t[1]) & 0x10 else s)
    return out


# ---- the comparison forms of the product's arrays
def ins_rows(a):
    """INSSTAT_DTYPE array -> the insertion tuples of consensus()"""
    return [(int(x["ref_id"]), int(x["left"]), bytes(x["bases"])[:int(x["len"])].decode(), int(x["left_extent"]), int(x["right_extent"]), int(x["support"])) for x in a]


def del_rows(a):
    return [(int(x["ref_id"]), int(x["left"]), int(x["right"]), int(x["left_extent"]), int(x["right_extent"]), int(x["support"])) for x in a]


def junc_rows(a):
    return [(int(x["ref_id"]), int(x["left"]), int(x["right"]), int(x["antisense"]), int(x["left_extent"]), int(x["right_extent"]), int(x["support"])) for x in a]
