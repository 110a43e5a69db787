"""Test-only: hand-worked cases of accepted_hits.bam for paired input (thj_juncbed_report_pairs_bam, thj_junctions --right-maps
--accepted-pairs-out).  Every expected record is written out here field by field, by hand, from reading print_sam_for_pair, both
rewrite_sam_record overloads, add_auxData and InsertAlignmentGrade (tophat_reports.cpp:580-1089, inserts.h:72-221) -- not through
accepted_pair_ref.py.  A case is a pair_cases case (L, R, best, pair, ...) plus cfg and either `want` (the output records in order)
or `loud` (a word of the message).  Also the input records of any case (raw_of) and the seeded crowd.

The usual insert, as in pair_cases: the left read is L0 = 40 unspliced bases at 1000, forward; the right read W = 40 unspliced bases
at 1240, reverse: inner distance 200, inside the window (mean 200, sd 20).  The generator (seed 1) draws 1791095845, 4282876139,
3093770124, 4005303368, 491263, ...: odd, odd, even, even, odd."""
import struct

import pair_cases as pc
from best_cases import D, M, N, plain
from ingest_cases import cw, record, tag
from jbknown_cases import rec

NAMES = ["chrA", "chrB"]
BAM_OP = {1: 0, 3: 1, 5: 2, 11: 3, 13: 4}                    # M I D N S of a case's cigar -> BAM's
L0, W = plain(1000, 40), plain(1240, 40)
MIXED = (200, 20, 10000000, True, False)
DISC = (200, 20, 10000000, False, True)


def seq_of(length, k=0):
    return [(1, 2, 4, 8)[(k + i) % 4] for i in range(length)]


def query_len(r):
    return sum(ln for op, ln in r[3] if op in (M, 3, 13))


def raw_record(name, r, anti, AS, extra=b"", mism=0):
    """the BAM record (block_size first) of a case's record: NM:C (mismatches and gap bases), AS:c, then `extra`"""
    nm = mism + sum(ln for op, ln in r[3] if op in (3, D))
    return record(name, tid=r[0] - 1, pos=r[1], flag=0x10 if anti else 0, cigar=[cw(BAM_OP[op], ln) for op, ln in r[3]], seq=seq_of(query_len(r), r[1]),
                  aux=tag("NM", "C", nm) + tag("AS", "c", AS) + extra)


def raw_of(c, extra=None):
    """{"L": [...], "R": [...]}: QNAME = the insert's number; extra(side, k) -> more aux bytes"""
    return {s: [raw_record("%d" % S["reads"][k], r, S["anti"][k], S["AS"][k], extra(s, k) if extra else b"", S["mism"][k]) for k, r in enumerate(S["recs"])] for s, S in (("L", c["L"]), ("R", c["R"]))}


def cfg_of(library_type=1, rg="", header=None):
    return {"library_type": library_type, "rg": rg, "names": NAMES, "header": header or NAMES}


def out(name, r, flag, mapq, mtid, mpos, tlen, score, tail, tid=None):
    """an expected record, block_size first, every field as given: r = the case's record (contig, pos, cigar, SEQ stay as they went in),
    tail = the tags behind NM and AS"""
    n = query_len(r)
    s = seq_of(n, r[1])
    sb = bytearray((n + 1) // 2)
    for i, ch in enumerate(s):
        sb[i >> 1] |= ch << (4 if i % 2 == 0 else 0)
    nm = sum(ln for op, ln in r[3] if op in (3, D))
    name = name.encode() + b"\0"
    cig = [cw(BAM_OP[op], ln) for op, ln in r[3]]
    body = name + b"".join(struct.pack("<I", w) for w in cig) + bytes(sb) + bytes([30]) * n + tag("NM", "C", nm) + tag("AS", "c" if score < 0 else "C", score) + tail
    core = struct.pack("<iiBBHHHiiii", r[0] - 1 if tid is None else tid, r[1], len(name), mapq, 4681, len(cig), flag, n, mtid, mpos, tlen)   # (every case lies below 16384: bin 4681)
    return struct.pack("<i", len(core) + len(body)) + core + body


NH = lambda n: tag("NH", "C", n)                              # noqa: E731
HI = lambda k: tag("HI", "C", k)                              # noqa: E731


def pcase(label, inserts, want=None, loud=None, cfg=None, **kw):
    c = pc.pcase(label, inserts, **kw)
    c["cfg"], c["want"], c["loud"] = cfg or cfg_of(), want, loud
    return c


def cases():
    cs = []
    one = [([(L0, 0)], [(W, 0)])]
    # ---- 1 x 1, opposite strands, inside the window: happy.  The right record first: 0x1 | 0x80 | 0x2 | its own 0x10 = 147, its mate is forward; mate at
    # 1000, TLEN = partner.left - its right = 1000 - 1280.  The left record: 0x1 | 0x40 | 0x2 | 0x20 (the mate is reverse) = 99, TLEN = partner.right -
    # its left = 1280 - 1000.  n = 1: MAPQ 50, both primary, no HI, no CC
    cs.append(pcase("happy_1x1", one, [out("0", W, 147, 50, 0, 1000, -280, 0, NH(1)), out("0", L0, 99, 50, 0, 1240, 280, 0, NH(1))]))
    # ---- TLEN.  The left record [1000, 1300) contains the right one [1100, 1140) and is strictly longer: +300; the right one: partner.left -
    # partner.right = -300.  (inner distance 0: too close, a penalty, the only pair all the same; not too far: happy)
    big, small = plain(1000, 300), plain(1100, 40)
    cs.append(pcase("tlen_left_contains_right", [([(big, 0)], [(small, 0)])], [out("0", small, 147, 50, 0, 1000, -300, 0, NH(1)), out("0", big, 99, 50, 0, 1100, 300, 0, NH(1))]))
    # the other way round the left read starts behind the right one: left() distance negative, a fusion pair -- reported with discordant pairs on;
    # opposite strands and not too far: 0x2 all the same
    cs.append(pcase("tlen_right_contains_left", [([(small, 0)], [(big, 0)])], [out("0", big, 147, 50, 0, 1100, 300, 0, NH(1)), out("0", small, 99, 50, 0, 1000, -300, 0, NH(1))], pair=DISC))
    # equal spans: neither is STRICTLY longer, so the last branch: its left is not below its partner's: partner.left - its right = -40, both ways
    same = plain(1000, 40)
    cs.append(pcase("tlen_equal_spans", [([(same, 0)], [(same, 0)])], [out("0", same, 147, 50, 0, 1000, -40, 0, NH(1)), out("0", same, 99, 50, 0, 1000, -40, 0, NH(1))]))
    # ---- the partner on another contig (a fusion pair: discordant pairs on): the mate's tid, TLEN 0; the distances do not ask for the contig: 0x2
    wb = plain(1240, 40, ref=2)
    cs.append(pcase("other_contig", [([(L0, 0)], [(wb, 0)])], [out("0", wb, 147, 50, 0, 1000, 0, 0, NH(1)), out("0", L0, 99, 50, 1, 1240, 0, 0, NH(1))], pair=DISC))
    # ---- equal strands (a fusion pair): no 0x2, no 0x10 on the right record, no 0x20 on the left
    cs.append(pcase("equal_strands", [([(L0, 0)], [(W, 0, 0, False)])], [out("0", W, 0x81, 50, 0, 1000, -280, 0, NH(1)), out("0", L0, 0x41, 50, 0, 1240, 280, 0, NH(1))], pair=DISC))
    # ---- too far: the right read 700 behind (M20 N100 M20 at 1740, it ends at 1880; its junction has first-pass support 1: its score is -8).  Ten
    # left-only reads show the junction (1100, 1600) inside the gap: 60 + 140 = 200 remain, rescued: happy.  Nine: not rescued, too far: no 0x2.
    # (Mixed alignments are off: the ten reads write nothing.)
    far = pc.right_at(700)
    sup = rec(1081, 20, 499, 20)
    for n_sup, bit in ((10, 2), (9, 0)):
        cs.append(pcase("too_far_support_%d" % n_sup, [([(sup, 0)], [])] * n_sup + [([(L0, 0)], [(far, 0)])],
                        [out("%d" % n_sup, far, 0x91 | bit, 50, 0, 1000, -880, -8, NH(1)), out("%d" % n_sup, L0, 0x61 | bit, 50, 0, 1740, 880, 0, NH(1))]))
    # ---- left 1 x right 2: two pairs tie, best_hits = [(L0, W), (L0, W5)]; index_vector by the right records: W, W5.  The draw is odd: pair 1 is the
    # primary.  The left record is written twice, once with each mate; CC / CP name the same side's record of the next pair: MAPQ 3 for n = 2
    w5 = plain(1245, 40)
    nxt_r, nxt_l = tag("CC", "Z", "=") + tag("CP", "S", 1246), tag("CC", "Z", "=") + tag("CP", "S", 1001)
    cs.append(pcase("left_1_right_2", [([(L0, 0)], [(W, 0), (w5, 0)])],
                    [out("0", W, 147 | 0x100, 3, 0, 1000, -280, 0, NH(2) + nxt_r + HI(0)), out("0", L0, 99 | 0x100, 3, 0, 1240, 280, 0, NH(2) + nxt_l + HI(0)),
                     out("0", w5, 147, 3, 0, 1000, -285, 0, NH(2) + HI(1)), out("0", L0, 99, 3, 0, 1245, 285, 0, NH(2) + HI(1))]))
    # ---- XS:A by side: fr-firststrand gives a forward LEFT record '-', and the RIGHT side the opposite sign of that rule: the reverse right record '-';
    # fr-secondstrand: '+' and '+'
    for lt, sign in ((2, "-"), (3, "+")):
        xs = tag("XS", "A", sign)
        cs.append(pcase("library_type_%d" % lt, one, [out("0", W, 147, 50, 0, 1000, -280, 0, NH(1) + xs), out("0", L0, 99, 50, 0, 1240, 280, 0, NH(1) + xs)], cfg=cfg_of(lt)))
    # ... and a forward right record with a reverse left one (a fusion pair by its left() distance... no: reverse left, forward right 240 BEFORE it)
    lrev, rfwd = plain(1240, 40), plain(1000, 40)
    cs.append(pcase("library_type_2_strands_swapped", [([(lrev, 0, 0, True)], [(rfwd, 0, 0, False)])],
                    [out("0", rfwd, 0x80 | 0x1 | 0x2 | 0x20, 50, 0, 1240, 280, 0, NH(1) + tag("XS", "A", "+")), out("0", lrev, 0x40 | 0x1 | 0x2 | 0x10, 50, 0, 1000, -280, 0, NH(1) + tag("XS", "A", "+"))],
                    cfg=cfg_of(2)))
    # ---- --rg-id: RG:Z last
    rg = tag("RG", "Z", "grp")
    cs.append(pcase("rg_id", one, [out("0", W, 147, 50, 0, 1000, -280, 0, NH(1) + rg), out("0", L0, 99, 50, 0, 1240, 280, 0, NH(1) + rg)], cfg=cfg_of(1, "grp")))
    # ---- the single-end way (mixed alignments): the only pair is a fusion pair (other contig) and is skipped, the list is empty: the left read, then the
    # right read, each through the unpaired overload with its side: 0x1 | 0x40 | 0x8 = 73; 0x1 | 0x80 | 0x8 | 0x10 = 153; the mate fields as they came
    # (mate "*", mpos -1, TLEN 0)
    lone = [([(L0, 0)], [(wb, 0)])]
    cs.append(pcase("single_end_way_mixed", lone, [out("0", L0, 73, 50, -1, -1, 0, 0, NH(1)), out("0", wb, 153, 50, -1, -1, 0, 0, NH(1))], pair=MIXED))
    cs.append(pcase("single_end_way_default_writes_nothing", lone, []))
    # ---- singletons: a left one and a right one
    cs.append(pcase("singletons_mixed", [([(L0, 0)], []), ([], [(W, 0)])], [out("0", L0, 73, 50, -1, -1, 0, 0, NH(1)), out("1", W, 153, 50, -1, -1, 0, 0, NH(1))], pair=MIXED))
    cs.append(pcase("singletons_default_write_nothing", [([(L0, 0)], []), ([], [(W, 0)])], []))
    # ---- over --max-multihits (2): four right records tie (AS -1, unspliced: -1 each): 1791095845 % 4 = 1 erases T2, 4282876139 % 3 = 2 erases T4
    # (the third of T1 T3 T4); T1 and T3 stay; print_sam_for_pair draws 3093770124: even, pair 0 is the primary.
    tt = [plain(1230 + 5 * k, 40) for k in range(4)]
    ins = [([(L0, 0)], [(t, -1) for t in tt])]
    cc_r, cc_l = tag("CC", "Z", "=") + tag("CP", "S", 1241), tag("CC", "Z", "=") + tag("CP", "S", 1001)
    kept = [out("0", tt[0], 147, 3, 0, 1000, -270, -1, NH(2) + cc_r + HI(0)), out("0", L0, 99, 3, 0, 1230, 270, 0, NH(2) + cc_l + HI(0)),
            out("0", tt[2], 147 | 0x100, 3, 0, 1000, -280, -1, NH(2) + HI(1)), out("0", L0, 99 | 0x100, 3, 0, 1240, 280, 0, NH(2) + HI(1))]
    cs.append(pcase("over_the_cap", ins, kept, best=(2, False, 6)))
    # --suppress-hits: nothing (mixed off); with mixed on the sides go alone: the left read's one record, the right read's four tie and are over the cap
    # too: suppressed as well
    cs.append(pcase("over_the_cap_suppressed", ins, [], best=(2, True, 6)))
    cs.append(pcase("over_the_cap_suppressed_mixed", ins, [out("0", L0, 73, 50, -1, -1, 0, 0, NH(1))], best=(2, True, 6), pair=MIXED))
    # ---- a mix: cap draws, single-end draws and primary draws interleave in the generator's order (mixed on, max_multihits 2).
    # insert 0, a left singleton of two tied alignments: draw 1 (odd): hits[1] is the primary.  hits order = BowtieHit's (by left): 1000, 1400.
    # insert 1: the pair list over the cap as above: draws 2 and 3: 4282876139 % 4 = 3 erases T4, 3093770124 % 3 = 0 erases T1: T2 and T3 stay; draw 4
    #   (4005303368, even): pair 0 (T2) is the primary.
    # insert 2, 1 x 1: draw 5 (491263 % 1 = 0).
    la, lb = plain(1000, 40), plain(1400, 40)
    mix = [([(la, 0), (lb, 0)], []), ([(L0, 0)], [(t, -1) for t in tt]), ([(L0, 0)], [(W, 0)])]
    want = [out("0", la, 73 | 0x100, 3, -1, -1, 0, 0, NH(2) + tag("CC", "Z", "=") + tag("CP", "S", 1401) + HI(0)), out("0", lb, 73, 3, -1, -1, 0, 0, NH(2) + HI(1)),
            out("1", tt[1], 147, 3, 0, 1000, -275, -1, NH(2) + tag("CC", "Z", "=") + tag("CP", "S", 1241) + HI(0)), out("1", L0, 99, 3, 0, 1235, 275, 0, NH(2) + cc_l + HI(0)),
            out("1", tt[2], 147 | 0x100, 3, 0, 1000, -280, -1, NH(2) + HI(1)), out("1", L0, 99 | 0x100, 3, 0, 1240, 280, 0, NH(2) + HI(1)),
            out("2", W, 147, 50, 0, 1000, -280, 0, NH(1)), out("2", L0, 99, 50, 0, 1240, 280, 0, NH(1))]
    cs.append(pcase("mix_of_draws", mix, want, best=(2, False, 6), pair=MIXED))
    return cs


MAPQ = {1: 50, 2: 3, 3: 1, 4: 1, 5: 0, 6: 0}                    # (int)(-10 log10(1 - 1/n)), :855-859


PRIMARY_OF = {1: 0, 2: 1, 3: 1, 4: 1, 5: 0, 6: 1}              # 1791095845 % n, the first draw


def mapq_case(n):
    """L0 against n tied right records R_k = 40 bases at 1230 + 3 k (inner distances 190 .. 205: all inside the window, all pairs score 0): n
    pairs, all reported, best_hits in generation order, which is index_vector's order too.  Pair k: the right record first -- 0x1 | 0x80 | 0x2 |
    0x10 = 147, 0x100 unless k is the primary, mate at 1000, TLEN 1000 - (1270 + 3 k); then L0 -- 99, mate at 1230 + 3 k, TLEN 270 + 3 k.  MAPQ from n;
    NH n; CC:Z:= and CP (the next pair's record of the SAME side: 1231 + 3 (k + 1), or L0's 1001) on all but the last pair; HI k when n > 1."""
    rights = [plain(1230 + 3 * k, 40) for k in range(n)]
    want = []
    for k, r in enumerate(rights):
        sec = 0 if k == PRIMARY_OF[n] else 0x100
        last = k == n - 1
        hi = HI(k) if n > 1 else b""
        want.append(out("0", r, 147 | sec, MAPQ[n], 0, 1000, -(270 + 3 * k), 0, NH(n) + (b"" if last else tag("CC", "Z", "=") + tag("CP", "S", 1231 + 3 * (k + 1))) + hi))
        want.append(out("0", L0, 99 | sec, MAPQ[n], 0, 1230 + 3 * k, 270 + 3 * k, 0, NH(n) + (b"" if last else tag("CC", "Z", "=") + tag("CP", "S", 1001)) + hi))
    return pcase("mapq_n%d" % n, [([(L0, 0)], [(r, 0) for r in rights])], want)


def loud_cases():
    """(label, case, extra(side, k) or None, raw patch(raw) or None, header, a word of the message)"""
    one = [([(L0, 0)], [(W, 0)])]
    out_ = []

    def flag_0x1(raw):
        r = bytearray(raw["R"][0])
        struct.pack_into("<H", r, 4 + 14, struct.unpack_from("<H", r, 4 + 14)[0] | 1)
        raw["R"][0] = bytes(r)
    out_.append(("flag_0x1", pcase("loud", one), None, flag_0x1, NAMES, "already has a mate"))
    out_.append(("xf_tag", pcase("loud", one), lambda s, k: tag("XF", "Z", "1 chrA-chrB 5 x y") if s == "L" else b"", None, NAMES, "fusion alignment"))
    out_.append(("tag_type_b", pcase("loud", one), lambda s, k: tag("ZB", "B", ("c", [1, 2])) if s == "R" else b"", None, NAMES, "type f, d, H or B"))
    out_.append(("contig_not_in_header", pcase("loud", [([(L0, 0)], [(plain(1240, 40, ref=2), 0)])], pair=DISC), None, None, ["chrA"], "without an @SQ line"))
    return out_


def crowd(n_inserts=300, seed=7, max_multihits=3, pair=MIXED):
    """pair_cases' crowd without fusion ops (a BAM needs two records and XF:Z for one), mixed alignments on so that every way is taken"""
    c = pc.crowd(seed=seed, n_inserts=n_inserts, max_multihits=max_multihits, fusion_ops=False)
    c["pair"] = pair
    return c


def crowd_extra(s, k):
    """tags of many kinds on the crowd's records: some shrink, some are dropped"""
    aux = b""
    if k % 4 == 1:
        aux += tag("NH", "C", 7) + tag("ZW", "Z", "a value that held NH:i:3 " * 2)
    if k % 5 == 2:
        aux += tag("YS", "s", -300) + tag("ZQ", "Z", "kept text") + tag("YI", "i", 5)
    if k % 7 == 3:
        aux += tag("XS", "A", "+")
    return aux
