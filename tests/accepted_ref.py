"""Test infrastructure: a plain-Python restatement of how tophat_reports writes a single-end read's reported alignments into
accepted_hits.bam -- print_sam_for_single (tophat_reports.cpp:985-1025), rewrite_sam_record's FRAG_UNPAIRED overload (:656-781),
add_auxData (:580-654) and the GBamRecord encoding (common.cpp:1000-1194) -- THROUGH THE TEXT the reference goes through: the input
record is formatted as bam_format1 formats it (bam.c:243-324), the line is cut into tokens, the tokens are edited, and the new record is
parsed from them.  It sits on top of best_ref.py's choice.  Written from reading the reference; nothing here runs on a GPU or calls the
product.

An input record is its bytes without the block_size field.  A loud case raises Loud."""
from __future__ import annotations

import math
import struct

from best_ref import Mt19937, groups, score, sort_unique  # noqa: F401  (score: what ch["score"] holds)

NT16 = "=ACMGRSVTWYHKDBN"
FR_FIRSTSTRAND, FR_SECONDSTRAND = 2, 3                      # thj_params.library_type's numbers
SORT_THRESHOLD = 16                                         # libstdc++: std::sort of at most 16 entries is an insertion sort


class Loud(Exception):
    pass


def mapq(n):
    """:734-738"""
    if n <= 1:
        return 50
    return int(-10.0 * math.log(1 - (1.0 / n)) / math.log(10.0))


# ---- bam_format1_core: the record as a SAM line's tokens
def sam_tokens(d, tname):
    tid, pos, l_rn, mq, _bin, n_cig, flag, l_seq, mtid, mpos, isize = struct.unpack_from("<iiBBHHHiiii", d, 0)
    p = 32
    qname = d[p:p + l_rn - 1].split(b"\0")[0].decode("latin-1")          # (the line is read back as a C string)
    p += l_rn
    cig = ""
    for k in range(n_cig):
        c = struct.unpack_from("<I", d, p + 4 * k)[0]
        if (c & 15) > 8:
            raise Loud("malformed")
        cig += "%d%s" % (c >> 4, "MIDNSHP=X"[c & 15])
    p += 4 * n_cig
    if mtid >= 0 or flag & 1:
        raise Loud("paired")
    if l_seq == 0:
        raise Loud("l_seq")
    seq = "".join(NT16[(d[p + (i >> 1)] >> (4 if i % 2 == 0 else 0)) & 15] for i in range(l_seq))
    p += (l_seq + 1) // 2
    q = d[p:p + l_seq]
    qual = "*" if q[0] == 0xFF else "".join(chr((x + 33) & 0xFF) for x in q)
    p += l_seq
    toks = [qname, str(flag), tname, str(pos + 1), str(mq), cig or "*", "*", str(mpos + 1), str(isize), seq, qual]
    while p < len(d):
        if p + 3 > len(d):
            raise Loud("malformed")
        key, ty = d[p:p + 2].decode("latin-1"), chr(d[p + 2])
        p += 3
        fmt = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}
        if ty == "A":
            toks.append("%s:A:%s" % (key, chr(d[p]))); p += 1
        elif ty in fmt:
            n = struct.calcsize(fmt[ty])
            if p + n > len(d):
                raise Loud("malformed")
            toks.append("%s:i:%d" % (key, struct.unpack_from(fmt[ty], d, p)[0])); p += n
        elif ty == "Z":
            e = d.find(b"\0", p)
            if e < 0:
                raise Loud("malformed")
            v = d[p:e].decode("latin-1")
            if not v or "\t" in v:
                raise Loud("Z")                             # add_aux's parse_error / a line that falls apart
            toks.append("%s:Z:%s" % (key, v)); p = e + 1
        else:
            raise Loud("tag type")                          # f, d, H, B: not taken
    return toks


# ---- GBamRecord: a record from tokens
def aux_bytes(s):
    """add_aux, common.cpp:1111-1194"""
    tag, ty, v = s[:2].encode("latin-1"), s[3], s[5:]
    if len(s) < 6:
        raise Loud("Z")
    if ty == "A":
        return tag + b"A" + v[:1].encode("latin-1")
    if ty == "i":
        x = int(v)
        if x < 0:
            return tag + (b"c" + struct.pack("<b", x) if x >= -127 else b"s" + struct.pack("<h", x) if x >= -32767 else b"i" + struct.pack("<i", x))
        return tag + (b"C" + struct.pack("<B", x) if x <= 255 else b"S" + struct.pack("<H", x) if x <= 65535 else b"I" + struct.pack("<I", x))
    assert ty == "Z"
    return tag + b"Z" + v.encode("latin-1") + b"\0"


def reg2bin(beg, end):
    beg &= 0xFFFFFFFF
    end = (end - 1) & 0xFFFFFFFF
    for sh, base in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> sh == end >> sh:
            return base + (beg >> sh)
    return 0


def new_record(qname, flag, tid, pos1, mapq_, cigar, mate_pos, tlen, seq, qual, aux):
    pos = -1 if pos1 <= 0 else pos1 - 1
    ops, end, qlen, num = [], pos & 0xFFFFFFFF, 0, ""
    if cigar != "*":
        for ch in cigar:                                    # set_cigar, :1025-1080: = and X become M
            if ch.isdigit():
                num += ch
                continue
            op = "MIDNSHP".index("M" if ch in "=X" else ch)
            ln = int(num); num = ""
            ops.append((ln << 4) | op)
            if op in (0, 2, 3):
                end = (end + ln) & 0xFFFFFFFF               # bam_calend
            if op in (0, 1, 4):
                qlen += ln                                  # bam_cigar2qlen
        if qlen != len(seq):
            raise Loud("qlen")                              # add_sequence: "CIGAR and sequence length are inconsistent"
        b = reg2bin(pos, end)
    else:
        b = reg2bin(pos, pos + 1)
    sb = bytearray((len(seq) + 1) // 2)
    for i, ch in enumerate(seq):
        sb[i >> 1] |= NT16.index(ch) << (4 if i % 2 == 0 else 0)
    ql = bytes([0xFF]) * len(seq) if qual == "*" else bytes((ord(c) - 33) & 0xFF for c in qual)
    name = qname.encode("latin-1") + b"\0"
    body = name + b"".join(struct.pack("<I", w) for w in ops) + bytes(sb) + ql + b"".join(aux_bytes(a) for a in aux)
    core = struct.pack("<iiBBHHHiiii", tid, pos, len(name), mapq_, b & 0xFFFF, len(ops), flag & 0xFFFF, len(seq), -1, mate_pos - 1, tlen)
    return struct.pack("<i", len(core) + len(body)) + core + body


def rewrite(d, cfg, ref_id, bh_score, anti, n, nxt, primary, hit_index):
    """rewrite_sam_record + add_auxData for one alignment.  nxt = (ref_id, left) of the next one in index_vector order, or None"""
    names = cfg["names"]
    toks = sam_tokens(d, names[ref_id - 1])
    for i in range(11, len(toks)):
        if toks[i].startswith("XF"):
            raise Loud("fusion")                            # :681: extract_partial_hits, two records
        if toks[i].startswith("AS"):
            toks[i] = "AS:i:%d" % min(0, bh_score)          # :703-708
    qname = toks[0]
    sl = qname.rfind("/")
    if sl >= 0 and len(qname) - sl < 4:
        qname = qname[:sl]                                  # :711-714
    flag = int(toks[1]) | (0 if primary else 0x100)
    aux, xs_found = [], False
    for t in toks[11:]:                                     # add_auxData
        if "NH:i:" not in t and "XS:i:" not in t:
            aux.append(t)
        if "XS:A:" in t:
            xs_found = True
    aux.append("NH:i:%d" % n)
    if nxt is not None:
        aux.append("CC:Z:" + ("=" if nxt[0] == ref_id else names[nxt[0] - 1]))
        aux.append("CP:i:%d" % (nxt[1] + 1))
    if not xs_found:
        if cfg["library_type"] == FR_FIRSTSTRAND:
            aux.append("XS:A:+" if anti else "XS:A:-")
        elif cfg["library_type"] == FR_SECONDSTRAND:
            aux.append("XS:A:-" if anti else "XS:A:+")
    if hit_index >= 0:
        aux.append("HI:i:%d" % hit_index)
    if cfg.get("rg"):
        aux.append("RG:Z:" + cfg["rg"])
    if names[ref_id - 1] not in cfg["header"]:
        raise Loud("contig")
    out = new_record(qname, flag, cfg["header"].index(names[ref_id - 1]), int(toks[3]), mapq(n), toks[5], int(toks[7]), int(toks[8]), toks[9], toks[10], aux)
    if len(out) > 65536:
        raise Loud("big")
    return out


def index_vector(keys, big_order=None):
    """std::sort under lex_hit_sort: (ref_id, left).  At most 16 entries: an insertion sort, ties stand in hits order.  Beyond that
    the order of ties is libstdc++'s own: big_order(keys) must give it (tests/acceptedsim runs std::sort); without ties any sort does."""
    n = len(keys)
    if n <= SORT_THRESHOLD or len(set(keys)) == n:
        return sorted(range(n), key=lambda k: keys[k])
    if big_order is None:
        raise ValueError("a read of more than 16 reported alignments with ties: the order is std::sort's own")
    return big_order(keys)


def print_sam_for_single(hits, draw, cfg, big_order=None):
    """hits = [(ref_id, AlignStatus score, record bytes)] in hits order -> the rewritten records in index_vector order"""
    n = len(hits)
    keys = [(h[0], struct.unpack_from("<i", h[2], 4)[0]) for h in hits]
    iv = index_vector(keys, big_order)
    primary = draw % n
    out = []
    for p, k in enumerate(iv):
        ref_id, sc, d = hits[k]
        anti = bool(struct.unpack_from("<H", d, 14)[0] & 0x10)
        out.append(rewrite(d, cfg, ref_id, sc, anti, n, keys[iv[p + 1]] if p + 1 < n else None, k == primary, p if n > 1 else -1))
    return out


def accepted(c, ch, raw, cfg, big_order=None):
    """c: a best_cases-style case, ch = best_ref.choose(...) over it, raw[i] = record i's bytes -> (the output records in order,
    {"big": reads on the std::sort list, "over": reads over the cap})"""
    cap, suppress, _mp = c["best"]
    g = Mt19937(1)
    out, seen = [], {"big": 0, "over": 0}
    for s, e in groups(c["reads"]):
        cand = [i for i in range(s, e) if ch["score"][i] is not None]
        top = max((ch["score"][i] for i in cand), default=None)
        left = sort_unique([i for i in cand if ch["score"][i] == top], c["recs"], c["mism"], c["anti"])[1]
        if len(left) > cap:
            seen["over"] += 1
            if not suppress:
                assert ch["draws"][s][0] == g.drawn
                for _ in range(len(left) - cap):
                    g()
        kept = sorted((i for i in range(s, e) if ch["keep"][i]), key=lambda i: ch["rank"][i])
        if not kept:
            continue
        seen["big"] += len(kept) > SORT_THRESHOLD
        out += print_sam_for_single([(c["recs"][i][0], ch["score"][i], raw[i]) for i in kept], g(), cfg, big_order)
    return out, seen
