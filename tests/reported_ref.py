"""Test-only: a Python restatement of thj_junctions' host reader as it stands -- parse_record and keep
(tophat_amd/csrc/host/thj_junctions_main.cpp:77-180) -- one BAM record -> one thj_aln for the junction consensus, or nothing, or the
end of the run.  Where parse_record follows the reference the lines of BAMHitFactory::get_hit_from_buf are given too
(bwt_map.cpp:1208-1318).  Pure Python, no GPU; the record core of the device route (thj_reported_core.h) and the device route itself
are held to this."""
import struct

MATCH, INS, DEL, REF_SKIP, SOFT_CLIP = 1, 3, 5, 11, 13
OPS = (MATCH, INS, DEL, REF_SKIP, SOFT_CLIP, 14, 15, MATCH, MATCH)          # :95  MIDNSHP=X
ANTISENSE_SPLICE = 4
NT16 = "=ACMGRSVTWYHKDBN"                                                    # bam_nt16_rev_table (bwt_map.cpp:1158-1165)
MAX_INS = 16                                                                 # thj_juncbed_add_records_seq: "at most 16 are held"

# the ways the host reader ends the run (die), and the add call behind it (THJ_EINVAL)
MALFORMED, XF_OPS, CIGAR_OPS, INS_RANGE, INS_LONG, INS_LETTER = "malformed", "xf_ops", "cigar_ops", "ins_range", "ins_long", "ins_letter"
REP_BITS = {MALFORMED: 1, XF_OPS: 2, CIGAR_OPS: 4, INS_RANGE: 8, INS_LONG: 16, INS_LETTER: 32}      # rpt::REP_* of the record core


class Loud(Exception):
    def __init__(self, what):
        Exception.__init__(self, what)
        self.what = what


class Kept:
    """ref_id, left, flags, edit_dist, n_cigar, cigar (16 words), letters (the inserted bases, op after op; "" unless indels are collected),
    key (QNAME + the 0x40 / 0x80 bits: what tells one read's alignments from the next's, :79-84)"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def row(self):
        return (self.ref_id, self.left, self.flags, self.edit_dist, self.n_cigar) + tuple(self.cigar)


def split(s, sep):
    """tokenize.cpp as thj_hostio.h has it: the non-empty runs between separators"""
    return [t for t in s.split(sep) if t]


def strtol(s):
    """strtol(s, &t, 10) -> (value saturated to a long, characters consumed; 0 when there is no digit)"""
    i = 0
    while i < len(s) and s[i] in b" \t\n\v\f\r":
        i += 1
    neg = False
    if i < len(s) and s[i] in b"+-":
        neg = s[i] == ord("-")
        i += 1
    j = i
    while j < len(s) and 48 <= s[j] <= 57:
        j += 1
    if j == i:
        return 0, 0
    v = int(s[i:j])
    v = -v if neg else v
    return max(-2 ** 63, min(2 ** 63 - 1, v)), j


def atoi(s):
    v = strtol(s)[0] & 0xFFFFFFFF
    return v - 2 ** 32 if v >= 2 ** 31 else v


def walk_ins(cigar, n_cigar, left):
    """jbw::inss (thj_jb_walk.h:80-98; insertions_from_spliced_hit, insertions.cpp:109-180) -> [(length, position in the read)]"""
    out, rpos = [], 0
    for c in range(n_cigar):
        op, ln = cigar[c] >> 28, cigar[c] & 0x0FFFFFFF
        if op in (1, 2):
            rpos += ln
        elif op in (3, 4):
            out.append((ln, rpos))
            rpos += ln
    return out


def keep(a, seq, indels, fusions, d):
    """:77-93 -- and what thj_juncbed_add_records_seq refuses behind it (an insertion of more than 16 bases, a letter outside ACGTN)"""
    flag_nc = struct.unpack_from("<I", d, 12)[0]
    l_rn = d[8]
    name = d[32:32 + l_rn].split(b"\0")[0]
    a.key = name + bytes([48 + ((flag_nc >> 22) & 3)])
    a.letters = ""
    if not indels:
        return a
    for ln, rpos in walk_ins(a.cigar, a.n_cigar, a.left):
        if rpos + ln > len(seq):
            raise Loud(INS_RANGE)                                            # :88
        a.letters += seq[rpos:rpos + ln]
    for ln, _rpos in walk_ins(a.cigar, a.n_cigar, a.left):
        if ln > MAX_INS:
            raise Loud(INS_LONG)
    if any(ch not in "ACGTN" for ch in a.letters):
        raise Loud(INS_LETTER)
    return a


def parse_record(d, tid2ref, name_id, max_report_intron, indels, fusions):
    """d = the record after its block_size field.  -> Kept, or None (skipped / dropped); raises Loud where the host reader dies.
    name_id: contig name (bytes) -> ref_id of the run's frozen table (RefTable::get_id: 0 for a name it does not hold)"""
    bs = len(d)
    if bs < 32:
        raise Loud(MALFORMED)
    tid, p0, bin_mq_nl, flag_nc, l_seq = struct.unpack_from("<iiIIi", d, 0)  # :96-97
    l_rn, n_cig = bin_mq_nl & 0xFF, flag_nc & 0xFFFF
    # bam_record_shape_ok (thj_hostio.h:907-915)
    if l_seq < 0 or l_rn == 0 or 32 + l_rn + 4 * n_cig + (l_seq + 1) // 2 + l_seq > bs or d[32 + l_rn - 1] != 0:
        raise Loud(MALFORMED)                                                # :98
    if tid < 0 or ((flag_nc >> 16) & 4):                                     # :100
        return None
    cigar = [0] * 16
    spliced = gapped = False
    pp = 32 + l_rn
    for i in range(n_cig):                                                   # :104
        c = struct.unpack_from("<I", d, pp)[0]
        pp += 4
        op = OPS[c & 15] if (c & 15) < 9 else 15
        spliced |= op == REF_SKIP
        gapped |= op in (INS, DEL)
        if i < 16:
            cigar[i] = (op << 28) | (c >> 4)
    seq4 = pp
    pp += (l_seq + 1) // 2 + l_seq                                           # :106
    xs, xf, nm = 0, None, 0
    fixed = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4, "d": 8, "B": 5}      # bam_aux_fixed_size
    while pp + 3 <= bs:                                                      # :109-128
        t, ty = d[pp:pp + 2], chr(d[pp + 2])
        pp += 3
        if fixed.get(ty, 0) > bs - pp:
            raise Loud(MALFORMED)                                            # :112
        if ty == "A":
            if t == b"XS":
                xs = d[pp]
            pp += 1
        elif ty in "cCsSiI":
            fmt = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}[ty]
            if t == b"NM":
                nm = struct.unpack_from(fmt, d, pp)[0]
            pp += struct.calcsize(fmt)
        elif ty == "f":
            pp += 4
        elif ty == "d":
            pp += 8
        elif ty in "ZH":                                                     # :123
            at = pp
            while pp < bs and d[pp]:
                pp += 1
            if pp < bs and ty == "Z" and t == b"XF":
                xf = bytes(d[at:pp])
            pp += 1
        elif ty == "B":                                                      # :124-125
            st = chr(d[pp])
            cnt = struct.unpack_from("<i", d, pp + 1)[0]
            if cnt < 0 or cnt > bs:
                raise Loud(MALFORMED)
            pp += 5 + cnt * (1 if st in "cC" else 2 if st in "sS" else 4)
        else:
            pp = bs                                                          # :126
    a = Kept(flags=ANTISENSE_SPLICE if xs == ord("-") else 0, edit_dist=0 if nm < 0 else 255 if nm > 255 else nm)      # :129-130
    if xf is not None:
        if xf[:1] == b"2":                                                    # :132 (bwt_map.cpp:1214-1216)
            return None
        f = split(xf, b" ")
        if len(f) < 4:                                                       # :134
            return None
        cs = split(f[1], b"-")
        # :138 -- fewer than two names: the second lookup is that of the empty name, which a frozen table does not hold
        r1 = name_id(cs[0]) if len(cs) >= 2 else (tid2ref[tid] if tid < len(tid2ref) else 0)
        r2 = name_id(cs[1]) if len(cs) >= 2 else name_id(b"")
        if not r1 or not r2:                                                 # :139
            return None
        op, spl, gap = [], False, False
        q = f[3]
        while q:                                                             # :142-163 (bwt_map.cpp:1240-1301)
            ln, used = strtol(q)
            if ln <= 0:
                return None
            ch = chr(q[used]) if used < len(q) else "\0"
            if ch in "MmIiDd":
                code = {"M": 1, "m": 2, "I": 3, "i": 4, "D": 5, "d": 6}[ch]
                gap |= ch in "IiDd"
            elif ch in "Nn":
                if ln > max_report_intron:
                    return None
                code, spl = (11 if ch == "N" else 12), True
            elif ch == "F":
                code, ln = 7, ln - 1
            elif ch in "SHP":
                code = {"S": 13, "H": 14, "P": 15}[ch]
            else:
                return None
            q = q[used + 1:]
            if len(op) >= 15:
                raise Loud(XF_OPS)                                           # :155
            op.append((code << 28) | (ln & 0x0FFFFFFF))
            n = len(op)
            if n >= 3 and (op[n - 2] >> 28) == 7:                            # :157-162 (bwt_map.cpp:1283-1301)
                up = lambda c: (c >> 28) in (1, 5, 3, 11)
                i1, i2 = up(op[n - 3]), up(op[n - 1])
                dr = 8 if (i1 and not i2) else 9 if (not i1 and i2) else 10 if (not i1 and not i2) else 7
                op[n - 2] = (dr << 28) | (op[n - 2] & 0x0FFFFFFF)
        if not spl and not (indels and gap) and not fusions:                 # :164
            return None
        a.cigar = op + [0] * (16 - len(op))
        a.cigar[15] = r2
        a.ref_id, a.left, a.n_cigar = r1, atoi(f[2]) - 1, len(op)
        fseq = f[4].decode("latin-1") if len(f) > 4 else ""                  # :169 (bwt_map.cpp:1231-1232)
        return keep(a, fseq, indels, fusions, d)
    if not (spliced and n_cig >= 3) and not (indels and gapped) and not (fusions and not spliced):      # :173
        return None
    if n_cig > 16:
        raise Loud(CIGAR_OPS)                                                # :175
    a.ref_id = tid2ref[tid] if tid < len(tid2ref) else 0
    if not a.ref_id:
        return None
    a.cigar, a.left, a.n_cigar = cigar, p0, n_cig
    seq = "".join(NT16[(d[seq4 + (k >> 1)] >> (4 if (k & 1) == 0 else 0)) & 15] for k in range(max(l_seq, 0)))      # :179
    return keep(a, seq, indels, fusions, d)


def parse_all(records, tid2ref, name_id, max_report_intron, indels, fusions):
    """records (each after its block_size field), in file order -> (the kept ones, read_idx of each: one number per run of records of one read, :249-254)"""
    kept = [k for k in (parse_record(d, tid2ref, name_id, max_report_intron, indels, fusions) for d in records) if k is not None]
    run, idx = 0, []
    for i, k in enumerate(kept):
        if i and k.key != kept[i - 1].key:
            run += 1
        idx.append(run)
    return kept, idx
