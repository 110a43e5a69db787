"""Test-only: the reference's reading of a BAM record, restated over the record's bytes.

`hit_from_record` follows BAMHitFactory::get_hit_from_buf (bwt_map.cpp:1101-1452) statement by statement, with the samtools
0.1.18 accessors it calls (bam_aux.c: bam_aux_get and its __skip_tag, bam_aux2i, bam_aux2A; bam.h: bam_aux_type2size), and
BowtieHit's own right() / read_len() (bwt_map.h:145-243), gap_length (bwt_map.cpp:32-43) and ReadTable::get_id (atoi,
bwt_map.h:546-552).  It is written from those sources and from neither parser of this project (thj_ingest.hip: parse_hit,
thj_hostio.h: parse_hit_bam), which are twins of one another.

Three rules are this project's and not the reference's; the restatement names them so:
  * a record whose target the run does not know (tid2ref gives 0, or the target id lies outside the file's table) is dropped
    -- the reference would make up a contig id (or index past its header);
  * a record of an unaligned read (tid < 0) is dropped -- the reference builds a hit on "*" that no finder uses;
  * an XF tag and a sixth counted CIGAR operation are errors of the run (the device records hold five).

Every branch taken leaves a label in TAKEN: the tests compare that set with a fixed list, so a case table that stops
reaching a branch is noticed.
"""
import struct

TAKEN = set()

CIG_MATCH, CIG_INS, CIG_DEL, CIG_REF_SKIP, CIG_SOFT_CLIP, CIG_HARD_CLIP, CIG_PAD = 1, 3, 5, 11, 13, 14, 15   # bwt_map.h:36-55
_BAM_OPS = {0: ("M", CIG_MATCH), 1: ("I", CIG_INS), 2: ("D", CIG_DEL), 3: ("N", CIG_REF_SKIP), 4: ("S", CIG_SOFT_CLIP),
            5: ("H", CIG_HARD_CLIP), 6: ("P", CIG_PAD)}          # the arms of the switch at bwt_map.cpp:1330-1350
SEQ_LETTERS = "=ACMGRSVTWYHKDBN"                               # bam_nt16_rev_table


def _take(label):
    TAKEN.add(label)


def _toupper(c):
    return c - 32 if 97 <= c <= 122 else c


def _type2size(x):
    """bam_aux_type2size (bam.h:754-760)"""
    if x in (ord("C"), ord("c"), ord("A")):
        return 1
    if x in (ord("S"), ord("s")):
        return 2
    if x in (ord("I"), ord("i"), ord("f")):
        return 4
    return 0


def aux_get(rec, start, name):
    """bam_aux_get: the position of the TYPE byte of the first tag called `name`, or None.  The walk is __skip_tag's: the type
    is upper-cased before its size is looked up, so an `f` or `d` value is NOT stepped over (neither 'F' nor 'D' has a size):
    the walk goes on inside it.  Past the record's end the walk stops (the reference would read on)."""
    s, end = start, len(rec)
    while s < end:
        if s + 2 > end:
            _take("aux_tail_short")
            return None
        tag = rec[s:s + 2]
        s += 2
        if tag == name:
            return s if s < end else None
        if s >= end:
            _take("aux_tail_short")
            return None
        raw = rec[s]
        ty = _toupper(raw)
        s += 1
        if ty in (ord("Z"), ord("H")):
            _take("skip_" + chr(raw))
            while s < end and rec[s]:
                s += 1
            s += 1
        elif ty == ord("B"):
            if s + 5 > end:
                _take("aux_tail_short")
                return None
            sub = rec[s]
            cnt, = struct.unpack_from("<i", rec, s + 1)
            _take("skip_B_%s_%s" % (chr(sub), "empty" if cnt == 0 else "some"))
            s += 5 + _type2size(sub) * cnt
            if s < start:                                          # a negative count: the reference walks backwards; no case plants one
                return None
        else:
            size = _type2size(ty)
            if raw in b"fd":
                _take("skip_%s_walked_into" % chr(raw))
            elif size == 0:
                _take("skip_unknown_type")
            else:
                _take("skip_" + chr(raw))
            s += size
    return None


def aux2i(rec, p):
    """bam_aux2i (bam_aux.c:159-170); the label says which arm and which sign"""
    ty = chr(rec[p])
    fmt = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<i"}.get(ty)
    if fmt is None or p + 1 + struct.calcsize(fmt) > len(rec):
        _take("int_of_non_integer_type")
        return 0
    v, = struct.unpack_from(fmt, rec, p + 1)
    _take("tag_%s%s" % (ty, "_neg" if v < 0 else ""))
    return v


def aux2A(rec, p):
    """bam_aux2A (bam_aux.c:190-197)"""
    if rec[p] != ord("A") or p + 2 > len(rec):
        _take("char_of_non_A_type")
        return 0
    return rec[p + 1]


def _atoi(b):
    i, n = 0, len(b)
    while i < n and b[i] in b" \t\n\v\f\r":
        i += 1
    sign = 1
    if i < n and b[i] in b"+-":
        sign = -1 if b[i] == ord("-") else 1
        i += 1
    v = 0
    while i < n and 48 <= b[i] <= 57:
        v = v * 10 + b[i] - 48
        i += 1
    return (sign * v) & 0xFFFFFFFF


def _scan_u(b, i):
    """one %u of sscanf: (value, next index) or None when no digit follows (white space and a sign are taken first)"""
    n = len(b)
    while i < n and b[i] in b" \t\n\v\f\r":
        i += 1
    neg = False
    if i < n and b[i] in b"+-":
        neg = b[i] == ord("-")
        i += 1
    j = i
    v = 0
    while j < n and 48 <= b[j] <= 57:
        v = v * 10 + b[j] - 48
        j += 1
    if j == i:
        return None
    return ((-v if neg else v) & 0xFFFFFFFF), j


def name_fields(qname):
    """bwt_map.cpp:1120-1143 -> (insert id, end)"""
    end = True
    pipe = qname.rfind(b"|")
    if pipe < 0:
        _take("name_no_pipe")
    else:
        if qname.count(b"|") > 1:
            _take("name_last_pipe")
        tag = qname[pipe + 1:]
        if b":" not in tag:
            _take("name_no_colon")
        else:
            vals = [0, 0, 0]                                    # seg_offset, seg_num, num_segs
            i = assigned = 0
            for k in range(3):
                r = _scan_u(tag, i)
                if r is None:                                   # sscanf stops at the first field it cannot convert
                    break
                vals[k], i = r
                assigned += 1
                if k < 2:
                    if i < len(tag) and tag[i] == ord(":"):
                        i += 1
                    else:
                        break
            _take("name_fields_%d" % assigned)
            end = ((vals[1] + 1) & 0xFFFFFFFF) == vals[2]
            _take("name_end" if end else "name_not_end")
        qname = qname[:pipe]
    return _atoi(qname), end


def hit_from_record(rec, tid2ref, max_report_intron):
    """rec: one BAM record without its block_size word.  -> ("keep", HitRec) | ("drop", id, reason) | ("error", id, reason).
    HitRec = (id, ref_id, left, right, antisense, end, mismatches, edit_dist, read_len, [(op, len) ...], antisense_splice)"""
    tid, pos, l_rn, _mq, _bin, n_cig, flag, l_seq, mtid, _mpos, _tlen = struct.unpack_from("<iiBBHHHiiii", rec, 0)
    qname = rec[32:32 + l_rn]
    qname = qname[:qname.index(0)] if 0 in qname else qname
    rid, end = name_fields(bytes(qname))
    if tid < 0:
        _take("tid_negative")
        return ("drop", rid, "tid_negative")
    aux0 = 32 + l_rn + 4 * n_cig + (l_seq + 1) // 2 + l_seq
    antisense_splice = False
    num_mismatches = 0
    p = aux_get(rec, aux0, b"XS")
    if p is not None:
        c = aux2A(rec, p)
        _take("xs_minus" if c == ord("-") else "xs_other")
        antisense_splice = c == ord("-")
    else:
        _take("xs_missing")
    p = aux_get(rec, aux0, b"NM")
    if p is not None:
        v = aux2i(rec, p)
        num_mismatches = v & 0xFF                               # unsigned char num_mismatches
        if not 0 <= v <= 255:
            _take("nm_cut_to_a_byte")
    else:
        _take("nm_missing")
    if aux_get(rec, aux0, b"XF") is not None:
        _take("xf_tag")
        return ("error", rid, "xf_tag")
    cigar = []
    spliced = False
    counted = 0
    for i in range(n_cig):
        w, = struct.unpack_from("<I", rec, 32 + l_rn + 4 * i)
        length = w >> 4
        if length <= 0:
            _take("op_zero_length")
            return ("drop", rid, "op_zero_length")
        arm = _BAM_OPS.get(w & 0xF)
        if arm is None:                                         # default: "BAM read: invalid CIGAR operation"
            _take("op_%s" % {7: "EQ", 8: "X"}.get(w & 0xF, "%d" % (w & 0xF)))
            return ("drop", rid, "op_without_an_arm")
        _take("op_" + arm[0])
        opcode = arm[1]
        if opcode == CIG_REF_SKIP:
            spliced = True
            if length > max_report_intron:
                _take("intron_above_max")
                return ("drop", rid, "intron_above_max")
            if length == max_report_intron:
                _take("intron_at_max")
        if opcode != CIG_HARD_CLIP:
            cigar.append((opcode, length))
            counted += 1
        if opcode in (CIG_INS, CIG_DEL):
            if length > num_mismatches:
                _take("nm_wrap")
            num_mismatches = (num_mismatches - length) & 0xFF
    if mtid >= 0:
        if mtid != tid:
            _take("mate_on_another_target")
            return ("drop", rid, "mate_on_another_target")
        _take("mate_on_the_same_target")
    else:
        _take("mate_none")
    if tid >= len(tid2ref):
        _take("tid_outside_table")
        return ("drop", rid, "tid_outside_table")
    ref_id = tid2ref[tid]
    if ref_id == 0:
        _take("contig_unknown")
        return ("drop", rid, "contig_unknown")
    if counted > 5:
        _take("six_counted_ops")
        return ("error", rid, "six_counted_ops")
    if counted == 5:
        _take("five_counted_ops")
    gap = sum(n for o, n in cigar if o in (CIG_INS, CIG_DEL))
    right = pos + sum(n for o, n in cigar if o in (CIG_MATCH, CIG_REF_SKIP, CIG_DEL))
    read_len = sum(n for o, n in cigar if o in (CIG_MATCH, CIG_INS, CIG_SOFT_CLIP))
    if read_len > 255:
        _take("read_len_above_255")
    if flag & 4:
        _take("flag_unmapped_with_a_target")
    _take("antisense" if flag & 0x10 else "sense")
    if antisense_splice and not spliced:
        _take("xs_minus_unspliced")
    _take("kept")
    return ("keep", (rid, ref_id, pos, right, bool(flag & 0x10), end, num_mismatches, (num_mismatches + gap) & 0xFF, read_len,
                     cigar, antisense_splice and spliced))


def records_of(data, start=0):
    """the records (without block_size) of an inflated BAM stream from `start`"""
    out = []
    p = start
    while p + 4 <= len(data):
        bs, = struct.unpack_from("<i", data, p)
        out.append(bytes(data[p + 4:p + 4 + bs]))
        p += 4 + bs
    return out


def kept_hits(recs, tid2ref, max_report_intron, begin_id=0, end_id=0xFFFFFFFF):
    """the HitRecs of a map's shard, in file order (HitStream: ids in [begin_id, end_id), segment_juncs.cpp:4005)"""
    out = []
    for r in recs:
        h = hit_from_record(r, tid2ref, max_report_intron)
        if h[0] == "error":
            raise ValueError("%s in record of id %d" % (h[2], h[1]))
        if h[0] == "keep" and begin_id <= h[1][0] < end_id:
            out.append(h[1])
    return out


def read_from_record(rec):
    """ReadStream::get_direct (reads.cpp:528-630) -> (id, bases, phred+33 qualities, qc_fail)"""
    _tid, _pos, l_rn, _mq, _bin, n_cig, flag, l_seq = struct.unpack_from("<iiBBHHHi", rec, 0)
    qname = rec[32:32 + l_rn]
    qname = qname[:qname.index(0)] if 0 in qname else qname
    p = 32 + l_rn + 4 * n_cig
    sb = rec[p:p + (l_seq + 1) // 2]
    seq = "".join(SEQ_LETTERS[(sb[i >> 1] >> (4 if (i & 1) == 0 else 0)) & 0xF] for i in range(l_seq))
    q = rec[p + (l_seq + 1) // 2:p + (l_seq + 1) // 2 + l_seq]
    return _atoi(bytes(qname)), seq, bytes((x + 33) & 0xFF for x in q), bool(flag & 0x200)


def reads_of(recs):
    """id -> (bases, qualities): QC-fail records are read past, the first remaining record of an id is the read (ReadStream::getRead)"""
    out = {}
    for r in recs:
        rid, seq, qual, qc = read_from_record(r)
        if qc:
            _take("read_qc_fail_skipped")
            continue
        if rid in out:
            continue
        out[rid] = (seq, qual)
    return out
