"""Test-only: hand-made BAM files for the ingest tests -- a raw record builder, a BGZF writer with explicit member cuts, and the
case tables (parser, layout, merge, reads, loud failures).  Pure Python, no GPU.  What a record MEANS is ingest_ref.py's business;
this module only plants bytes."""
import struct
import zlib

M, I, D, N, S, H, P, EQ, X = range(9)                 # BAM CIGAR op codes ("MIDNSHP=X")
MAX_INTRON = 5000                                      # max_report_intron of every test here
TARGETS = (("chr1", 1000000), ("chr2", 1000000), ("chrU", 5000))
KNOWN = "chr1,chr2"                                    # the contigs the run knows: chrU's records are dropped
TID2REF = (1, 2, 0)
NIB = {"=": 0, "A": 1, "C": 2, "G": 4, "T": 8, "N": 15}


def cw(op, n):
    """one raw CIGAR word"""
    return ((n << 4) | op) & 0xFFFFFFFF


def codes(s):
    return [NIB[c] for c in s]


def record(name, tid=0, pos=1000, flag=0, mtid=-1, cigar=(), seq=(), qual=None, aux=b"", spare=0, l_seq=None, block_size=None):
    """one BAM record WITH its block_size word.  seq = nibble codes (all 16 can be planted; `spare` fills the unused low nibble of an
    odd length); aux = the aux block as literal bytes; l_seq / block_size override what the header claims"""
    name = name if isinstance(name, bytes) else str(name).encode()
    n = len(seq)
    sb = bytearray((n + 1) // 2)
    for i, c in enumerate(seq):
        sb[i >> 1] |= (c & 15) << (4 if (i & 1) == 0 else 0)
    if n & 1:
        sb[-1] |= spare & 15
    if qual is None:
        qual = bytes([30]) * n
    assert len(qual) == n and len(name) < 255
    body = name + b"\0" + b"".join(struct.pack("<I", w) for w in cigar) + bytes(sb) + bytes(qual) + aux
    core = struct.pack("<iiBBHHHiiii", tid, pos, len(name) + 1, 255, 4680, len(cigar), flag, n if l_seq is None else l_seq, mtid, -1, 0)
    rec = core + body
    return struct.pack("<i", len(rec) if block_size is None else block_size) + rec


def tag(name, ty, v=None):
    name = name.encode()
    if ty in "cCsSiI":
        return name + ty.encode() + struct.pack({"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}[ty], v)
    if ty == "A":
        return name + b"A" + v.encode()
    if ty in "ZH":
        return name + ty.encode() + (v if isinstance(v, bytes) else v.encode()) + b"\0"
    if ty == "B":
        sub, items = v
        fmt = {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I", "f": "f"}[sub]
        return name + b"B" + sub.encode() + struct.pack("<i", len(items)) + struct.pack("<%d%s" % (len(items), fmt), *items)
    return name + ty.encode() + (v or b"")                # f, d, unknown types: literal value bytes


def int_types_for(v):
    """every BAM integer type that can hold v"""
    rng = {"c": (-128, 127), "C": (0, 255), "s": (-32768, 32767), "S": (0, 65535), "i": (-2 ** 31, 2 ** 31 - 1), "I": (0, 2 ** 32 - 1)}
    return [t for t in "cCsSiI" if rng[t][0] <= v <= rng[t][1]]


def filler(name, total, **kw):
    """a record of exactly `total` bytes (block_size word included), padded by a ZZ:Z tag"""
    base = len(record(name, aux=tag("ZZ", "Z", b""), **kw))
    assert total >= base, (total, base)
    return record(name, aux=tag("ZZ", "Z", b"x" * (total - base)), **kw)


# ---------------------------------------------------------------------------------------------------------------- BGZF
def bgzf_member(data, level=6):
    assert len(data) <= 65536
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    comp = co.compress(data) + co.flush()
    assert len(comp) + 26 <= 65536, "member does not fit a BGZF block at level %d" % level
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(comp) + 25) + comp +
            struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))


def bam_header(targets=TARGETS, text=""):
    out = b"BAM\x01" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(targets))
    for n, l in targets:
        out += struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", l)
    return out


class Written:
    """what write_bam made: data (the file's bytes), member_off / member_len (file offset / inflated length per member), header_len,
    chunks[k] = (member, offset inside the member, bytes) of the k-th chunk handed in"""

    def piece(self, chunk=None):
        """(bytes from a member start to the end of the file, first_skip): the whole file, or the shard that begins at a chunk"""
        if chunk is None:
            return self.data, self.header_len
        m, off, _ = self.chunks[chunk]
        return self.data[self.member_off[m]:], off

    def records_from(self, chunk=0):
        """the record bytes (without block_size) from a chunk on: what a reader positioned there sees"""
        return [c[2][4:] for c in self.chunks[chunk:]]


def write_bam(path, members, targets=TARGETS, text="", header_alone=False):
    """members: [(list of chunks, zlib level)]; a chunk is normally one record.  The header opens member 0, or is a member of its own.
    Level 0 gives stored blocks."""
    w = Written()
    hdr = bam_header(targets, text)
    w.header_len = len(hdr)
    w.member_off, w.member_len, w.chunks = [], [], []
    out = bytearray()
    todo = list(members)
    if header_alone:
        todo.insert(0, ([], 6))
    for k, (chunks, level) in enumerate(todo):
        data = bytearray(hdr if k == 0 else b"")
        for c in chunks:
            w.chunks.append((k, len(data), bytes(c)))
            data += c
        w.member_off.append(len(out))
        w.member_len.append(len(data))
        out += bgzf_member(bytes(data), level)
    out += bgzf_member(b"")                            # samtools' EOF marker
    w.data = bytes(out)
    w.path = path
    if path:
        with open(path, "wb") as f:
            f.write(w.data)
    return w


# ---------------------------------------------------------------------------------------------------------------- parser table
SEQ25 = codes("ACGTACGTACGTACGTACGTACGTA")
NM1 = tag("NM", "C", 1)
SPL = [cw(M, 10), cw(N, 300), cw(M, 15)]


def _c(label, qname=None, **kw):
    kw.setdefault("cigar", [cw(M, 25)])
    kw.setdefault("seq", SEQ25)
    kw.setdefault("aux", NM1)
    return (label, qname, kw)


def parser_cases():
    """[(label, qname or None, record arguments)]: one record each.  Cases without a name get a running id."""
    out = []
    # ---- names: one group of id 7 (and one record whose id is 0)
    for qn in (b"7", b"7|0:0:3", b"7|50:2:3", b"7|0:1", b"7|abc", b"a|9|25:0:1", b"7" + b"x" * 247 + b"|0:2:3", b"7|:1:2", b"7|0::1"):
        out.append(_c("name_" + (qn.decode() if len(qn) < 20 else "254_chars"), qn))
    assert len(out[6][1]) == 254
    # ---- CIGAR operations
    out.append(_c("m_only"))
    out.append(_c("n_at_max", cigar=[cw(M, 10), cw(N, MAX_INTRON), cw(M, 15)], aux=NM1 + tag("XS", "A", "+")))
    out.append(_c("n_above_max", cigar=[cw(M, 10), cw(N, MAX_INTRON + 1), cw(M, 15)]))
    out.append(_c("op_I", cigar=[cw(M, 10), cw(I, 2), cw(M, 13)], aux=tag("NM", "C", 3)))
    out.append(_c("op_D", cigar=[cw(M, 10), cw(D, 3), cw(M, 15)], aux=tag("NM", "C", 4)))
    out.append(_c("op_S", cigar=[cw(S, 3), cw(M, 22)]))
    out.append(_c("op_H_front", cigar=[cw(H, 5), cw(M, 25)]))
    out.append(_c("op_H_back", cigar=[cw(M, 25), cw(H, 5)]))
    out.append(_c("five_ops_and_two_H", cigar=[cw(H, 2), cw(M, 10), cw(I, 1), cw(M, 5), cw(D, 2), cw(M, 9), cw(H, 3)], aux=tag("NM", "C", 5)))
    out.append(_c("op_P", cigar=[cw(M, 10), cw(P, 2), cw(M, 15)]))
    out.append(_c("op_zero_length", cigar=[cw(M, 10), cw(I, 0), cw(M, 15)]))
    out.append(_c("op_zero_length_H", cigar=[cw(H, 0), cw(M, 25)]))
    out.append(_c("op_EQ", cigar=[cw(EQ, 10), cw(M, 15)]))
    out.append(_c("op_X", cigar=[cw(M, 12), cw(X, 1), cw(M, 12)]))
    for op in range(9, 16):
        out.append(_c("op_%d" % op, cigar=[cw(M, 10), cw(op, 5), cw(M, 10)]))
    out.append(_c("exactly_five_ops", cigar=[cw(M, 5), cw(I, 1), cw(M, 5), cw(D, 1), cw(M, 14)], aux=tag("NM", "C", 2)))
    out.append(_c("five_ops_S_I_N", cigar=[cw(S, 2), cw(M, 8), cw(N, 77), cw(I, 3), cw(M, 12)], aux=tag("NM", "C", 4) + tag("XS", "A", "-")))
    for n in (255, 256, 300):
        out.append(_c("read_len_%d" % n, cigar=[cw(M, n)], seq=codes("ACGT" * 75)[:n]))
    out.append(_c("read_len_256_by_S_and_I", cigar=[cw(S, 100), cw(M, 100), cw(I, 56)], seq=codes("ACGT" * 64), aux=tag("NM", "C", 60)))
    # ---- NM: every integer type that holds the value
    for v in (0, 1, 127, 128, 255, 256, 257, 32767, 32768, 65535, 65536, 2 ** 31, -1, -128, -129, -32768, -32769):
        for t in int_types_for(v):
            out.append(_c("nm_%d_%s" % (v, t), aux=tag("NM", t, v)))
    out.append(_c("nm_missing", aux=b""))
    out.append(_c("nm_missing_other_tags", aux=tag("AS", "c", -5) + tag("XS", "A", "+")))
    out.append(_c("nm_after_other_tags", aux=tag("XS", "A", "+") + tag("ZZ", "Z", "abc") + tag("AS", "s", -300) + tag("NM", "C", 3)))
    out.append(_c("nm_before_other_tags", aux=tag("NM", "C", 3) + tag("XS", "A", "+") + tag("ZZ", "Z", "abc") + tag("AS", "s", -300)))
    for t in int_types_for(2):                           # NM - indel wraps as an unsigned char: 2 - 5 = 253, and 253 + 5 = 2 again
        out.append(_c("nm_below_indel_%s" % t, cigar=[cw(M, 10), cw(I, 5), cw(M, 10)], aux=tag("NM", t, 2)))
    out.append(_c("nm_below_indel_D_neg", cigar=[cw(M, 10), cw(D, 200), cw(M, 15)], aux=tag("NM", "c", -3)))
    # ---- tags to step over on the way to NM.  samtools 0.1.18 does not step over an `f` or `d` VALUE (__skip_tag upper-cases the
    # type and knows no size for 'F' / 'D'): it walks into the value.  The values planted here read, to that walk, as one-byte
    # tags ("qqC?"), so that it lands on the next tag like a walk that knows the sizes.
    out.append(_c("skip_f", aux=tag("XX", "f", b"qqCq") + tag("NM", "C", 3)))
    out.append(_c("skip_d", aux=tag("XX", "d", b"qqCqrrCr") + tag("NM", "C", 3)))
    out.append(_c("skip_Z", aux=tag("MD", "Z", "10A14") + tag("NM", "C", 3)))
    out.append(_c("skip_Z_empty", aux=tag("MD", "Z", "") + tag("NM", "C", 3)))
    out.append(_c("skip_H", aux=tag("XH", "H", "1AE301") + tag("NM", "C", 3)))
    for sub in "cCsSiIf":
        for items in ((), (1, 2, 3)):
            out.append(_c("skip_B_%s_%d" % (sub, len(items)), aux=tag("XB", "B", (sub, items)) + tag("NM", "C", 3) + tag("XS", "A", "+")))
    out.append(_c("unknown_type_ends_the_walk", aux=tag("NM", "C", 3) + b"ZQ?"))
    out.append(_c("xs_plus_unspliced", aux=NM1 + tag("XS", "A", "+")))
    # ---- XS
    out.append(_c("xs_minus_spliced", cigar=SPL, aux=NM1 + tag("XS", "A", "-")))
    out.append(_c("xs_plus_spliced", cigar=SPL, aux=NM1 + tag("XS", "A", "+")))
    out.append(_c("xs_minus_unspliced", aux=NM1 + tag("XS", "A", "-")))
    out.append(_c("xs_typed_Z", cigar=SPL, aux=NM1 + tag("XS", "Z", "-")))
    out.append(_c("xs_missing_spliced", cigar=SPL))
    # ---- the first tag of a name counts (bam_aux_get)
    out.append(_c("nm_twice", aux=tag("NM", "C", 1) + tag("NM", "C", 9)))
    out.append(_c("nm_Z_then_C", aux=tag("NM", "Z", "9") + tag("NM", "C", 9)))
    out.append(_c("xs_minus_then_plus", cigar=SPL, aux=NM1 + tag("XS", "A", "-") + tag("XS", "A", "+")))
    out.append(_c("xs_plus_then_minus", cigar=SPL, aux=NM1 + tag("XS", "A", "+") + tag("XS", "A", "-")))
    out.append(_c("xs_Z_then_minus", cigar=SPL, aux=NM1 + tag("XS", "Z", "+") + tag("XS", "A", "-")))
    # ---- the other rules
    out.append(_c("flag_4_with_a_target", flag=4))
    out.append(_c("flag_16", flag=16))
    out.append(_c("flag_16_spliced", flag=16, cigar=SPL, aux=NM1 + tag("XS", "A", "-")))
    out.append(_c("flag_4_tid_minus_1", flag=4, tid=-1, pos=-1, cigar=[]))
    out.append(_c("tid_minus_1", tid=-1))
    out.append(_c("tid_second_contig", tid=1))
    out.append(_c("tid_unknown_contig", tid=2))
    out.append(_c("tid_at_n_tid", tid=3))
    out.append(_c("tid_above_n_tid", tid=40000))
    out.append(_c("mtid_same", mtid=0))
    out.append(_c("mtid_same_second_contig", tid=1, mtid=1))
    out.append(_c("mtid_other", mtid=1))
    out.append(_c("mtid_minus_1", mtid=-1))
    out.append(_c("pos_zero", pos=0))
    return out


FIRST_RUNNING_ID = 10


def parser_records():
    """-> [(label, record bytes)]: the parser table as the records of one id-sorted map"""
    out, rid = [], FIRST_RUNNING_ID
    for k, (label, qname, kw) in enumerate(parser_cases()):
        if qname is None:
            qname = b"%d" % rid
            rid += 1
        out.append((label, record(qname, pos=kw.pop("pos", 1000 + 7 * k), **kw)))
    return out


def plain_hit(rid, pos, n=25, flag=0, seg=None):
    name = b"%d" % rid if seg is None else b"%d|%d:%d:%d" % (rid, seg[0] * 25, seg[0], seg[1])
    return record(name, pos=pos, flag=flag, cigar=[cw(M, n)], seq=SEQ25[:n] if n <= 25 else codes("ACGT" * 64)[:n], aux=NM1)


def plain_read(rid, seq="ACGTACGTACGTACGTACGTACGTA", qual=None, **kw):
    return record(b"%d" % rid, tid=-1, pos=-1, flag=kw.pop("flag", 4), seq=codes(seq) if isinstance(seq, str) else seq, qual=qual, **kw)


# ---------------------------------------------------------------------------------------------------------------- loud failures
def loud_cases():
    """[(label, record, return code name, piece of the message)]: each goes into a map of its own, between two good records"""
    return [
        ("xf_tag", record(b"20", cigar=[cw(M, 25)], seq=SEQ25, aux=NM1 + tag("XF", "Z", "1 chr1-chr2 100 10M5F10M ACGT IIII")), "EINVAL", "fusion (XF)"),
        ("six_counted_ops", record(b"20", cigar=[cw(M, 5), cw(I, 1), cw(M, 5), cw(D, 1), cw(M, 5), cw(S, 9)], seq=SEQ25, aux=tag("NM", "C", 2)), "EINVAL", "more than 5 CIGAR"),
        ("header_does_not_fit_block_size", record(b"20", cigar=[cw(M, 25)], seq=SEQ25, aux=NM1, l_seq=4000), "EINVAL", "malformed BAM record"),
        ("fixed_size_tag_cut_off", record(b"20", cigar=[cw(M, 25)], seq=SEQ25, aux=tag("AS", "C", 1) + b"NMi\x01\x00"), "EINVAL", "malformed BAM record"),
        ("double_tag_cut_off", record(b"20", cigar=[cw(M, 25)], seq=SEQ25, aux=NM1 + b"XDd\x01\x02\x03\x04\x05\x06\x07"), "EINVAL", "malformed BAM record"),
        ("array_tag_count_past_the_record", record(b"20", cigar=[cw(M, 25)], seq=SEQ25, aux=b"XBBi" + struct.pack("<i", 1000) + b"\1\0\0\0" + NM1), "EINVAL", "malformed BAM record"),
        ("array_tag_count_wraps_32_bits", record(b"20", cigar=[cw(M, 25)], seq=SEQ25, aux=b"XBBi" + struct.pack("<I", 0x40000001) + b"\1\0\0\0" + NM1), "EINVAL", "malformed BAM record"),
    ]


def loud_members(rec):
    return [([plain_hit(19, 500), rec, plain_hit(21, 900)], 6)]


# ---------------------------------------------------------------------------------------------------------------- layout table
class Table:
    """files (name -> Written) and whatever else a table's tests need"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _w(dirname, fname, members, **kw):
    import os
    return write_bam(os.path.join(dirname, fname) if dirname else None, members, **kw)


def layout_table(dirname=None):
    """one segment map for thj_k_walk, first_skip and the compaction, and the reads of its ids.  hit_ids[k] = id of hits.chunks[k]"""
    kept = dict(cigar=[cw(M, 25)], seq=SEQ25)
    members, ids = [], []

    def add(chunks, level):
        members.append(([c for _, c in chunks], level))
        ids.extend(i for i, _ in chunks)

    # a first member that is mostly header
    text = "@HD\tVN:1.0\tSO:unsorted\n" + "".join("@CO\tlayout table, header line %05d %s\n" % (k, "pad " * 12) for k in range(650))
    add([(1, plain_hit(1, 100)), (2, plain_hit(2, 200)), (2, plain_hit(2, 210)), (3, plain_hit(3, 300))], 6)
    # a member of the smallest legal records (no CIGAR, no bases, a one-letter name): one group of id 9, more records than thj_k_parse
    # has threads, fewer than MAXREC
    tiny = [(9, record(b"9", pos=5000 + k)) for k in range(65536 // 38)]
    assert len(tiny[0][1]) == 38 and 1700 <= len(tiny) < 1824
    add(tiny, 6)
    # a block_size field at each offset 4090 .. 4110 of a member (the walk's 4 KiB window and its 16-byte apron), one member each; the
    # one at 4100 is a stored member; three of them go on to the next window's edge
    rid = 10
    for T in range(4090, 4111):
        chunks = [(rid, filler(b"%d" % rid, T, pos=1000 + T, **kept)), (rid, plain_hit(rid, 2000 + T)), (rid + 1, plain_hit(rid + 1, 3000 + T))]
        if T % 7 == 0:
            used = sum(len(c) for _, c in chunks)
            chunks += [(rid + 1, filler(b"%d" % (rid + 1), 8192 - 4096 + T - used, pos=4000 + T, **kept)), (rid + 2, plain_hit(rid + 2, 5000 + T))]
            rid += 1
        add(chunks, 0 if T == 4100 else 1 if T & 1 else 9)
        rid += 2
    # one record larger than 4 KiB and one larger than 8 KiB
    add([(rid, plain_hit(rid, 7000)), (rid + 1, filler(b"%d" % (rid + 1), 5003, pos=7100, **kept)), (rid + 1, plain_hit(rid + 1, 7200)),
         (rid + 2, filler(b"%d" % (rid + 2), 9001, pos=7300, **kept)), (rid + 3, plain_hit(rid + 3, 7400))], 6)
    rid += 4
    # a member of exactly 65536 bytes that ends on a record end
    chunks = [(rid + k // 2, plain_hit(rid + k // 2, 8000 + k)) for k in range(500)]
    used = sum(len(c) for _, c in chunks)
    rid += 250
    chunks.append((rid, filler(b"%d" % rid, 65536 - used, pos=9000, **kept)))
    add(chunks, 6)
    rid += 1
    add([(rid, plain_hit(rid, 9500)), (rid + 1, plain_hit(rid + 1, 9600))], 0)
    hits = _w(dirname, "layout_hits.bam", members, text=text)
    assert hits.header_len > 50000 and hits.member_len[-2] == 65536
    starts = {off for (m, off, _) in hits.chunks if m >= 2}
    assert all(T in starts for T in range(4090, 4111))
    all_ids = sorted(set(ids))
    reads = _w(dirname, "layout_reads.bam", [([plain_read(i) for i in all_ids[:40]], 6), ([plain_read(i) for i in all_ids[40:]], 1)])
    # three id shards whose borders fall inside members: the second begins at its first record, the third one record early
    k2 = next(k for k in range(1, len(ids)) if ids[k] > 20 and ids[k] != ids[k - 1] and hits.chunks[k][1] > 0)
    b2 = ids[k2]
    b3 = all_ids[-100]
    k3 = next(k for k, i in enumerate(ids) if i == b3) - 1
    assert hits.chunks[k3][1] > 0 and hits.chunks[k3][0] == hits.chunks[k3 + 1][0]
    shards = [(None, 1, b2), (k2, b2, b3), (k3, b3, 0xFFFFFFFF)]
    # a member that ends in the middle of a record
    r = plain_hit(5, 700)
    straddle = _w(dirname, "layout_straddle.bam", [([plain_hit(4, 600), r[:50]], 6), ([r[50:], plain_hit(6, 800)], 6)])
    return Table(hits=hits, hit_ids=ids, reads=reads, shards=shards, straddle=straddle)


# ---------------------------------------------------------------------------------------------------------------- merge table
MERGE_SEG = {0: (0, 1, 0), 99: (1, 1, 1), 100: (2, 1, 3), 101: (2, 0, 0), 102: (0, 1, 2), 103: (1, 1, 1), 110: (1, 1, 0), 111: (0, 2, 1),
             112: (1, 63, 0), 113: (0, 64, 1), 114: (1, 65, 0), 115: (0, 300, 1), 120: (1, 0, 1), 500120: (1, 1, 1), 500121: (1, 0, 1),
             500122: (1, 1, 1)}
MERGE_MATE_FULL = {97: 1, 100: 2, 103: 1, 112: 3, 500121: 1, 500150: 1}
MERGE_MATE_LAST = {97: 1, 101: 1, 103: 2, 113: 65, 120: 1, 500120: 1, 500150: 2}
MERGE_READS = (98, 99, 100, 101, 102, 103, 104, 105, 110, 111, 112, 113, 114, 115, 116, 120, 500120, 500121, 500122, 500130)
# (begin_id, end_id, include_top0): the id range's ends, first-segment-only reads both ways, mates outside the segment ids, id 0
MERGE_CALLS = ((100, 500122, 0), (100, 500122, 1), (95, 500200, 0), (0, 104, 1))


def merge_read(rid, qc_fail=False):
    n = 30 + rid % 40
    seq = ("ACGTTGCANACG" * 9)[rid % 7:rid % 7 + n]
    if qc_fail:
        return plain_read(rid, seq="T" * n, flag=4 | 0x200)
    return plain_read(rid, seq=seq, qual=bytes((rid + k) % 41 for k in range(n)))


def merge_table(dirname=None):
    """nseg = 3 and both mate maps.  seg_start[s] = the chunk a reader of segment map s starts at (map 2: inside the group of id 100)"""
    segs = []
    for s in range(3):
        recs = []
        for rid in sorted(MERGE_SEG):
            for j in range(MERGE_SEG[rid][s]):
                recs.append(record(b"%d|%d:%d:3" % (rid, 25 * s, s), tid=j % 2, pos=100000 * s + (rid % 1000) * 400 + j, flag=16 * (j % 3 == 1),
                                   cigar=[cw(M, 25)], seq=SEQ25, aux=tag("NM", "C", j % 3)))
        if s == 1:                                     # member borders inside the groups of ids 114 and 115
            cut1 = next(k for k, r in enumerate(recs) if r[36:40] == b"114|") + 30
            cut2 = next(k for k, r in enumerate(recs) if r[36:40] == b"115|") + 150
            members = [(recs[:cut1], 6), (recs[cut1:cut2], 0), (recs[cut2:], 1)]
        else:
            members = [(recs[:3], 6), (recs[3:], 6)]
        segs.append(_w(dirname, "merge_seg%d.bam" % s, members))
    seg_start = [0, 0, next(k for k, c in enumerate(segs[2].chunks) if c[2][36:40] == b"100|") + 1]
    assert segs[2].chunks[seg_start[2]][2][36:40] == b"100|"
    mates = []
    for name, table in (("full", MERGE_MATE_FULL), ("last", MERGE_MATE_LAST)):
        recs = [record(b"%d" % rid, tid=1, pos=900000 + (rid % 1000) * 100 + j + (50 if name == "last" else 0), cigar=[cw(M, 25)], seq=SEQ25, aux=NM1)
                for rid in sorted(table) for j in range(table[rid])]
        mates.append(_w(dirname, "merge_mate_%s.bam" % name, [(recs[:2], 6), (recs[2:], 6)]))
    reads, missing = [], []
    for rid in MERGE_READS:
        if rid == 103:
            reads.append(merge_read(rid, qc_fail=True))           # directly before the good record of the same id
        else:
            missing.append(merge_read(rid))
        reads.append(merge_read(rid))
    return Table(segs=segs, seg_start=seg_start, mate_full=mates[0], mate_last=mates[1],
                 reads=_w(dirname, "merge_reads.bam", [(reads[:7], 6), (reads[7:], 6)]),
                 reads_missing=_w(dirname, "merge_reads_missing.bam", [(missing, 6)]))


# ---------------------------------------------------------------------------------------------------------------- reads table
READS_NSEG = 2                                         # with segment_length 25: W = 2 words per plane, a quality stride of 76


def reads_table(dirname=None, W=2):
    lens = [0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, W * 64, W * 64 + 72]
    quals = (0, 40, 93, 0xFF)
    recs, rid = [], 1
    for n in lens:
        seq = [(1, 2, 4, 8, 15)[(k * 7 + n) % 5] for k in range(n)]
        recs.append(record(b"0" * (rid % 4) + b"%d" % rid, tid=-1, pos=-1, flag=4, seq=seq, spare=0xF, qual=bytes(quals[(k + n) % 4] for k in range(n))))
        rid += 1
    # all sixteen nibble codes, at even and odd places; an odd length with every code in the spare nibble's neighbourhood
    recs.append(record(b"%d" % rid, tid=-1, pos=-1, flag=4, seq=list(range(16)), qual=bytes(range(16))))
    recs.append(record(b"%d" % (rid + 1), tid=-1, pos=-1, flag=4, seq=[3] + list(range(16)) * 2, spare=0x1, qual=bytes([93]) * 33))
    # a read record with a CIGAR (the bases begin behind it)
    recs.append(record(b"%d" % (rid + 2), tid=-1, pos=-1, flag=4, cigar=[cw(M, 20)], seq=codes("GATTACAGATTACAGATTAC"), qual=bytes(range(20, 40))))
    rid += 3
    ids = list(range(1, rid))
    reads = _w(dirname, "reads_reads.bam", [(recs[:9], 6), (recs[9:], 0)])
    assert {(4 + off) % 4 for (_m, off, _c) in reads.chunks} == {0, 1, 2, 3}, "record starts at all four byte alignments"
    segs = [_w(dirname, "reads_seg%d.bam" % s, [([plain_hit(i, 1000 * s + 10 * i, seg=(s, 2)) for i in ids], 6)]) for s in range(2)]
    return Table(segs=segs, reads=reads, ids=ids, W=W)
