"""Test-only: hand-worked cases of the unmapped-read files and the align-summary counters (thj_juncbed_collect_unmapped,
thj_junctions --left-reads ...).  Every expected record is written out here field by field, and every expected counter by hand, from
reading the worker loop, CReadProc::process, write_singleton_alignments, writeUnmapped and GBamRecord -- not through unmapped_ref.py.
Also the loud cases and the seeded crowds.  Nothing here calls the product.

A reads-file record: rd(number, ...) -> the raw BAM record WITH its block_size field (prep_reads' unaligned BAM: QNAME = the number, ZN:Z =
the read's name, ZT:A = why it was trashed).  Read numbers of a case: numbers[k] = the number of the case's read / insert k."""
import struct

import numpy as np

import best_cases as bc
import pair_cases as pc
from ingest_cases import codes, record, tag

STATS = 15
(AL_L, UM_L, MULTI_L, XMULTI_L, AL_R, UM_R, MULTI_R, XMULTI_R, PAIRS, PAIRS_MULTI, PAIRS_DISC, AL_U, UM_U, MULTI_U, XMULTI_U) = range(15)
ACGT = codes("ACGT")


def rd(number, seq=ACGT, qual=None, flag=4, zn=None, zt=None, pre=b"", post=b"", **kw):
    """zn: the ZN:Z value (None: no tag), zt: the ZT:A value; pre / post: other tags before and behind them"""
    aux = pre + (tag("ZN", "Z", zn) if zn is not None else b"") + (tag("ZT", "A", zt) if zt is not None else b"") + post
    return record(str(number) if not isinstance(number, (bytes, str)) else number, tid=-1, pos=-1, flag=flag, seq=seq, qual=qual, aux=aux, **kw)


def out(name, flag, seq, qual, l_seq, zt=None):
    """an expected record, block_size first: tid, pos -1, MAPQ 0, bin 4680, no CIGAR, mate -1 / -1, TLEN 0"""
    name = name.encode() + b"\0"
    body = name + seq + qual + (b"ZTA" + zt.encode() if zt else b"")
    core = struct.pack("<iiBBHHHiiii", -1, -1, len(name), 0, 4680, 0, flag, l_seq, -1, -1, 0)
    return struct.pack("<i", len(core) + len(body)) + core + body


Q4 = bytes([30]) * 4
S4 = bytes([0x12, 0x48])


def shape_cases():
    """[(label, reads-file record, the record expected)]: none of these reads has an alignment, so each is written"""
    cs = []
    cs.append(("zn_absent", rd(1), out("", 4, S4, Q4, 4)))
    cs.append(("zn_a/1", rd(2, zn="a/1"), out("a", 4, S4, Q4, 4)))                    # 2 characters remain from the slash on: cut
    cs.append(("zn_a/123", rd(3, zn="a/123"), out("a/123", 4, S4, Q4, 4)))            # 4 remain: not cut
    cs.append(("zn_/2", rd(4, zn="/2"), out("", 4, S4, Q4, 4)))
    cs.append(("zn_last_slash", rd(5, zn="x/y/2"), out("x/y", 4, S4, Q4, 4)))
    cs.append(("l_seq_0", rd(6, seq=[], zn="n0"), out("n0", 4, b"", b"", 0)))
    cs.append(("l_seq_1", rd(7, seq=codes("G"), spare=7, zn="n1"), out("n1", 4, bytes([0x40]), bytes([30]), 1)))      # the spare nibble comes out 0
    cs.append(("l_seq_2", rd(8, seq=codes("GT"), zn="n2"), out("n2", 4, bytes([0x48]), bytes([30, 30]), 2)))
    cs.append(("l_seq_3", rd(9, seq=codes("GTN"), spare=3, zn="n3"), out("n3", 4, bytes([0x48, 0xF0]), bytes([30]) * 3, 3)))
    # a 0x10 input of 5 bases A M N T R, qualities 1 .. 5: reversed R T N M A, complemented Y A N K T = 10 1 15 12 8; 0x10 does not come out
    cs.append(("reverse_odd_ambiguity", rd(10, seq=[1, 3, 15, 8, 5], qual=bytes([1, 2, 3, 4, 5]), flag=0x14, spare=9, zn="rv"),
               out("rv", 4, bytes([0xA1, 0xFC, 0x80]), bytes([5, 4, 3, 2, 1]), 5)))
    # every code through the complement: = A C M G R S V T W Y H K D B N reversed and complemented
    cs.append(("reverse_all_codes", rd(11, seq=list(range(16)), qual=bytes(range(16)), flag=0x14, zn="all"),
               out("all", 4, bytes([0xF7, 0xB3, 0xD5, 0x61, 0xE9, 0xA2, 0xC4, 0x80]), bytes(range(15, -1, -1)), 16)))
    cs.append(("qual_all_ff", rd(12, seq=codes("ACG"), qual=bytes([0xFF]) * 3, zn="ff"), out("ff", 4, bytes([0x12, 0x40]), bytes([40]) * 3, 3)))      # 0xff reads as 'I'
    cs.append(("one_base_quality_9", rd(13, seq=codes("A"), qual=bytes([9]), zn="q9"), out("q9", 4, bytes([0x10]), bytes([0xFF]), 1)))      # its text is "*"
    cs.append(("two_bases_quality_9", rd(14, seq=codes("AC"), qual=bytes([9, 9]), zn="q99"), out("q99", 4, bytes([0x12]), bytes([9, 9]), 2)))
    cs.append(("one_base_quality_ff", rd(15, seq=codes("A"), qual=bytes([0xFF]), zn="qf"), out("qf", 4, bytes([0x10]), bytes([40]), 1)))
    # ZT is kept (a read that was trashed but not for multi-mapping), every other tag is dropped
    cs.append(("zt_kept_others_dropped", rd(16, zn="t", zt="L", pre=tag("XA", "i", 7) + tag("ZZ", "Z", "text"), post=tag("YB", "B", ("s", [1, 2]))), out("t", 4, S4, Q4, 4, zt="L")))
    cs.append(("zt_not_of_type_A", rd(17, zn="t", pre=tag("ZT", "c", 77)), out("t", 4, S4, Q4, 4)))
    cs.append(("second_zn_ignored", rd(18, zn="first", post=tag("ZN", "Z", "second")), out("first", 4, S4, Q4, 4)))
    # matenum from 0x40 / 0x80 alone; 0x1 comes with it
    cs.append(("mate_1", rd(19, flag=0x44, zn="m/1"), out("m", 0x45, S4, Q4, 4)))
    cs.append(("mate_2", rd(20, flag=0x85, zn="m/2"), out("m", 0x85, S4, Q4, 4)))
    cs.append(("mate_both_bits", rd(21, flag=0xC4, zn="m"), out("m", 0x45, S4, Q4, 4)))
    cs.append(("paired_bit_alone", rd(22, flag=0x5, zn="m"), out("m", 4, S4, Q4, 4)))
    cs.append(("qc_fail_taken", rd(23, flag=0x204, zn="qc"), out("qc", 4, S4, Q4, 4)))
    cs.append(("leading_zeros", rd(b"0024", zn="z"), out("z", 4, S4, Q4, 4)))
    cs.append(("long_read", rd(25, seq=codes("ACGTN") * 60, qual=bytes(range(100)) * 3, zn="long"),
               out("long", 4, bytes([0x12, 0x48, 0xF1, 0x24, 0x8F] * 30), bytes(range(100)) * 3, 300)))
    return cs


def single_case():
    """four reads with groups (numbers 10 .. 13) among reads without: every single-end outcome row.  best = (2, suppress, 6), limits (2, 2, 2).
      10 one alignment: aligned            11 two tied: aligned, multi            12 three tied, the cap is 2: aligned, multi, xmulti
      13 its only alignment is over the limits: unmapped and written, whatever its ZT (M here)
      5 no group: unmapped, written        7 no group, ZT:A:M: xmulti, not written      14 no group, ZT:A:L      20 trailing, no group
    -> {suppress: (the numbers written, the counters)}"""
    reads_of = [[(bc.plain(1000, 40), 0)], [(bc.plain(2000, 40), 0), (bc.plain(2100, 40), 0)], [(bc.plain(3000, 40), 0), (bc.plain(3100, 40), 0), (bc.plain(3200, 40), 0)],
                [(bc.plain(4000, 40), 0, 5)]]
    c = bc.case("unmapped_single", reads_of, limits=(2, 2, 2), best=(2, False, 6))
    c["numbers"] = [10, 11, 12, 13]
    c["file"] = [rd(5, zn="r5"), rd(7, zn="r7", zt="M"), rd(10, zn="r10"), rd(11, zn="r11"), rd(12, zn="r12"), rd(13, zn="r13", zt="M"), rd(14, zn="r14", zt="L"), rd(20, zn="r20")]
    z = [0] * STATS
    a = list(z); a[AL_L], a[UM_L], a[MULTI_L], a[XMULTI_L] = 3, 4, 2, 2      # unmapped: 5 13 14 20; xmulti: 12 and 7
    b = list(z); b[AL_L], b[UM_L], b[MULTI_L], b[XMULTI_L] = 2, 5, 1, 2      # --suppress-hits: 12 is xmulti AND unmapped, and written
    c["want"] = {False: ([5, 13, 14, 20], a), True: ([5, 12, 13, 14, 20], b)}
    return c


def Rr(inner):
    """the right read's record `inner` bases behind L0 (40 bases at 1000, forward): 40 unspliced bases, reverse"""
    return bc.plain(1040 + inner, 40)


def paired_case():
    """seven inserts (numbers 10 .. 16), max_report_intron 500, mean 200, sd 20:
      10 one pair in the window                       11 two tied pairs                12 one pair, inner distance 500: concordant
      13 one pair, inner distance 501: discordant     14 both reads forward: a fusion pair (skipped unless discordant pairs are reported)
      15 the left read alone                          16 the right read alone, and that read has no mate bits
    reads without a group: left 9, left 16 (ZT:A:M), left 17 (no mate bits), right 15, right 18 (ZT:A:M, no mate bits)
    -> {(mixed, discordant, best): (left numbers written, right numbers written, the counters)}"""
    L0 = pc.L0
    ins = [([(L0, 0)], [(Rr(200), 0)]), ([(L0, 0)], [(Rr(200), 0), (Rr(210), 0)]), ([(L0, 0)], [(Rr(500), 0)]), ([(L0, 0)], [(Rr(501), 0)]),
           ([(L0, 0)], [(Rr(200), 0, 0, False)]), ([(L0, 0)], []), ([], [(Rr(200), 0)])]
    c = pc.pcase("unmapped_paired", ins)
    c["numbers"] = [10, 11, 12, 13, 14, 15, 16]
    c["max_report_intron"] = 500
    lf, rf = 0x45, 0x85
    c["left_file"] = [rd(9, flag=lf, zn="r9/1")] + [rd(k, flag=lf, zn="r%d/1" % k) for k in range(10, 16)] + [rd(16, flag=lf, zn="r16/1", zt="M"), rd(17, flag=4, zn="r17")]
    c["right_file"] = [rd(k, flag=rf, zn="r%d/2" % k) for k in range(10, 16)] + [rd(16, flag=4, zn="r16"), rd(18, flag=4, zn="r18", zt="M")]

    def st(**kw):
        v = [0] * STATS
        for k, x in kw.items():
            v[globals()[k]] = x
        return v
    want = {}
    # no mixed, no discordant: 14's list is empty (both unmapped, both written); 15 and 16 go alone and are written; 16's right read counts unpaired
    want[(False, False, (20, False, 6))] = ([9, 14, 15, 17], [14, 15, 16],
                                            st(AL_L=4, UM_L=3, MULTI_L=1, XMULTI_L=1, AL_R=4, UM_R=2, MULTI_R=1, PAIRS=4, PAIRS_MULTI=1, PAIRS_DISC=1, UM_U=2, XMULTI_U=1))
    # mixed: 14's sides, 15 and 16 take the single-end way and each has one alignment
    want[(True, False, (20, False, 6))] = ([9, 17], [15],
                                           st(AL_L=6, UM_L=1, MULTI_L=1, XMULTI_L=1, AL_R=5, UM_R=1, MULTI_R=1, PAIRS=4, PAIRS_MULTI=1, PAIRS_DISC=1, AL_U=1, UM_U=1, XMULTI_U=1))
    # discordant pairs reported: 14 is a pair, and a discordant one (equal strands)
    want[(False, True, (20, False, 6))] = ([9, 15, 17], [15, 16],
                                           st(AL_L=5, UM_L=2, MULTI_L=1, XMULTI_L=1, AL_R=5, UM_R=1, MULTI_R=1, PAIRS=5, PAIRS_MULTI=1, PAIRS_DISC=2, UM_U=2, XMULTI_U=1))
    # --max-multihits 1 --suppress-hits: 11's list is emptied -- both sides unmapped, multi and xmulti, neither written
    want[(False, False, (1, True, 6))] = ([9, 14, 15, 17], [14, 15, 16],
                                          st(AL_L=3, UM_L=4, MULTI_L=1, XMULTI_L=2, AL_R=3, UM_R=3, MULTI_R=1, XMULTI_R=1, PAIRS=3, PAIRS_MULTI=1, PAIRS_DISC=1, UM_U=2, XMULTI_U=1))
    # ... and with mixed the emptied list sends 11's sides down the single-end way: the left read has one alignment, the right read two over the cap of 1, suppressed
    want[(True, False, (1, True, 6))] = ([9, 17], [11, 15],
                                         st(AL_L=6, UM_L=1, XMULTI_L=1, AL_R=4, UM_R=2, XMULTI_R=1, PAIRS=3, PAIRS_DISC=1, AL_U=1, UM_U=1, XMULTI_U=1))
    c["want"] = want
    return c


def loud_cases():
    """[(label, reads file, what the message names)]: single-end, no alignments"""
    good = rd(5, zn="g")
    return [
        ("qname_letters", [good, rd(b"12a")], "not digits"),
        ("qname_empty", [good, rd(b"")], "not digits"),
        ("qname_19_digits", [good, rd(b"1234567890123456789")], "not digits"),
        ("number_0", [rd(0), good], "read number 0"),
        ("numbers_fall", [rd(7), rd(6)], "fall or repeat"),
        ("numbers_repeat", [good, rd(5)], "fall or repeat"),
        ("long_l_seq", [good, rd(6, l_seq=70000)], "65535"),
        ("zn_integer", [good, rd(6, pre=tag("ZN", "i", 3))], "ZN tag"),
        ("zn_too_long", [good, rd(6, zn="n" * 255)], "ZN tag"),
        ("tag_of_no_type", [good, rd(6, post=tag("ZQ", "?", b"\1"))], "malformed"),
        ("tag_cut_short", [good, rd(6, post=b"ZQi\1\2")], "malformed"),
    ]


def read_shape(rng, number, flag, group):
    """a reads-file record of a random shape"""
    ln = int(rng.choice([0, 1, 1, 2, 3, 36, 75, 76, 257]))
    qual = bytes([0xFF] * ln) if rng.integers(0, 8) == 0 else bytes(int(x) for x in rng.integers(0, 42, ln))
    if ln == 1 and rng.integers(0, 2):
        qual = bytes([9])
    zn = [None, "q%d" % number, "q%d/1" % number, "q%d/12" % number, "q%d/123" % number, "/2"][int(rng.integers(0, 6))]
    zt = [None, None, None, "M", "L"][int(rng.integers(0, 5))]
    pre = tag("XQ", "C", 3) if rng.integers(0, 3) == 0 else b""
    post = tag("ZZ", "Z", "x" * int(rng.integers(0, 9))) if rng.integers(0, 3) == 0 else b""
    if rng.integers(0, 3) == 0:
        flag |= 0x10
    return rd(number, seq=[int(x) for x in rng.integers(0, 16, ln)], qual=qual, flag=flag, zn=zn, zt=zt, pre=pre, post=post, spare=int(rng.integers(0, 16)))


def numbers_and_gaps(rng, n):
    """rising numbers for n units with gaps for reads without groups -> (numbers, every number of the file)"""
    numbers, all_, at = [], [], 1
    for _ in range(n):
        for _g in range(int(rng.choice([0, 0, 1, 2]))):
            all_.append(at); at += int(rng.integers(1, 3))
        numbers.append(at); all_.append(at); at += int(rng.integers(1, 4))
    for _g in range(3):
        all_.append(at); at += 1
    return numbers, all_


def single_crowd(seed=4, n_reads=300):
    """best_cases' crowd with a reads file around it: every read with a group, and reads without before, between and behind them"""
    rng = np.random.default_rng(seed)
    c = bc.crowd(seed=seed + 7, n_reads=n_reads, max_multihits=2)
    c["limits"] = (0, 2, 2)                                     # (some reads lose all their records)
    for k in range(0, len(c["mism"]), 9):
        c["mism"][k] = 1
    c["numbers"], all_ = numbers_and_gaps(rng, n_reads)
    c["file"] = [read_shape(rng, k, 4, True) for k in all_]
    return c


def paired_crowd(seed=7, n_inserts=300, mate_bits=True):
    """pair_cases' crowd (no fusion ops) with the two reads files around it; mate_bits false: one read in six comes without mate bits"""
    rng = np.random.default_rng(seed)
    c = pc.crowd(seed=seed + 3, n_inserts=n_inserts, max_multihits=2, fusion_ops=False)
    c["numbers"], all_ = numbers_and_gaps(rng, n_inserts)
    c["max_report_intron"] = 230
    for key, fl in (("left_file", 0x45), ("right_file", 0x85)):
        c[key] = [read_shape(rng, k, fl if mate_bits or rng.integers(0, 6) else 4, True) for k in all_ if rng.integers(0, 12) or k in c["numbers"]]
    return c
