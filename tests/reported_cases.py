"""Test-only: planted BAM records of REPORTED alignments for the record core of thj_juncbed_add_bam and for the device route itself:
one case per arm of thj_junctions' host reader (reported_ref.py restates it).  Built with ingest_cases' record / tag / write_bam; this
module only plants bytes and writes down, by hand, what becomes of each record."""
import struct

from ingest_cases import D, EQ, H, I, M, MAX_INTRON, N, P, S, X, codes, cw, record, tag, write_bam

TARGETS = (("chr1", 1000000), ("chr2", 1000000), ("chrU", 5000))
KNOWN = ("chr1", "chr2")                                # the run's contigs, ref_id 1 and 2: chrU's records are dropped
TID2REF = (1, 2, 0)
MODES = ((0, 0), (1, 0), (0, 1), (1, 1))                # (indels collected, fusions collected)


def name_id(name):
    return KNOWN.index(name.decode()) + 1 if name.decode("latin-1") in KNOWN else 0


LETTERS = "ACGTTGCAGGATCCTTAACCGGTTACGTACGATAGC"


def seq(n, at=None, put=None):
    s = (LETTERS * (n // len(LETTERS) + 1))[:n]
    c = codes(s)
    if at is not None:
        c[at] = put
    return c


SPL = [cw(M, 10), cw(N, 300), cw(M, 15)]                # kept whatever is collected
XS_MINUS, XS_PLUS = tag("XS", "A", "-"), tag("XS", "A", "+")


def xf(text, ty="Z"):
    return tag("XF", ty, text)


def fus(cigar, bases="", contigs="chr1-chr2", pos=1001, part="1"):
    """the tag print_bamhit writes (bwt_map.cpp:2047-2083): part, contigs, position, cigar and -- when given -- bases and qualities"""
    fields = [part, contigs, str(pos), cigar] + ([bases, "I" * len(bases)] if bases else [])
    return xf(" ".join(fields))


def _cases():
    """[(label, outcomes, record bytes)]; outcomes: one letter per MODES entry -- K kept, D dropped or skipped, L the run ends"""
    out = []

    def c(label, outcomes, aux=b"", cigar=SPL, n=25, **kw):
        kw.setdefault("seq", seq(n))
        out.append((label, outcomes, record(kw.pop("name", label), cigar=cigar, aux=aux, **kw)))

    # ---- tags
    c("nm_c_neg", "KKKK", tag("NM", "c", -3))
    c("nm_c_pos", "KKKK", tag("NM", "c", 5))
    c("nm_C_200", "KKKK", tag("NM", "C", 200))
    c("nm_s_neg", "KKKK", tag("NM", "s", -300))
    c("nm_s_300", "KKKK", tag("NM", "s", 300))
    c("nm_S_40000", "KKKK", tag("NM", "S", 40000))
    c("nm_i_neg", "KKKK", tag("NM", "i", -70000))
    c("nm_i_7", "KKKK", tag("NM", "i", 7))
    c("nm_i_70000", "KKKK", tag("NM", "i", 70000))
    c("nm_I_big", "KKKK", tag("NM", "I", 4000000000))
    c("nm_twice", "KKKK", tag("NM", "C", 3) + tag("NM", "i", 9))
    c("nm_as_A", "KKKK", tag("NM", "A", "x") + XS_MINUS)                      # an NM that is no integer is not read
    c("xs_minus_then_plus", "KKKK", XS_MINUS + XS_PLUS)
    c("xs_plus_then_minus", "KKKK", XS_PLUS + XS_MINUS)
    c("xs_as_Z", "KKKK", tag("XS", "Z", "-"))
    c("tags_before", "KKKK", tag("ZF", "f", b"\0\0\x80\x3f") + tag("ZD", "d", b"\0" * 8) + tag("ZH", "H", "1AE3") + tag("ZB", "B", ("c", [1, -2, 3])) +
      tag("ZS", "B", ("S", [7, 8])) + tag("ZI", "B", ("I", [9])) + tag("ZG", "B", ("f", [1.5])) + XS_MINUS + tag("NM", "C", 4))
    c("unknown_type_last", "KKKK", XS_MINUS + tag("NM", "C", 2) + b"ZQ?" + tag("NM", "C", 9))
    c("unknown_type_first", "KKKK", b"ZQ?" + XS_MINUS + tag("NM", "C", 9))
    c("tag_past_end_i", "LLLL", XS_MINUS + b"NMi\x01\x02")
    c("tag_past_end_d", "LLLL", b"ZDd\0\0\0\0")
    c("tag_past_end_B_header", "LLLL", b"ZBBc\x01\0")
    c("tag_B_count_negative", "LLLL", b"ZBBc" + struct.pack("<i", -1))
    c("tag_B_count_huge", "LLLL", b"ZBBi" + struct.pack("<i", 1 << 20))
    c("tag_B_runs_out_quietly", "KKKK", XS_MINUS + b"ZBBi" + struct.pack("<i", 20) + b"\0" * 8)      # 20 <= the record's bytes: the walk just ends
    c("tail_of_two_bytes", "KKKK", tag("NM", "C", 1) + b"XS")
    c("xf_unterminated", "KKKK", tag("NM", "C", 1) + b"XFZ2 chr1-chr2 5 10M")                       # no NUL inside the record: not a tag value
    c("skipped_before_its_tags", "DDDD", b"NMi\x01", tid=-1)
    c("header_does_not_fit", "LLLL", l_seq=4000)
    # ---- CIGAR
    c("ops_eq_x", "KKKK", cigar=[cw(EQ, 5), cw(X, 3), cw(N, 300), cw(M, 10)], n=18)
    c("ops_S_H_P", "KKKK", cigar=[cw(H, 2), cw(S, 3), cw(M, 10), cw(N, 300), cw(M, 10), cw(P, 2), cw(S, 2)], n=25)
    c("ops_code_9_and_15", "KKKK", cigar=[cw(M, 10), cw(9, 5), cw(N, 300), cw(15, 1), cw(M, 15)], n=25)
    c("cigar_16", "KKKK", cigar=[cw(M, 2), cw(N, 50)] * 7 + [cw(M, 2), cw(S, 1)], n=17)
    c("cigar_17_spliced", "LLLL", cigar=[cw(M, 2), cw(N, 50)] * 8 + [cw(M, 2)], n=18)
    c("cigar_17_unspliced", "DDLL", cigar=[cw(M, 2), cw(P, 1)] * 8 + [cw(M, 2)], n=18)
    c("cigar_17_gapped", "DLLL", cigar=[cw(M, 2), cw(D, 1)] * 8 + [cw(M, 2)], n=18)
    c("spliced_two_ops", "DDDD", cigar=[cw(M, 25), cw(N, 300)])
    # ---- skips
    c("unmapped_flag", "DDDD", flag=4)
    c("tid_minus_one", "DDDD", tid=-1)
    c("tid_beyond_table", "DDDD", tid=5)
    c("tid_to_zero", "DDDD", tid=2)
    c("on_chr2", "KKKK", tid=1, pos=777)
    # ---- keep rules
    c("plain_unspliced", "DDKK", cigar=[cw(M, 25)])
    c("gapped_del", "DKKK", cigar=[cw(M, 10), cw(D, 3), cw(M, 15)])
    c("spliced_with_ins", "KKKK", cigar=[cw(M, 5), cw(I, 2), cw(M, 5), cw(N, 300), cw(M, 13)])
    # ---- insertions of plain records: letters from the 4-bit SEQ
    c("ins_even", "DKKK", cigar=[cw(M, 10), cw(I, 2), cw(M, 13)])
    c("ins_odd", "DKKK", cigar=[cw(M, 11), cw(I, 2), cw(M, 12)])
    c("ins_odd_length_odd", "DKKK", cigar=[cw(M, 11), cw(I, 3), cw(M, 11)])
    c("ins_on_last_base", "DKKK", cigar=[cw(M, 23), cw(I, 2)])
    c("ins_one_past", "DLKL", cigar=[cw(M, 24), cw(I, 2)])
    c("ins_16", "DKKK", cigar=[cw(M, 5), cw(I, 16), cw(M, 5)], n=26)
    c("ins_17", "DLKL", cigar=[cw(M, 5), cw(I, 17), cw(M, 5)], n=27)
    c("ins_letter_M", "DLKL", cigar=[cw(M, 10), cw(I, 2), cw(M, 13)], seq=seq(25, 11, 3))
    c("ins_letter_N", "DKKK", cigar=[cw(M, 10), cw(I, 2), cw(M, 13)], seq=seq(25, 10, 15))
    c("ins_behind_clip", "DKKK", cigar=[cw(S, 3), cw(M, 10), cw(I, 2), cw(M, 10)])
    c("ins_twice", "DKKK", cigar=[cw(M, 4), cw(I, 1), cw(M, 4), cw(I, 3), cw(M, 13)])
    # ---- XF:Z -- the record's own fields do not matter once the tag is there
    one = [cw(M, 25)]
    c("xf_ff", "DDKK", fus("20M5000F10M") + tag("NM", "C", 1), cigar=one)
    c("xf_fr", "DDKK", fus("20M5000F10m"), cigar=one)
    c("xf_rf", "DDKK", fus("20m5000F10M"), cigar=one)
    c("xf_rr", "DDKK", fus("20m5000F10m"), cigar=one)
    c("xf_same_contig_swapped", "DDKK", fus("20M100F10M", contigs="chr2-chr1"), cigar=one)
    c("xf_pieces", "KKKK", fus("10M2I8M100N5M5000F4m3d2i50n6m", LETTERS[:37]) + XS_MINUS, cigar=one)
    c("xf_F_first", "DDKK", fus("5000F10M20M"), cigar=one)
    c("xf_15_ops", "DDKK", fus("1M" * 7 + "9F" + "1M" * 7), cigar=one)
    c("xf_16_ops", "LLLL", fus("1M" * 7 + "9F" + "1M" * 8), cigar=one)
    c("xf_N_at_max", "KKKK", fus("10M%dN10M200F10M" % MAX_INTRON), cigar=one)
    c("xf_N_above_max", "DDDD", fus("10M%dN10M200F10M" % (MAX_INTRON + 1)), cigar=one)
    c("xf_n_above_max", "DDDD", fus("10M200F10m%dn5m" % (MAX_INTRON + 1)), cigar=one)
    c("xf_length_zero", "DDDD", fus("10M0I10M100F5M"), cigar=one)
    c("xf_length_missing", "DDDD", fus("10MI10M100F5M"), cigar=one)
    c("xf_unknown_letter", "DDDD", fus("10M5X100F5M"), cigar=one)
    c("xf_dropped_before_16th", "DDDD", fus("1M" * 7 + "9F" + "1M" * 7 + "1X"), cigar=one)
    c("xf_unknown_second_name", "DDDD", fus("20M5000F10M", contigs="chr1-chrZ"), cigar=one)
    c("xf_unknown_first_name", "DDDD", fus("20M5000F10M", contigs="chrU-chr2"), cigar=one)
    c("xf_name_is_a_prefix", "DDDD", fus("20M5000F10M", contigs="chr-chr2"), cigar=one)
    c("xf_single_name", "DDDD", fus("20M5000F10M", contigs="chr1"), cigar=one)
    c("xf_three_fields", "DDDD", xf("1 chr1-chr2 1001"), cigar=one)
    c("xf_empty", "DDDD", xf(""), cigar=SPL)
    c("xf_second_part", "DDDD", fus("20M5000F10M", part="2"), cigar=SPL)
    c("xf_last_wins", "DDKK", fus("20M5000F10M", part="2") + fus("20M5000F10m"), cigar=one)
    c("xf_as_H_is_no_xf", "DDKK", xf("2 chr1-chr2 1001 20M5000F10M", ty="H"), cigar=one)
    c("xf_blanks_doubled", "DDKK", xf("1  chr1--chr2-x   1001  20M5000F10M"), cigar=one)
    c("xf_ins_without_bases", "DLKL", fus("10M2I10M100F5M"), cigar=one)
    c("xf_ins_letters_from_tag", "DKKK", fus("10M2I10M100F5M", "ACGTACGTACTTACGTACGTACGTACG"), cigar=[cw(M, 10), cw(I, 2), cw(M, 13)], seq=seq(25, 10, 15))
    c("xf_ins_letter_lower_case", "DLKL", fus("10M2I10M100F5M", "ACGTACGTACttACGTACGTACGTACG"), cigar=one)
    c("xf_pos_signed", "DDKK", xf("1 chr1-chr2 +700 20m5000F10M"), cigar=one)
    # ---- read keys (fusions collected): QNAME up to the first NUL, and the 0x40 / 0x80 bits
    for k in range(3):
        c("read_a_%d" % k, "DDKK", cigar=one, name="read_a", pos=2000 + 100 * k, flag=0x40)
    c("read_a_mate", "DDKK", cigar=one, name="read_a", flag=0x80)
    c("read_a_unpaired", "DDKK", cigar=one, name="read_a")
    c("read_nul_inside", "DDKK", cigar=one, name=b"read_a\0tail")
    c("read_a_dropped_between", "DDDD", cigar=one, name="read_b", tid=2)
    c("read_a_again", "DDKK", cigar=one, name="read_a")
    return out


CASES = _cases()
LABELS = [c[0] for c in CASES]
assert len(set(LABELS)) == len(LABELS)

# what some records become, by hand: label -> (ref_id, left, flags, edit_dist, [(op, length) ...], ref_id2 or 0, letters with indels on)
BY_HAND = {
    "nm_c_neg": (1, 1000, 0, 0, [(1, 10), (11, 300), (1, 15)], 0, ""),
    "nm_s_300": (1, 1000, 0, 255, [(1, 10), (11, 300), (1, 15)], 0, ""),
    "nm_twice": (1, 1000, 0, 9, [(1, 10), (11, 300), (1, 15)], 0, ""),
    "nm_I_big": (1, 1000, 0, 255, [(1, 10), (11, 300), (1, 15)], 0, ""),
    "xs_minus_then_plus": (1, 1000, 0, 0, [(1, 10), (11, 300), (1, 15)], 0, ""),
    "xs_plus_then_minus": (1, 1000, 4, 0, [(1, 10), (11, 300), (1, 15)], 0, ""),
    "tags_before": (1, 1000, 4, 4, [(1, 10), (11, 300), (1, 15)], 0, ""),
    "unknown_type_last": (1, 1000, 4, 2, [(1, 10), (11, 300), (1, 15)], 0, ""),
    "unknown_type_first": (1, 1000, 0, 0, [(1, 10), (11, 300), (1, 15)], 0, ""),
    "ops_eq_x": (1, 1000, 0, 0, [(1, 5), (1, 3), (11, 300), (1, 10)], 0, ""),
    "ops_S_H_P": (1, 1000, 0, 0, [(14, 2), (13, 3), (1, 10), (11, 300), (1, 10), (15, 2), (13, 2)], 0, ""),
    "ops_code_9_and_15": (1, 1000, 0, 0, [(1, 10), (15, 5), (11, 300), (15, 1), (1, 15)], 0, ""),
    "on_chr2": (2, 777, 0, 0, [(1, 10), (11, 300), (1, 15)], 0, ""),
    "ins_even": (1, 1000, 0, 0, [(1, 10), (3, 2), (1, 13)], 0, LETTERS[10:12]),
    "ins_odd": (1, 1000, 0, 0, [(1, 11), (3, 2), (1, 12)], 0, LETTERS[11:13]),
    "ins_on_last_base": (1, 1000, 0, 0, [(1, 23), (3, 2)], 0, LETTERS[23:25]),
    "ins_behind_clip": (1, 1000, 0, 0, [(13, 3), (1, 10), (3, 2), (1, 10)], 0, LETTERS[10:12]),
    "ins_twice": (1, 1000, 0, 0, [(1, 4), (3, 1), (1, 4), (3, 3), (1, 13)], 0, LETTERS[4:5] + LETTERS[9:12]),
    "ins_letter_N": (1, 1000, 0, 0, [(1, 10), (3, 2), (1, 13)], 0, "N" + LETTERS[11]),
    "xf_ff": (1, 1000, 0, 1, [(1, 20), (7, 4999), (1, 10)], 2, ""),
    "xf_fr": (1, 1000, 0, 0, [(1, 20), (8, 4999), (2, 10)], 2, ""),
    "xf_rf": (1, 1000, 0, 0, [(2, 20), (9, 4999), (1, 10)], 2, ""),
    "xf_rr": (1, 1000, 0, 0, [(2, 20), (10, 4999), (2, 10)], 2, ""),
    "xf_same_contig_swapped": (2, 1000, 0, 0, [(1, 20), (7, 99), (1, 10)], 1, ""),
    "xf_F_first": (1, 1000, 0, 0, [(7, 4999), (1, 10), (1, 20)], 2, ""),
    "xf_pieces": (1, 1000, 4, 0, [(1, 10), (3, 2), (1, 8), (11, 100), (1, 5), (8, 4999), (2, 4), (6, 3), (4, 2), (12, 50), (2, 6)], 2, LETTERS[10:12] + LETTERS[29:31]),
    "xf_last_wins": (1, 1000, 0, 0, [(1, 20), (8, 4999), (2, 10)], 2, ""),
    "xf_blanks_doubled": (1, 1000, 0, 0, [(1, 20), (7, 4999), (1, 10)], 2, ""),
    "xf_ins_letters_from_tag": (1, 1000, 0, 0, [(1, 10), (3, 2), (1, 10), (7, 99), (1, 5)], 2, "TT"),
    "xf_pos_signed": (1, 699, 0, 0, [(2, 20), (9, 4999), (1, 10)], 2, ""),
    "xf_as_H_is_no_xf": (1, 1000, 0, 0, [(1, 25)], 0, ""),
}
# the runs of kept records with fusions collected: read_a x3 | its mate | unpaired: two spellings of one name and, a dropped record
# between, the same read again -- one run of three
READ_RUN_HEADS = {"read_a_0": 1, "read_a_1": 0, "read_a_2": 0, "read_a_mate": 1, "read_a_unpaired": 1, "read_nul_inside": 0, "read_a_again": 0}
LOUD_WHAT = {"tag_past_end_i": "malformed", "tag_past_end_d": "malformed", "tag_past_end_B_header": "malformed", "tag_B_count_negative": "malformed",
             "tag_B_count_huge": "malformed", "header_does_not_fit": "malformed", "cigar_17_spliced": "cigar_ops", "cigar_17_unspliced": "cigar_ops",
             "cigar_17_gapped": "cigar_ops", "ins_one_past": "ins_range", "ins_17": "ins_long", "ins_letter_M": "ins_letter", "xf_16_ops": "xf_ops",
             "xf_ins_without_bases": "ins_range", "xf_ins_letter_lower_case": "ins_letter"}


def quiet(mode):
    """the cases that do not end the run in MODES[mode]"""
    return [c for c in CASES if c[1][mode] != "L"]


def write(path, cases, per_member=None, **kw):
    """the cases' records as a BAM file: one member, or members of per_member records"""
    recs = [c[2] for c in cases]
    per = per_member or max(1, len(recs))
    members = [(recs[i:i + per], 6) for i in range(0, len(recs), per)] or [([], 6)]
    return write_bam(path, members, targets=TARGETS, **kw)
