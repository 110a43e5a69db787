"""Test-only: planted junction-db ("spliced") segment maps for the spliced hit factory -- one record per decision of
SplicedBAMHitFactory::get_hit_from_buf / spliceCigar / getBAMmismatches, each with a label and with what must become of it --, the
reading of the Python restatement (tophat_amd/samtext.py: parse_spliced_sam_hits) in the form the ingest hands out, and a merge
table of contig and spliced maps.  Pure Python, no GPU.  Records are written as SAM text; tophat_amd.bamio.write_bam_from_sam makes
the BAM the factories read.

Coordinates: a junction target `chr1|975|999-1500|1525|GTAG|fwd` is the 25 bases up to 999 followed by the 25 bases from 1500; a
record at 0-based contig offset p starts at genome position 975 + p, and the splice lies 1000 - (975 + p) bases into it."""
import os

import numpy as np

from ingest_cases import MAX_INTRON
from tophat_amd.bamio import write_bam_from_sam
from tophat_amd.batch import SPAN_HIT_DTYPE, span_hit_struct
from tophat_amd.samtext import parse_spliced_sam_hits

KNOWN = "chr1,chr2,chr|X"                               # the contigs the run knows, ids 1..3; chrU is in no header
REF_IDS = {"chr1": 1, "chr2": 2, "chr|X": 3}
BEGIN_ID = 10                                          # the shard: ids in [BEGIN_ID, END_ID)
END_ID = 0xFFFFFFFF

J_FWD = "chr1|975|999-1500|1525|GTAG|fwd"
J_REV = "chr2|1975|1999-2300|2325|GTAG|rev"
J_PIPE = "chr|X|975|999-1500|1525|GTAG|fwd"            # a contig name with '|' in it
J_WIDE = "chr1|7951|7999-8500|8549|GTAG|fwd"           # 49-base flanks: a read's last segment
DEL = "chr1|2975|2999-3004|3029|del|fwd"               # deletes 3000..3003
INS3 = "chr1|4975|4999-ACG|5025|ins|fwd"
INS1 = "chr1|5975|5999-T|6025|ins|fwd"
INS6 = "chr2|6975|6999-ACGTAC|7025|ins|rev"
INS_XYZ = "chr1|4975|4999-ACG|5025|ins|xyz"
INS_WIDE = "chr1|9873|9999-ACG|10127|ins|fwd"          # segment length 64: 127-base flanks
T_FIVE = "chr1|975|999-1500|1525|GTAG"                 # five fields
T_ONE_PART = "chr1|975|999|1525|GTAG|fwd"              # `l-r` is one part
T_STRAND = "chr1|975|999-1500|1525|GTAG|xyz"           # an unknown strand word
T_UNKNOWN = "chrU|975|999-1500|1525|GTAG|fwd"          # a contig the run does not know
FUS = "chr1-chr2|975|999-2000|2025|fus|ff"
TARGETS = (J_FWD, J_REV, J_PIPE, J_WIDE, DEL, INS3, INS1, INS6, INS_WIDE, INS_XYZ, T_FIVE, T_ONE_PART, T_STRAND, T_UNKNOWN, FUS)

KEPT, DROPPED, SIX_OPS, FALLBACK = "kept", "dropped", "six operations", "fallback"


def _seq(n):
    return ("ACGTTGCA" * 16)[:n]


def cases():
    """[(label, outcome, id, SAM fields)] in id order.  outcome: KEPT / DROPPED by the factory, SIX_OPS (the loud outcome), FALLBACK (a
    fusion contig).  The expected CIGAR of a kept record is in `CIGARS`."""
    out = []

    def add(label, outcome, target, pos0, cigar, md="", flag=0, rnext="*", n=25, rid=None, name_tail="|0:0:4"):
        rid = (BEGIN_ID + len(out)) if rid is None else rid
        tags = ["NM:i:0"] + (["MD:Z:" + md] if md is not None else [])
        out.append((label, outcome, rid, ["%d%s" % (rid, name_tail), str(flag), target, str(pos0 + 1), "255", cigar, rnext, "0", "0", _seq(n), "I" * n] + tags))

    add("id_below_begin", DROPPED, J_FWD, 10, "25M", "25", rid=5)
    # ---- junction targets
    for tg, sd in ((J_FWD, "fwd"), (J_REV, "rev")):
        add("junc_%s_inside_M" % sd, KEPT, tg, 10, "25M", "25")
        add("junc_%s_inside_M_antisense" % sd, KEPT, tg, 3, "25M", "25", flag=16)
        add("junc_%s_ends_at_splice" % sd, DROPPED, tg, 0, "25M", "25")
        add("junc_%s_starts_at_splice" % sd, DROPPED, tg, 25, "25M", "25")
        add("junc_%s_starts_after_splice" % sd, DROPPED, tg, 30, "20M", "20", n=20)
        # the splice exactly between two operations: the gap operation goes in between, nothing is split, and the size test drops it
        add("junc_%s_on_boundary_before_I" % sd, DROPPED, tg, 10, "15M1I9M", "24")
        add("junc_%s_on_boundary_before_D" % sd, DROPPED, tg, 10, "15M2D8M", "15^AC8", n=23)
        add("junc_%s_in_second_M_after_I" % sd, KEPT, tg, 10, "5M1I19M", "24")
        add("junc_%s_in_second_M_after_D" % sd, KEPT, tg, 10, "5M2D18M", "5^AC18", n=23)
        add("junc_%s_S_first" % sd, DROPPED, tg, 10, "3S22M", "22")
        add("junc_%s_H_skipped" % sd, KEPT, tg, 10, "2H25M3H", "25")
        add("junc_%s_P" % sd, KEPT, tg, 10, "10M2P15M", "25")
    add("junc_contig_with_pipe", KEPT, J_PIPE, 10, "25M", "25")
    add("junc_not_the_last_segment", KEPT, J_FWD, 12, "25M", "25", name_tail="|25:1:4")
    add("junc_last_segment", KEPT, J_FWD, 12, "25M", "25", name_tail="|75:3:4")
    # ---- deletion targets
    add("del_plain", KEPT, DEL, 10, "25M", "25")
    add("del_input_D_ends_at_the_deletion", DROPPED, DEL, 10, "10M5D10M", "10^ACGTA10", n=20)       # cigar_add: 5D becomes 9D and 4D is appended again
    add("del_inside_an_input_D", KEPT, DEL, 12, "10M6D10M", "10^ACGTAC10", n=20)                   # 10M 7D 7D 3D 10M: extended AND appended, twice
    # ---- insertion targets
    add("ins_whole", KEPT, INS3, 10, "25M", "25")
    # a record that starts inside the inserted bases has left > lsp: the early out drops it like any other, so spliceCigar's arm for
    # spl_ofs < 0 (the shortened insertion) is never entered -- not by this record, not by any
    add("ins_starts_inside", DROPPED, INS3, 26, "20M", "20", n=20)
    add("ins_ends_inside", DROPPED, INS3, 1, "25M", "25")
    add("ins_left_after_lsp", DROPPED, INS3, 30, "20M", "20", n=20)
    add("ins_left_at_lsp", KEPT, INS3, 24, "25M", "25")
    add("ins_mismatch_inside_and_outside", KEPT, INS3, 10, "25M", "3A12C8")
    add("ins_one_base", KEPT, INS1, 10, "25M", "15G9")
    add("ins_six_bases", KEPT, INS6, 10, "25M", "2A17C4")
    add("ins_unknown_strand_word", KEPT, INS_XYZ, 10, "25M", "25")          # the BAM factory checks the strand word of the other types only
    # ---- MD
    add("md_absent", KEPT, J_FWD, 10, "25M", None)
    add("md_25", KEPT, J_FWD, 10, "25M", "25")
    add("md_leading_zero", KEPT, J_FWD, 10, "25M", "0A24")
    add("md_two_adjacent", KEPT, J_FWD, 10, "25M", "5AC18")
    add("md_deletion_letters", KEPT, J_FWD, 10, "10M2D13M", "10^AC5T7", n=23)
    add("md_last_base", KEPT, J_FWD, 10, "25M", "24A")
    add("md_all_mismatches", KEPT, J_FWD, 10, "25M", "A" * 25)
    add("md_49_base_last_segment", KEPT, J_WIDE, 20, "49M", "30C17G", n=49, name_tail="|75:3:4")
    add("md_127_bases_mismatch_past_bit_64", KEPT, INS_WIDE, 50, "127M", "78A21C26", n=127, name_tail="|0:0:2")
    # ---- dropped records
    add("flag_4", DROPPED, J_FWD, 10, "25M", "25", flag=4)
    add("no_target", DROPPED, "*", -1, "25M", "25")
    add("mate_on_another_target", DROPPED, J_FWD, 10, "25M", "25", rnext=J_REV)
    add("mate_on_the_same_target", KEPT, J_FWD, 10, "25M", "25", rnext="=")
    add("zero_length_op", DROPPED, J_FWD, 10, "10M0I15M", "25")
    add("op_EQ", DROPPED, J_FWD, 10, "10=15M", "25")
    add("N_at_the_limit", KEPT, J_FWD, 10, "20M%dN5M" % MAX_INTRON, "25")
    add("N_above_the_limit", DROPPED, J_FWD, 10, "20M%dN5M" % (MAX_INTRON + 1), "25")
    add("target_of_five_fields", DROPPED, T_FIVE, 10, "25M", "25")
    add("target_l_r_one_part", DROPPED, T_ONE_PART, 10, "25M", "25")
    add("target_unknown_strand_word", DROPPED, T_STRAND, 10, "25M", "25")
    add("target_on_unknown_contig", DROPPED, T_UNKNOWN, 10, "25M", "25")
    # ---- the loud outcomes, last: each also goes into a map of its own
    rid = BEGIN_ID + len(out)
    out.append(("six_ops", SIX_OPS, rid, ["%d|0:0:4" % rid, "0", J_FWD, "11", "255", "5M1I5M1D14M", "*", "0", "0", _seq(25), "I" * 25, "NM:i:0", "MD:Z:10^A14"]))
    out.append(("fus_target", FALLBACK, rid + 1, ["%d|0:0:4" % (rid + 1), "0", FUS, "11", "255", "25M", "*", "0", "0", _seq(25), "I" * 25, "NM:i:0", "MD:Z:25"]))
    return out


# what the kept records' CIGARs must be: (CigarOpCode, length) with 1 MATCH, 3 INS, 5 DEL, 11 REF_SKIP, 15 PAD
CIGARS = {
    "junc_fwd_inside_M": [(1, 15), (11, 500), (1, 10)], "junc_rev_inside_M": [(1, 15), (11, 300), (1, 10)],
    "junc_fwd_inside_M_antisense": [(1, 22), (11, 500), (1, 3)],
    "junc_fwd_in_second_M_after_I": [(1, 5), (3, 1), (1, 10), (11, 500), (1, 9)],
    "junc_fwd_in_second_M_after_D": [(1, 5), (5, 2), (1, 8), (11, 500), (1, 10)],
    "junc_fwd_H_skipped": [(1, 15), (11, 500), (1, 10)],
    "junc_fwd_P": [(1, 10), (15, 2), (1, 3), (11, 500), (1, 12)],
    "del_plain": [(1, 15), (5, 4), (1, 10)],
    "del_inside_an_input_D": [(1, 10), (5, 7), (5, 7), (5, 3), (1, 10)],
    "ins_whole": [(1, 15), (3, 3), (1, 7)], "ins_left_at_lsp": [(1, 1), (3, 3), (1, 21)],
    "ins_one_base": [(1, 15), (3, 1), (1, 9)], "ins_six_bases": [(1, 15), (3, 6), (1, 4)], "ins_unknown_strand_word": [(1, 15), (3, 3), (1, 7)],
    "md_49_base_last_segment": [(1, 29), (11, 500), (1, 20)],
    "md_127_bases_mismatch_past_bit_64": [(1, 77), (3, 3), (1, 47)],
    "N_at_the_limit": [(1, 15), (11, 500), (1, 5), (11, MAX_INTRON), (1, 5)],
}
# (mismatches, edit_dist) where the MD string matters
MISMATCHES = {
    "ins_mismatch_inside_and_outside": (1, 4),         # two in MD, the one inside the inserted bases is taken off; + 3 inserted
    "ins_one_base": (0, 1),                            # the only mismatch is the inserted base
    "ins_six_bases": (1, 7),                           # of the mismatches at 2 and 20 the second lies in the inserted bases (15..20)
    "md_absent": (0, 0), "md_25": (0, 0), "md_leading_zero": (1, 1), "md_two_adjacent": (2, 2), "md_deletion_letters": (1, 3), "md_last_base": (1, 1),
    "md_all_mismatches": (25, 25),
    "md_49_base_last_segment": (2, 2),
    "md_127_bases_mismatch_past_bit_64": (1, 4),       # the mismatch at read offset 78 lies in the inserted bases (77..79)
    "del_plain": (0, 4), "del_inside_an_input_D": (0, 17),
}


def sam_text(recs, targets=TARGETS):
    return ("@HD\tVN:1.0\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:300\n" % t for t in targets) + "".join("\t".join(f) + "\n" for f in recs))


def write_map(dirname, name, recs, targets=TARGETS):
    """-> (sam path, bam path)"""
    sam, bam = os.path.join(dirname, name + ".sam"), os.path.join(dirname, name + ".bam")
    with open(sam, "w") as f:
        f.write(sam_text(recs, targets))
    write_bam_from_sam(sam, bam)
    return sam, bam


class _Refs(dict):                                     # an unknown contig is id 0: the factories drop its records at the very end
    def __missing__(self, k):
        return 0


def restated(sam, begin_id=BEGIN_ID, end_id=END_ID, max_ops=None):
    """the restatement's hits of a SAM map, as the factory hands them to the stream: id 0, ids outside the shard and unknown contigs gone.
    -> [HitRec]; max_ops: leave out hits of more operations (the loud outcome is somebody else's to check)"""
    out = []
    for h in parse_spliced_sam_hits(sam, _Refs(REF_IDS), max_report_intron=MAX_INTRON):
        if h[0] == 0 or not (begin_id <= h[0] < end_id) or h[1] == 0 or (len(h) > 11 and h[11] == 0):
            continue
        if max_ops is not None and len(h[9]) > max_ops:
            continue
        out.append(h)
    return out


def hit_row(h):
    """a HitRec -> (ref_id, left, flags, mismatches, edit_dist, n_cigar, c0..c4): thj_span_hit's fields"""
    ref, left, flags, mm, ed, n, cig = span_hit_struct(h)
    return (ref, left, flags, mm, ed, n) + tuple(cig)


def hits_array(hs):
    return np.array([span_hit_struct(h) for h in hs], dtype=SPAN_HIT_DTYPE) if hs else np.zeros(0, dtype=SPAN_HIT_DTYPE)


# ---------------------------------------------------------------------------------------------------------------- merge table
MERGE_NSEG = 4
# id -> hits per segment in the contig maps / in the spliced maps (three spliced maps for four segments)
MERGE_CONTIG = {20: (1, 1, 1, 1), 21: (2, 0, 1, 0), 23: (1, 2, 0, 1), 24: (0, 1, 1, 0), 25: (1, 0, 0, 0), 27: (3, 1, 1, 1), 28: (0, 0, 1, 1), 30: (1, 1, 1, 1),
                31: (1, 1, 0, 2), 35: (2, 2, 2, 2), 36: (0, 2, 0, 0)}
MERGE_SPLICED = {18: (1, 0, 1), 22: (1, 0, 0), 23: (2, 1, 1), 24: (0, 0, 2), 26: (0, 1, 0), 27: (1, 0, 2), 29: (0, 0, 1), 30: (0, 3, 0), 32: (2, 1, 0),
                 35: (1, 1, 1), 36: (0, 1, 0), 40: (1, 0, 0)}
# contig hits only: 20 21 25 31; spliced only in segment 0: 22 32 (rows); both in one segment: 23 27 35; spliced only in a later segment and
# nothing in segment 0: 26 29 (no row), with contig hits in later segments only: 24 28 36 (no row); lowest / highest id only in the spliced map: 18 / 40
MERGE_WINDOWS = ((BEGIN_ID, END_ID), (23, 36), (33, 35), (19, 40))           # (33, 35): empty


def merge_maps(dirname):
    """-> (contig sam/bam pairs x4, spliced sam/bam pairs x3): plain 25M contig hits, spliced hits on the junction targets"""
    contig, spliced = [], []
    hdr = "@HD\tVN:1.0\tSO:unsorted\n@SQ\tSN:chr1\tLN:1000000\n@SQ\tSN:chr2\tLN:1000000\n"
    for s in range(MERGE_NSEG):
        lines = []
        for rid in sorted(MERGE_CONTIG):
            for j in range(MERGE_CONTIG[rid][s]):
                lines.append("\t".join(["%d|%d:%d:4" % (rid, 25 * s, s), str(16 * (j % 2)), "chr%d" % (1 + j % 2), str(1000 * s + 40 * rid + j + 1), "255", "25M", "*", "0", "0",
                                        _seq(25), "I" * 25, "NM:i:%d" % (j % 3)]))
        sam, bam = os.path.join(dirname, "merge_seg%d.sam" % s), os.path.join(dirname, "merge_seg%d.bam" % s)
        with open(sam, "w") as f:
            f.write(hdr + "".join(l + "\n" for l in lines))
        write_bam_from_sam(sam, bam)
        contig.append((sam, bam))
    for s in range(3):
        recs = []
        for rid in sorted(MERGE_SPLICED):
            for j in range(MERGE_SPLICED[rid][s]):
                recs.append(["%d|%d:%d:4" % (rid, 25 * s, s), str(16 * (j % 2)), (J_FWD, J_REV, DEL)[(rid + j) % 3], str(5 + (rid + 3 * j) % 15 + 1), "255", "25M", "*", "0", "0",
                             _seq(25), "I" * 25, "NM:i:0", "MD:Z:" + ("25", "7A17")[j % 2]])
        spliced.append(write_map(dirname, "merge_seg%d.to_spliced" % s, recs))
    return contig, spliced
