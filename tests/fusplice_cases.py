"""Test-only: planted junction-db ("spliced") segment maps whose targets are fusion contigs -- one record per decision of the fusion
branch of SplicedBAMHitFactory::get_hit_from_buf / spliceCigar (bwt_map.cpp:1664-1759, :681-865), per direction, each with a label
and with what must become of it --, beside splice_cases.py, whose map writer, restatement reading and id window these reuse.  Pure
Python, no GPU.

Coordinates: an ff / fr target `chr1-chr2|975|999-2000|2025|fus|..` is the 25 bases of chr1 up to 999 followed by 25 bases of chr2 at
2000; a record at 0-based contig offset p starts at 975 + p, and the break lies 1000 - (975 + p) bases into it.  An rf / rr target
`chr1-chr2|1024|1000-..` runs DOWN chr1 from 1024 to 1000: the record starts at 1024 - p, and the break lies (1024 - p) - 999 bases
into it -- the same 25 - p."""
import splice_cases as sc
from splice_cases import BEGIN_ID, END_ID, KNOWN, REF_IDS, hit_row, restated, write_map  # noqa: F401  (the tests' one door)
from tophat_amd.samtext import parse_spliced_sam_hits
from ingest_cases import MAX_INTRON

FF = "chr1-chr2|975|999-2000|2025|fus|ff"
FR = "chr1-chr2|975|999-2024|2000|fus|fr"
RF = "chr1-chr2|1024|1000-2000|2025|fus|rf"
RR = "chr1-chr2|1024|1000-2024|2000|fus|rr"
U2 = "chr1-chrU|975|999-2000|2025|fus|ff"              # the second contig is one the run does not know
U1 = "chrU-chr2|975|999-2000|2025|fus|ff"              # the first one
ONE_CONTIG = "chr1|975|999-2000|2025|fus|ff"           # the contig field is not two parts: THJ_JUNCDB_INVALID
J_FWD = sc.J_FWD                                       # a junction target: plain and fused records share a map
DIRS = (("ff", FF), ("fr", FR), ("rf", RF), ("rr", RR))
TARGETS = (FF, FR, RF, RR, U2, U1, ONE_CONTIG, J_FWD)

KEPT, DROPPED, LOUD = sc.KEPT, sc.DROPPED, "a fused hit's fifth operation"
FUSED, FLIPPED, ANTISENSE, END = 16, 8, 1, 2
# the fusion operation per direction: (CigarOpCode, length = the target's second splice position as it stands)
FUSION_OP = {"ff": (7, 2000), "fr": (8, 2024), "rf": (9, 2000), "rr": (10, 2024)}
BEFORE = {"ff": 1, "fr": 1, "rf": 2, "rr": 2}          # MATCH / mATCH of the piece before the break ...
AFTER = {"ff": 1, "fr": 2, "rf": 1, "rr": 2}           # ... and after it


def cases():
    """[(label, outcome, id, SAM fields)] in id order; the quiet records first, the loud ones last"""
    out, loud = [], []

    def add(label, outcome, target, pos0, cigar, md="25", flag=0, name_tail="|0:0:4"):
        (loud if outcome == LOUD else out).append((label, outcome, target, pos0, cigar, md, flag, name_tail))

    for d, tg in DIRS:
        add("fus_%s_inside_M" % d, KEPT, tg, 10, "25M")
        add("fus_%s_antisense_mismatch" % d, KEPT, tg, 3, "25M", "3A21", flag=16)
        add("fus_%s_ends_at_break" % d, DROPPED, tg, 0, "25M")
        add("fus_%s_starts_at_break" % d, DROPPED, tg, 25, "25M")
        add("fus_%s_one_base_before" % d, KEPT, tg, 24, "25M")
        add("fus_%s_one_base_after" % d, KEPT, tg, 1, "25M")
        add("fus_%s_H_skipped" % d, KEPT, tg, 10, "2H25M3H")
        add("fus_%s_last_segment" % d, KEPT, tg, 10, "25M", name_tail="|75:3:4")
        # the break exactly between two operations: the fusion operation goes in between, nothing is split, and the size test drops it
        add("fus_%s_on_boundary" % d, DROPPED, tg, 10, "15M1I9M", "24")
        add("fus_%s_S_first" % d, DROPPED, tg, 10, "3S22M", "22")
        add("fus_%s_I_before_break" % d, LOUD, tg, 10, "5M1I19M", "24")         # 5M 1I 10M F 9M
        add("fus_%s_I_after_break" % d, LOUD, tg, 10, "17M1I7M", "24")          # 15M F 2M 1I 7M
        add("fus_%s_I_and_D" % d, LOUD, tg, 10, "5M1I5M1D14M", "10^A14")        # seven operations
    add("junc_plain", KEPT, J_FWD, 10, "25M")
    add("one_contig_25M", DROPPED, ONE_CONTIG, 10, "25M")
    add("one_contig_indel", DROPPED, ONE_CONTIG, 10, "5M1I19M", "24")
    add("unknown_second_contig", DROPPED, U2, 10, "25M")
    add("unknown_first_contig", DROPPED, U1, 10, "25M")
    add("unknown_second_contig_five_ops", DROPPED, U2, 10, "5M1I19M", "24")     # ref_id2 == 0 is looked at before the operations are counted
    add("unknown_first_contig_five_ops", LOUD, U1, 10, "5M1I19M", "24")         # ... ref_id == 0 after
    recs = []
    for k, (label, outcome, target, pos0, cigar, md, flag, name_tail) in enumerate(out + loud):
        rid = BEGIN_ID + k
        recs.append((label, outcome, rid, ["%d%s" % (rid, name_tail), str(flag), target, str(pos0 + 1), "255", cigar, "*", "0", "0", sc._seq(25), "I" * 25,
                                           "NM:i:0", "MD:Z:" + md]))
    return recs


def _fused(d, n_before, n_after):
    return [(BEFORE[d], n_before), FUSION_OP[d], (AFTER[d], n_after)]


# what the kept records must be, written out: label -> (left, operations, flags, mismatches); cigar[4] is chr2's id, 2, on every one
EXPECTED = {"junc_plain": (985, [(1, 15), (11, 500), (1, 10)], 0, 0)}
for _d, _down in (("ff", False), ("fr", False), ("rf", True), ("rr", True)):
    _fl = FUSED | ((FLIPPED | ANTISENSE) if _down else 0)
    _at = (lambda p, down=_down: 1024 - p if down else 975 + p)
    EXPECTED["fus_%s_inside_M" % _d] = (_at(10), _fused(_d, 15, 10), _fl, 0)
    # record flag 0x10: antisense on ff / fr, and flipped back to sense on rf / rr
    EXPECTED["fus_%s_antisense_mismatch" % _d] = (_at(3), _fused(_d, 22, 3), _fl ^ ANTISENSE, 1)
    EXPECTED["fus_%s_one_base_before" % _d] = (_at(24), _fused(_d, 1, 24), _fl, 0)
    EXPECTED["fus_%s_one_base_after" % _d] = (_at(1), _fused(_d, 24, 1), _fl, 0)
    EXPECTED["fus_%s_H_skipped" % _d] = (_at(10), _fused(_d, 15, 10), _fl, 0)
    EXPECTED["fus_%s_last_segment" % _d] = (_at(10), _fused(_d, 15, 10), _fl | END, 0)
# ... and by hand, the issue's own table, so that the loop above is not the only statement of it
BY_HAND = {
    "fus_ff_inside_M": (985, [(1, 15), (7, 2000), (1, 10)], 16, 0), "fus_fr_inside_M": (985, [(1, 15), (8, 2024), (2, 10)], 16, 0),
    "fus_rf_inside_M": (1014, [(2, 15), (9, 2000), (1, 10)], 25, 0), "fus_rr_inside_M": (1014, [(2, 15), (10, 2024), (2, 10)], 25, 0),
    "fus_ff_antisense_mismatch": (978, [(1, 22), (7, 2000), (1, 3)], 17, 1), "fus_fr_antisense_mismatch": (978, [(1, 22), (8, 2024), (2, 3)], 17, 1),
    "fus_rf_antisense_mismatch": (1021, [(2, 22), (9, 2000), (1, 3)], 24, 1), "fus_rr_antisense_mismatch": (1021, [(2, 22), (10, 2024), (2, 3)], 24, 1),
    "fus_ff_one_base_before": (999, [(1, 1), (7, 2000), (1, 24)], 16, 0), "fus_ff_one_base_after": (976, [(1, 24), (7, 2000), (1, 1)], 16, 0),
}
# the restatement's operations of the loud records (it has no limit of its own): what makes them loud
LOUD_OPS = {
    "fus_ff_I_before_break": [(1, 5), (3, 1), (1, 10), (7, 2000), (1, 9)],
    "fus_fr_I_after_break": [(1, 15), (8, 2024), (2, 2), (4, 1), (2, 7)],              # INS comes out lower-case behind an fr break
    "fus_rf_I_before_break": [(2, 5), (4, 1), (2, 10), (9, 2000), (1, 9)],             # ... and before an rf break
    "fus_rr_I_and_D": [(2, 5), (4, 1), (2, 5), (6, 1), (2, 4), (10, 2024), (2, 10)],
}
LOUD_N_OPS = {"I_before_break": 5, "I_after_break": 5, "I_and_D": 7, "unknown_first_contig_five_ops": 5}


def restated_raw(sam):
    """every hit the restatement makes of the map, whatever its contigs and however many operations: id -> HitRec"""
    return {h[0]: h for h in parse_spliced_sam_hits(sam, sc._Refs(REF_IDS), max_report_intron=MAX_INTRON)}


def restated_quiet(sam, begin_id=BEGIN_ID, end_id=END_ID):
    """splice_cases.restated for a map without loud records: what the factory hands to the stream"""
    return restated(sam, begin_id, end_id)


# ---------------------------------------------------------------------------------------------------------------- merge table
def merge_maps(dirname):
    """splice_cases.merge_maps with the spliced maps' records alternating between the junction targets and fusion targets of all
    four directions -> (contig sam/bam pairs x4, spliced sam/bam pairs x3)"""
    contig, _ = sc.merge_maps(dirname)
    cycle = (J_FWD, FF, RF, J_FWD, FR, RR)
    spliced = []
    n = 0
    for s in range(3):
        recs = []
        for rid in sorted(sc.MERGE_SPLICED):
            for j in range(sc.MERGE_SPLICED[rid][s]):
                recs.append(["%d|%d:%d:4" % (rid, 25 * s, s), str(16 * (j % 2)), cycle[n % len(cycle)], str(5 + (rid + 3 * j) % 15 + 1), "255", "25M", "*", "0", "0",
                             sc._seq(25), "I" * 25, "NM:i:0", "MD:Z:" + ("25", "7A17")[j % 2]])
                n += 1
        spliced.append(write_map(dirname, "fusmerge_seg%d.to_spliced" % s, recs, TARGETS))
    return contig, spliced
