"""CPU: the reference reading of planted BAM records (ingest_ref.py, restated from get_hit_from_buf and the samtools accessors it
calls) against the host parser (thj_hostio.h: parse_hit_bam, through `hostio_check hitdump`) and, on the golden cases, against
samtext.parse_sam_hits.  The GPU tests (test_gpu_ingest_records.py) compare the device ingest with the same reading; this file
checks that reading, and that the case tables reach every branch, before any GPU sees them."""
import gzip
import os
import subprocess

import pytest

import ingest_cases as ic
import ingest_ref as ir
from golden_util import CASES, GOLD
from locked_make import locked_make
from tophat_amd.bamio import write_bam_from_sam
from tophat_amd.batch import hit_tuple_to_struct, span_hit_struct
from tophat_amd.samtext import parse_header, parse_sam_hits

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "hostio", "hostio_check")


@pytest.fixture(scope="module")
def exe():
    locked_make(os.path.join(HERE, "hostio"))
    return EXE


def hitdump(exe, path, known=ic.KNOWN):
    """one child per file: die() exits"""
    r = subprocess.run([exe, "hitdump", path, str(ic.MAX_INTRON), known], capture_output=True, text=True)
    return r.returncode, r.stdout.splitlines(), r.stderr


def dump_line(h):
    """the line `hostio_check hitdump` prints for what hit_from_record returned"""
    if h[0] != "keep":
        return "D %d" % h[1]
    t = h[1]
    a, b = hit_tuple_to_struct(t), span_hit_struct(t)
    return "K %d %d %d %d %d %d %d %d %d %d %d %d %s" % ((t[0],) + tuple(a) + (b[2], b[3], b[4], b[5], " ".join("%d" % x for x in b[6])))


@pytest.fixture(scope="module")
def parser_file(tmp_path_factory):
    recs = ic.parser_records()
    w = ic.write_bam(str(tmp_path_factory.mktemp("parser") / "parser.bam"), [([r for _, r in recs[:60]], 6), ([r for _, r in recs[60:]], 0)])
    return recs, w


def test_parser_table_reads_like_the_host_parser(exe, parser_file):
    recs, w = parser_file
    rc, lines, err = hitdump(exe, w.path)
    assert rc == 0, err
    assert len(lines) == len(recs)
    for (label, r), got in zip(recs, lines):
        want = dump_line(ir.hit_from_record(r[4:], ic.TID2REF, ic.MAX_INTRON))
        assert got == want, label


# what the REFERENCE gives where reading the two parsers against it found them different (both were changed to it): the case's whole
# hitdump line, worked out by hand from bwt_map.cpp:1101-1452 and bam_aux.c
M25 = (1 << 28) | 25
SPL_CIG = "%d %d %d 0 0" % ((1 << 28) | 10, (11 << 28) | 300, (1 << 28) | 15)
FINDINGS = {
    # '=' and 'X' have no arm in the CIGAR switch (:1330-1350): "invalid CIGAR operation", the record is dropped
    "op_EQ": "D %(id)d",
    "op_X": "D %(id)d",
    # bam_aux_get returns the FIRST tag of a name; bam_aux2i / bam_aux2A give 0 for a type that is not theirs
    "nm_twice": "K %(id)d 1 %(pos)d %(right)d 2 1 1 25 2 1 1 1 " + "%d 0 0 0 0" % M25,
    "nm_Z_then_C": "K %(id)d 1 %(pos)d %(right)d 2 0 0 25 2 0 0 1 " + "%d 0 0 0 0" % M25,
    "xs_minus_then_plus": "K %(id)d 1 %(pos)d %(right325)d 2 1 1 25 6 1 1 3 " + SPL_CIG,
    "xs_plus_then_minus": "K %(id)d 1 %(pos)d %(right325)d 2 1 1 25 2 1 1 3 " + SPL_CIG,
    "xs_Z_then_minus": "K %(id)d 1 %(pos)d %(right325)d 2 1 1 25 2 1 1 3 " + SPL_CIG,
    # sscanf("%u:%u:%u") stops at the first field without a digit: seg_num and num_segs stay 0, 0 + 1 != 0, `end` is false
    "name_7|:1:2": "K 7 1 %(pos)d %(right)d 0 1 1 25 0 1 1 1 " + "%d 0 0 0 0" % M25,
    "name_7|0::1": "K 7 1 %(pos)d %(right)d 0 1 1 25 0 1 1 1 " + "%d 0 0 0 0" % M25,
    # get_hit_from_buf never looks at BAM_FUNMAP: a record with a target is a hit
    "flag_4_with_a_target": "K %(id)d 1 %(pos)d %(right)d 2 1 1 25 2 1 1 1 " + "%d 0 0 0 0" % M25,
}


def test_findings_are_pinned_to_the_references_answer(exe, parser_file):
    recs, w = parser_file
    rc, lines, err = hitdump(exe, w.path)
    assert rc == 0, err
    seen = set()
    for (label, r), got in zip(recs, lines):
        if label not in FINDINGS:
            continue
        seen.add(label)
        pos = int.from_bytes(r[8:12], "little")
        name = r[36:36 + r[12] - 1]
        rid = int(name) if name.isdigit() else 7
        want = FINDINGS[label] % dict(id=rid, pos=pos, right=pos + 25, right325=pos + 325)
        assert dump_line(ir.hit_from_record(r[4:], ic.TID2REF, ic.MAX_INTRON)) == want, label
        assert got == want, label
    assert seen == set(FINDINGS)


# every branch of the restatement the parser table has to reach
LABELS = """antisense char_of_non_A_type contig_unknown five_counted_ops flag_unmapped_with_a_target int_of_non_integer_type
intron_above_max intron_at_max kept mate_none mate_on_another_target mate_on_the_same_target name_end name_fields_0 name_fields_1
name_fields_2 name_fields_3 name_last_pipe name_no_colon name_no_pipe name_not_end nm_cut_to_a_byte nm_missing nm_wrap op_10 op_11
op_12 op_13 op_14 op_15 op_9 op_D op_EQ op_H op_I op_M op_N op_P op_S op_X op_zero_length read_len_above_255 sense skip_A
skip_B_C_empty skip_B_C_some skip_B_I_empty skip_B_I_some skip_B_S_empty skip_B_S_some skip_B_c_empty skip_B_c_some skip_B_f_empty
skip_B_f_some skip_B_i_empty skip_B_i_some skip_B_s_empty skip_B_s_some skip_C skip_H skip_S skip_Z skip_c skip_d_walked_into
skip_f_walked_into skip_s skip_unknown_type tag_C tag_I tag_I_neg tag_S tag_c tag_c_neg tag_i tag_i_neg tag_s tag_s_neg tid_negative
tid_outside_table xs_minus xs_minus_unspliced xs_missing xs_other""".split()
# drop reason -> (a case dropped for it, its neighbour that is kept)
DROPS = {"tid_negative": ("tid_minus_1", "tid_second_contig"), "op_zero_length": ("op_zero_length", "op_I"),
         "op_without_an_arm": ("op_9", "op_P"), "intron_above_max": ("n_above_max", "n_at_max"),
         "mate_on_another_target": ("mtid_other", "mtid_same"), "tid_outside_table": ("tid_at_n_tid", "tid_second_contig"),
         "contig_unknown": ("tid_unknown_contig", "tid_second_contig")}


def test_the_parser_table_reaches_every_branch():
    """The labels say which arm of bam_aux2i read NM and with which sign.  What the arm's SIGNEDNESS is cannot be seen in any field of a
    hit: num_mismatches is an unsigned char, and a value's low byte is the same read signed or unsigned (a parser that read `s` as
    `S` passes every case here, and rightly).  The widths can: nm_256_s against nm_256_i, nm_65535_S, nm_-129_s."""
    ir.TAKEN.clear()
    status = {}
    for label, r in ic.parser_records():
        assert label not in status, "case labels are unique"
        status[label] = ir.hit_from_record(r[4:], ic.TID2REF, ic.MAX_INTRON)
    missing = sorted(set(LABELS) - ir.TAKEN)
    assert not missing, "branches no case reaches: %s" % missing
    reasons = {h[2] for h in status.values() if h[0] == "drop"}
    assert reasons == set(DROPS)
    for reason, (dropped, kept) in DROPS.items():
        assert status[dropped][0] == "drop" and status[dropped][2] == reason, dropped
        assert status[kept][0] == "keep", kept
    assert not [l for l, h in status.items() if h[0] == "error"], "the loud failures have files of their own"
    # each integer case exists once per type that holds its value
    for v in (255, 256, 65535, -1, -129):
        assert [l for l in status if l.startswith("nm_%d_" % v)] == ["nm_%d_%s" % (v, t) for t in ic.int_types_for(v)]


def test_layout_and_merge_maps_read_like_the_host_parser(exe, tmp_path):
    lay, mer = ic.layout_table(str(tmp_path)), ic.merge_table(str(tmp_path))
    for w in [lay.hits] + mer.segs + [mer.mate_full, mer.mate_last]:
        rc, lines, err = hitdump(exe, w.path)
        assert rc == 0, err
        assert lines == [dump_line(ir.hit_from_record(r, ic.TID2REF, ic.MAX_INTRON)) for r in w.records_from(0)], w.path


HOST_SAYS = {"xf_tag": "fusion (XF)", "six_counted_ops": "CIGAR operations", "header_does_not_fit_block_size": "malformed BAM record",
             "fixed_size_tag_cut_off": "malformed BAM record", "double_tag_cut_off": "malformed BAM record",
             "array_tag_count_past_the_record": "malformed BAM record", "array_tag_count_wraps_32_bits": "malformed BAM record"}


def test_loud_failures_end_the_host_reader(exe, tmp_path):
    for label, rec, _code, _piece in ic.loud_cases():
        w = ic.write_bam(str(tmp_path / (label + ".bam")), ic.loud_members(rec))
        rc, lines, err = hitdump(exe, w.path)
        assert rc != 0 and HOST_SAYS[label] in err, (label, rc, err)
        assert lines == ["K 19 1 500 525 2 1 1 25 2 1 1 1 %d 0 0 0 0" % M25], label       # the record before it was read, nothing after it
        want = ir.hit_from_record(rec[4:], ic.TID2REF, ic.MAX_INTRON)
        if label in ("xf_tag", "six_counted_ops"):
            assert want[0] == "error" and want[2] == label


def test_reads_read_like_the_host_reader(exe, tmp_path):
    """ReadStream on the planted reads files: QC-fail records are read past, the first remaining record of an id is the read"""
    for tab, ids in ((ic.merge_table(str(tmp_path)), ic.MERGE_READS), (ic.reads_table(str(tmp_path)), None)):
        want = ir.reads_of(tab.reads.records_from(0))
        ids = sorted(want) if ids is None else ids
        out = subprocess.run([exe, "reads", tab.reads.path] + ["%d" % i for i in ids], capture_output=True).stdout.split(b"\n")
        for i, line in zip(ids, out):
            seq, qual = want[i]
            assert line == b"%d %s %s" % (i, seq.encode(), qual), i
    assert "read_qc_fail_skipped" in ir.TAKEN


@pytest.mark.parametrize("name", CASES)
def test_golden_maps_read_like_the_sam_model(name, tmp_path):
    d = os.path.join(GOLD, name)
    maps = sorted(f for f in os.listdir(d) if f.endswith(".sam") and ("_seg" in f or "_map" in f) and "to_spliced" not in f and not f.startswith("expected"))
    assert maps
    for f in maps:
        sam = os.path.join(d, f)
        names, _ = parse_header(sam)
        bam = str(tmp_path / (f[:-4] + ".bam"))
        write_bam_from_sam(sam, bam)
        data = gzip.open(bam, "rb").read()
        hdr = len(ic.bam_header([(n, 0) for n in names], "".join(l for l in open(sam) if l.startswith("@"))))
        got = ir.kept_hits(ir.records_of(data, hdr), list(range(1, len(names) + 1)), 500000)
        want = [tuple(h) for h in parse_sam_hits(sam, {n: i + 1 for i, n in enumerate(names)})]
        assert [tuple(h) for h in got] == want, f
