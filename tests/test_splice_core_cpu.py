"""CPU: the spliced hit factory of the device-side ingest (tophat_amd/csrc/thj_splice_core.h, compiled for the CPU by
tests/splicesim) on the planted junction-db records of splice_cases.py, against the Python restatement of
SplicedBAMHitFactory::get_hit_from_buf / spliceCigar / getBAMmismatches (tophat_amd/samtext.py: parse_spliced_sam_hits) -- and the
executables' host factory (parse_spliced_hit, through the same program) against both.  Every label's outcome is asserted."""
import os
import subprocess

import pytest

import splice_cases as sc
from ingest_cases import MAX_INTRON
from locked_make import locked_make

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "splicesim", "splicesim")
REP_CIGAR, REP_FUSION = 2, 4


@pytest.fixture(scope="module")
def exe():
    locked_make(os.path.join(HERE, "splicesim"))
    return EXE


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("splice"))
    cs = sc.cases()
    sam, bam = sc.write_map(d, "planted", [c[3] for c in cs])
    quiet = [c for c in cs if c[1] in (sc.KEPT, sc.DROPPED)]
    qsam, qbam = sc.write_map(d, "planted_quiet", [c[3] for c in quiet])
    return cs, sam, bam, qbam


def run(exe, mode, bam):
    """-> (target lines, [(kept, id, report bits, fields)]) in file order"""
    out = subprocess.check_output([exe, mode, bam, str(MAX_INTRON), sc.KNOWN], stderr=subprocess.DEVNULL).decode().split("\n")
    tg = [tuple(int(x) for x in l.split()[1:]) for l in out if l.startswith("T ")]
    recs = []
    for l in out:
        if l[:2] in ("K ", "D "):
            f = l.split()
            recs.append((f[0] == "K", int(f[1]), int(f[2]), tuple(int(x) for x in f[3:])))
    return tg, recs


def test_target_table(exe, planted):
    _cs, _sam, bam, _q = planted
    tg, _ = run(exe, "core", bam)
    by_name = {sc.TARGETS[t[0]]: t[1:] for t in tg}
    assert len(tg) == len(sc.TARGETS)
    # (ref_id, ref_id2, left, lsp, second, type, strand); types junction 0, del 1, ins 2, fus 3, invalid 4; strands fwd 0, rev 1, ff 2, other 6
    assert by_name[sc.J_FWD] == (1, 0, 975, 999, 1500, 0, 0)
    assert by_name[sc.J_REV] == (2, 0, 1975, 1999, 2300, 0, 1)
    assert by_name[sc.J_PIPE] == (3, 0, 975, 999, 1500, 0, 0)
    assert by_name[sc.DEL] == (1, 0, 2975, 2999, 3004, 1, 0)
    assert by_name[sc.INS6] == (2, 0, 6975, 6999, 6, 2, 1)
    assert by_name[sc.INS_XYZ] == (1, 0, 4975, 4999, 3, 2, 6)
    assert by_name[sc.FUS] == (1, 2, 975, 999, 2000, 3, 2)
    assert by_name[sc.T_UNKNOWN][0] == 0 and by_name[sc.T_UNKNOWN][5] == 0          # unknown contig: a valid target, contig 0
    for bad in (sc.T_FIVE, sc.T_ONE_PART, sc.T_STRAND):
        assert by_name[bad][5] == 4, bad


def test_every_planted_record(exe, planted):
    cs, sam, bam, _q = planted
    _, got = run(exe, "core", bam)
    assert [g[1] for g in got] == [c[2] for c in cs], "one output line per record, in file order"
    want = {h[0]: h for h in sc.restated(sam, 0, sc.END_ID)}                       # (the shard's id window is the caller's: thj_k_parse, the stream)
    seen = set()
    for (label, outcome, rid, _f), (kept, _id, rep, fields) in zip(cs, got):
        seen.add(label)
        if outcome == sc.SIX_OPS:
            assert not kept and rep == REP_CIGAR, label
            assert len(want[rid][9]) == 7, "the restatement splices it into seven operations"
        elif outcome == sc.FALLBACK:
            assert not kept and rep == REP_FUSION, label
            assert rid in want, "the restatement (and the host factory) keep a record on a fusion contig"
        elif outcome == sc.DROPPED and label != "id_below_begin":
            assert not kept and rep == 0 and rid not in want, label
        else:
            assert kept and rep == 0, label
            assert rid in want, label
            assert fields == sc.hit_row(want[rid]), "%s: the core gives %r, the restatement %r" % (label, fields, sc.hit_row(want[rid]))
            if label in sc.CIGARS:
                assert list(want[rid][9]) == sc.CIGARS[label], "%s: %r" % (label, want[rid][9])
            if label in sc.MISMATCHES:
                assert (fields[3], fields[4]) == sc.MISMATCHES[label], "%s: mismatches, edit distance %r" % (label, fields[3:5])
    assert seen == {c[0] for c in cs} and len(seen) == len(cs)
    assert set(sc.CIGARS) <= seen and set(sc.MISMATCHES) <= seen
    # flags: THJ_HIT_END for the last segment, THJ_HIT_ANTISENSE_SPLICE on a rev target, THJ_HIT_ANTISENSE from the record's flag
    by_label = {c[0]: g for c, g in zip(cs, got)}
    assert by_label["junc_last_segment"][3][2] & 2 and not by_label["junc_not_the_last_segment"][3][2] & 2
    assert by_label["junc_rev_inside_M"][3][2] & 4 and not by_label["junc_fwd_inside_M"][3][2] & 4
    assert by_label["junc_fwd_inside_M_antisense"][3][2] & 1 and by_label["ins_six_bases"][3][2] & 4


def test_host_factory_agrees(exe, planted):
    """parse_spliced_hit, which tokenises the target's name through the same function the target table is made with, on the records
    that do not end the run"""
    cs, _sam, _bam, qbam = planted
    quiet = [c for c in cs if c[1] in (sc.KEPT, sc.DROPPED)]
    _, core = run(exe, "core", qbam)
    _, hst = run(exe, "host", qbam)
    assert len(core) == len(hst) == len(quiet)
    for c, a, b in zip(quiet, core, hst):
        assert a == b, "%s: the core gives %r, the host factory %r" % (c[0], a, b)
