"""CPU: the fusion branch of the spliced hit factory of the device-side ingest (tophat_amd/csrc/thj_splice_core.h:
splc::spliced_hit_as<true>, compiled for the CPU by tests/fusplicesim) on the planted fusion-contig records of fusplice_cases.py,
against the Python restatement of SplicedBAMHitFactory::get_hit_from_buf / spliceCigar (tophat_amd/samtext.py:
parse_spliced_sam_hits) and against the executables' host factory (parse_spliced_hit, through the same program).  Every label's
outcome is asserted; the old splc::spliced_hit (tests/splicesim, unchanged) still reports the same records as REP_FUSION."""
import os
import subprocess

import pytest

import fusplice_cases as fc
from ingest_cases import MAX_INTRON
from locked_make import locked_make
from tophat_amd import host

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "fusplicesim", "fusplicesim")
OLD_EXE = os.path.join(HERE, "splicesim", "splicesim")
REP_CIGAR, REP_FUSION = 2, 4


@pytest.fixture(scope="module")
def exe():
    locked_make(os.path.join(HERE, "fusplicesim"))
    return EXE


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("fusplice"))
    cs = fc.cases()
    sam, bam = fc.write_map(d, "planted", [c[3] for c in cs], fc.TARGETS)
    quiet = [c for c in cs if c[1] != fc.LOUD]
    _qsam, qbam = fc.write_map(d, "planted_quiet", [c[3] for c in quiet], fc.TARGETS)
    return cs, sam, bam, qbam


def run(exe, mode, bam):
    """-> (target lines, [(kept, id, report bits, fields)]) in file order"""
    out = subprocess.check_output([exe, mode, bam, str(MAX_INTRON), fc.KNOWN], stderr=subprocess.DEVNULL).decode().split("\n")
    tg = [tuple(int(x) for x in l.split()[1:]) for l in out if l.startswith("T ")]
    recs = []
    for l in out:
        if l[:2] in ("K ", "D "):
            f = l.split()
            recs.append((f[0] == "K", int(f[1]), int(f[2]), tuple(int(x) for x in f[3:])))
    return tg, recs


def pack(ops):
    return tuple((o << 28) | n for o, n in ops)


def test_symbol_is_part_of_the_abi():
    assert "thj_span_juncdb_fusion_contigs" in host.ABI_SYMBOLS
    assert "int thj_span_juncdb_fusion_contigs(thj_ctx* ctx, int32_t on);" in open(os.path.join(os.path.dirname(HERE), "include", "thj.h")).read()


def test_target_table(exe, planted):
    _cs, _sam, bam, _q = planted
    tg, _ = run(exe, "core", bam)
    by_name = {fc.TARGETS[t[0]]: t[1:] for t in tg}
    assert len(tg) == len(fc.TARGETS)
    # (ref_id, ref_id2, left, lsp, second, type, strand); type fus 3, invalid 4; strands ff 2, fr 3, rf 4, rr 5
    assert by_name[fc.FF] == (1, 2, 975, 999, 2000, 3, 2)
    assert by_name[fc.FR] == (1, 2, 975, 999, 2024, 3, 3)
    assert by_name[fc.RF] == (1, 2, 1024, 1000, 2000, 3, 4)
    assert by_name[fc.RR] == (1, 2, 1024, 1000, 2024, 3, 5)
    assert by_name[fc.U2][:2] == (1, 0) and by_name[fc.U2][5] == 3
    assert by_name[fc.U1][:2] == (0, 2) and by_name[fc.U1][5] == 3
    assert by_name[fc.ONE_CONTIG][5] == 4
    assert by_name[fc.J_FWD] == (1, 0, 975, 999, 1500, 0, 0)


def test_expectations_written_out_agree():
    for label, want in fc.BY_HAND.items():
        assert fc.EXPECTED[label] == want, label


def test_every_planted_record(exe, planted):
    cs, sam, bam, _q = planted
    _, got = run(exe, "core", bam)
    assert [g[1] for g in got] == [c[2] for c in cs], "one output line per record, in file order"
    raw = fc.restated_raw(sam)
    want = {h[0]: h for h in fc.restated(sam, 0, fc.END_ID)}
    seen, dirs_kept = set(), set()
    for (label, outcome, rid, f), (kept, _id, rep, fields) in zip(cs, got):
        seen.add(label)
        if outcome == fc.LOUD:
            assert not kept and rep == REP_CIGAR, label
            n_ops = fc.LOUD_N_OPS[label if label in fc.LOUD_N_OPS else label.split("_", 2)[2]]
            assert len(raw[rid][9]) == n_ops, "%s: the restatement splices it into %r" % (label, raw[rid][9])
            if label in fc.LOUD_OPS:
                assert list(raw[rid][9]) == fc.LOUD_OPS[label], label
        elif outcome == fc.DROPPED:
            assert not kept and rep == 0 and rid not in want, label
        else:
            assert kept and rep == 0, label
            assert rid in want, label
            assert fields == fc.hit_row(want[rid]), "%s: the core gives %r, the restatement %r" % (label, fields, fc.hit_row(want[rid]))
            left, ops, flags, mm = fc.EXPECTED[label]
            fused = bool(flags & fc.FUSED)
            gap = sum(n for o, n in ops if 3 <= o <= 6)
            assert list(want[rid][9]) == ops, "%s: %r" % (label, want[rid][9])
            assert fields == (1, left, flags, mm, mm + gap, len(ops)) + pack(ops) + (0,) * (4 - len(ops)) + ((2,) if fused else (0,)), label
            assert not flags & 4 or not fused, "never THJ_HIT_ANTISENSE_SPLICE on a fused hit"
            if fused:
                dirs_kept.add(label.split("_")[1])
    assert seen == {c[0] for c in cs} and len(seen) == len(cs)
    assert {c[0] for c in cs if c[1] == fc.KEPT} == set(fc.EXPECTED)
    assert set(fc.LOUD_OPS) <= seen and dirs_kept == {"ff", "fr", "rf", "rr"}


def test_host_factory_agrees(exe, planted):
    """parse_spliced_hit on the records that do not end the run: field by field what the core gives"""
    cs, _sam, _bam, qbam = planted
    quiet = [c for c in cs if c[1] != fc.LOUD]
    _, core = run(exe, "core", qbam)
    _, hst = run(exe, "host", qbam)
    assert len(core) == len(hst) == len(quiet)
    for c, a, b in zip(quiet, core, hst):
        assert a == b, "%s: the core gives %r, the host factory %r" % (c[0], a, b)
    assert sum(1 for a in core if a[0]) == len(fc.EXPECTED)


def test_host_factory_ends_the_run_at_a_fifth_operation(exe, planted, tmp_path):
    """... and on the loud ones it dies with the message the device path's THJ_EINVAL stands for"""
    cs = planted[0]
    for label in ("fus_fr_I_after_break", "unknown_first_contig_five_ops"):
        _sam, bam = fc.write_map(str(tmp_path), label, [c[3] for c in cs if c[0] == label], fc.TARGETS)
        r = subprocess.run([exe, "host", bam, str(MAX_INTRON), fc.KNOWN], capture_output=True, text=True)
        assert r.returncode != 0 and "4 on a fusion contig" in r.stderr, label
    _sam, bam = fc.write_map(str(tmp_path), "quiet_u2", [c[3] for c in cs if c[0] == "unknown_second_contig_five_ops"], fc.TARGETS)
    r = subprocess.run([exe, "host", bam, str(MAX_INTRON), fc.KNOWN], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("D ")


def test_old_entry_point_still_reports_fusion(planted):
    """splc::spliced_hit keeps its answer: a record on a fusion contig is REP_FUSION and not kept, whatever would become of it"""
    locked_make(os.path.join(HERE, "splicesim"))
    cs, _sam, bam, _q = planted
    _, got = run(OLD_EXE, "core", bam)
    assert len(got) == len(cs)
    for (label, _outcome, _rid, f), (kept, _id, rep, _fields) in zip(cs, got):
        if f[2] in (fc.FF, fc.FR, fc.RF, fc.RR, fc.U1, fc.U2):
            assert not kept and rep == REP_FUSION, label
        elif label == "junc_plain":
            assert kept and rep == 0
        else:
            assert not kept and rep == 0, label
