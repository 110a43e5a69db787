"""CPU: insertions.bed and deletions.bed of tophat_reports' consensus pass.  The Python restatement of the reference
(tests/indelbed_ref.py) is pinned by the recorded outputs of the reference's nine regression cases and, for the junction filter
that decides which records count, by the C oracle; the walker header the device kernels run (tophat_amd/csrc/thj_jb_walk.h) is
compiled for the CPU (tests/indelsim) and compared with the restatement's walkers."""
import os
import subprocess

import pytest

import indelbed_cases as ic
import indelbed_ref as ir
import orc
import ref_regression as rr
from locked_make import locked_make

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("case", rr.CASES)
def test_restatement_gives_the_recorded_bed_files(case):
    recs = rr.recorded_alignment_records(case)
    js, ins, dels = ir.consensus(recs, ir.recorded_seqs(rr.GOLD, case))
    gold = lambda f: open(os.path.join(rr.GOLD, case, f)).read()
    assert ir.insertions_bed(ins, ["fake"]) == gold("insertions.bed")
    assert ir.deletions_bed(dels, ["fake"]) == gold("deletions.bed")
    assert ir.junctions_bed(js, ["fake"]) == gold("junctions.bed")


def test_recorded_cases_hold_indels():
    """what the nine cases pin: five of them have an insertion, four a deletion (test_IndelWithErrors three)"""
    n = {c: (open(os.path.join(rr.GOLD, c, "insertions.bed")).read().count("\n") - 1, open(os.path.join(rr.GOLD, c, "deletions.bed")).read().count("\n") - 1)
         for c in rr.CASES}
    assert n["test_IndelWithErrors"] == (1, 3) and n["test_Indel_1"] == (1, 0) and n["test_SimpleIndel"] == (1, 1)
    assert sum(1 for v in n.values() if v == (0, 0)) == 4


def _oracle_rows(recs):
    return ir.junc_rows(orc.junction_consensus(orc.jrecs_from_tuples(recs)))


@pytest.mark.parametrize("case", rr.CASES)
def test_junction_filter_equals_the_oracle_on_recorded_cases(case):
    recs = rr.recorded_alignment_records(case)
    assert ir.consensus(recs)[0] == _oracle_rows(recs)


def test_junction_filter_equals_the_oracle_on_hand_made_lists():
    lists = ic.filter_cases() + [ic.fusion_cases() * 3, ic.fusion_indel_cases() * 2, ic.crowd()]
    for recs in lists:
        assert ir.consensus(recs)[0] == _oracle_rows(recs), recs[:3]
    assert len(ir.consensus(lists[-1])[0]) > 20 and len(ir.consensus(lists[-4])[0]) > 50


def test_walker_header_equals_the_restatement():
    """thj_jb_walk.h, compiled for the CPU, prints every occurrence of the hand-made records; the restatement's walkers say the same"""
    locked_make(os.path.join(HERE, "indelsim"))
    recs = ic.fusion_indel_cases() + ic.crowd()[:400] + [r for c in ic.filter_cases()[:11] for r in c]
    recs += [(1, 0, False, [(ic.I, 2), (ic.M, 20), (ic.D, 1), (ic.M, 3)]), (1, 5, False, [(ic.m, 10), (ic.d, 2), (ic.m, 4)])]      # at the contig's start: unsigned wrap
    got = subprocess.run([os.path.join(HERE, "indelsim", "indelsim")], input=ic.sim_input(recs), capture_output=True, text=True, check=True).stdout
    want = ic.sim_expected(recs, ir)
    assert got == want
    assert want.count("\nD ") > 100 and want.count("\nI ") > 100 and want.count("\nJ ") > 100


def test_hand_made_properties():
    M, I, D = ic.M, ic.I, ic.D
    a = (1, 100, False, [(M, 20), (I, 2), (M, 20)])
    # (a) same place and length, other letters: one entry, the first record's letters
    _, ins, _ = ir.consensus([a, a], ["A" * 20 + "CG" + "A" * 20, "A" * 20 + "TT" + "A" * 20])
    assert [(x[2], x[5]) for x in ins] == [("CG", 2)]
    # (b) lengths 2 and 3 at one place: two entries, the shorter first
    b = (1, 100, False, [(M, 20), (I, 3), (M, 20)])
    _, ins, _ = ir.consensus([b, a], ["A" * 20 + "GGG" + "A" * 20, "A" * 20 + "TT" + "A" * 20])
    assert [x[2] for x in ins] == ["TT", "GGG"]
    # (c) the cap is the printer's, and only the insertion printer's
    _, ins, dels = ir.consensus([a] * 1001 + [(1, 300, False, [(M, 20), (D, 2), (M, 20)])] * 1001, ["A" * 42] * 1001 + ["A" * 40] * 1001)
    assert ins[0][5] == 1001 and ir.insertions_bed(ins, ["x"]).endswith("\t1000\n") and ir.deletions_bed(dels, ["x"]).endswith("\t1001\n")
    # (d) a deletion on a record whose junction fails min_anchor does not count
    dj = (1, 100, False, [(M, 20), (D, 2), (M, 20), (ic.N, 200), (M, 5)])
    dc = (1, 100, False, [(M, 20), (D, 2), (M, 30)])
    assert ir.consensus([dj])[2] == [] and [x[5] for x in ir.consensus([dj, dc])[2]] == [1]
    # the clipped record of the fusion list: letters from in front of where the aligner put them
    r = ic.fusion_indel_cases()[-2]
    assert ir.rec_inss(r, "".join(chr(65 + k % 26) for k in range(ic.seq_len(r))))[0][2] == "UVW"
