"""CPU: the junction consensus with annotated junctions (--gtf-juncs) and the read filter.  (a) the restatement (jbknown_ref.py) with
neither switched on is pinned by the oracle and by indelbed_ref; (b) (c) its answers on the planted cases are the ones written out by
hand in jbknown_cases.py; (d) the decisions of tophat_amd/csrc/thj_jbknown_core.h, compiled for the CPU by tests/jbknownsim, are the
restatement's on the planted cases and on a crowd with 30 % of its junctions annotated; (e) the --gtf-juncs line reader."""
import os
import subprocess

import numpy as np
import pytest

import indelbed_ref as ir
import jbknown_cases as jc
import jbknown_ref as jr
import orc
import ref_regression as rr
from locked_make import locked_make
from tophat_amd import host

HERE = os.path.dirname(os.path.abspath(__file__))
LENS = [len(s) for s in jc.GENOME]


def orc_rows(recs, min_anchor=8):
    return [tuple(int(x) for x in r)[:7] for r in orc.junction_consensus(orc.jrecs_from_tuples(recs), min_anchor).tolist()]


# ---------------------------------------------------------------- (a)

def _test_filters_case_lists():
    """every case list of test_juncbed_cpu.test_filters"""
    rec = jc.rec
    M, N = jc.M, jc.N
    long1 = [rec(100, 20, 60000, 20)]
    return [
        [rec(100, 20, 500, 7)], [rec(100, 20, 500, 7), rec(90, 30, 500, 12)],
        long1, long1 * 2, [rec(100, 20, 60000, 12)] * 2,
        [rec(100, 20, 500, 20, anti=False)] * 3 + [rec(103, 20, 497, 20, anti=True)],
        [(1, 100, False, [(M, 20), (N, 300), (M, 30), (N, 400), (M, 25)])],
        [(1, 100, False, [(M, 20), (N, 300), (M, 30), (N, 400), (M, 5)])],
        [(2, 1000, True, [(M, 10), (5, 3), (M, 10), (N, 100), (M, 15), (3, 2), (M, 9)])],
    ]


@pytest.mark.parametrize("k", range(9))
def test_plain_restatement_equals_the_oracle_on_the_filter_cases(k):
    recs = _test_filters_case_lists()[k]
    assert jr.consensus(recs)[0] == orc_rows(recs)
    assert jr.consensus(recs) == ir.consensus(recs)


@pytest.mark.parametrize("min_anchor", (8, 12))
def test_plain_restatement_equals_the_oracle_on_the_crowd(min_anchor):
    recs = jc.crowd()
    got = jr.consensus(recs, min_anchor=min_anchor)
    assert got[0] == orc_rows(recs, min_anchor) and len(got[0]) > 50
    assert got == ir.consensus(recs, min_anchor=min_anchor)


@pytest.mark.parametrize("case", rr.CASES)
def test_plain_restatement_equals_the_oracle_on_the_recorded_cases(case):
    recs = rr.recorded_alignment_records(case)
    seqs = ir.recorded_seqs(rr.GOLD, case)
    got = jr.consensus(recs, seqs)
    assert got[0] == orc_rows(recs)
    assert got == ir.consensus(recs, seqs)


# ---------------------------------------------------------------- (b) (c)

@pytest.mark.parametrize("case", jc.KNOWN_CASES, ids=lambda c: c[0])
def test_annotated_junctions_by_hand(case):
    _label, anchor, recs, known, want_j, want_d = case
    j, _i, d = jr.consensus(recs, min_anchor=anchor, known=known)
    assert (j, d) == (want_j, want_d)


def test_the_by_hand_cases_differ_only_by_the_annotation():
    """each pair of cases over the same records: without the annotation the plain consensus, which the oracle gives too"""
    for _label, anchor, recs, _known, _j, _d in jc.KNOWN_CASES:
        assert jr.consensus(recs, min_anchor=anchor)[0] == orc_rows(recs, anchor)
    by = {c[0]: c for c in jc.KNOWN_CASES}
    assert by["short_anchor_unknown"][4] != by["short_anchor_known"][4] and by["deletion_without_annotation"][5] != by["deletion_with_annotation"][5]
    assert by["shadow_no_annotation"][4] == by["shadow_stronger_known"][4] != by["shadow_weaker_known"][4]


@pytest.mark.parametrize("case", jc.FILTER_CASES, ids=lambda c: c[0])
def test_read_filter_by_hand(case):
    _label, rec, nm, outcomes = case
    mism = jr.mismatches(nm, rec[3])
    for limits, (want_mm, want_gap, want_ed), want_drop in outcomes:
        assert (mism, jr.gap_length(rec[3]), jr.edit_dist(mism, rec[3])) == (want_mm, want_gap, want_ed)
        assert jr.dropped(mism, rec[3], limits) == want_drop
        rows = jr.consensus([rec], limits=limits, mism=[mism])[0]
        assert rows == ([] if want_drop else [(1, rec[1] + sum(ln for op, ln in rec[3][:-2] if op != jc.I) - 1, rec[1] + sum(ln for op, ln in rec[3][:-1] if op != jc.I), 0,
                                                 rec[3][-3][1], 20, 1)])


def test_a_dropped_record_is_gone_for_both_passes():
    """three good records accept a junction; a fourth over the limits neither supports it nor widens its extents, and its deletion
    is in no set"""
    good = [jc.rec(100, 20, 500, 20)] * 3
    bad = (1, 90, False, [(jc.M, 10), (jc.D, 1), (jc.M, 19), (jc.N, 500), (jc.M, 40)])
    recs, mism = good + [bad], [0, 0, 0, 3]
    assert jr.consensus(recs, mism=mism)[0] == [(1, 119, 620, 0, 20, 40, 4)] and len(jr.consensus(recs, mism=mism)[2]) == 1
    assert jr.consensus(recs, limits=(2, 2, 2), mism=mism) == ([(1, 119, 620, 0, 20, 20, 3)], [], [])


# ---------------------------------------------------------------- (d) the CPU sim

@pytest.fixture(scope="module")
def exes():
    d = os.path.join(HERE, "jbknownsim")
    locked_make(d)
    return os.path.join(d, "jbknownsim"), os.path.join(d, "jbknownsim_san")


def sim_text(cases):
    """cases: [(min_anchor, limits or None, annotated junctions, records, NMs)]"""
    out = []
    for anchor, limits, known, recs, nms in cases:
        out.append("A %d\nF %d %d %d %d\nC %s\n" % ((anchor, 1 if limits else 0) + tuple(limits or (0, 0, 0)) + (" ".join(str(x) for x in LENS),)))
        out += ["K %d %d %d %d\n" % tuple(k) for k in known]
        for r, nm in zip(recs, nms):
            out.append("R %d %d %d %d %d %d %s\n" % (r[0], r[1], 1 if r[2] else 0, -1 if nm is None else nm, r[4] if len(r) > 4 else 0, len(r[3]),
                                                      " ".join("%d %d" % c for c in r[3])))
        out.append("E\n")
    return "".join(out)


def run_sim(exe, cases, tmp_path):
    p = tmp_path / "cases.txt"
    p.write_text(sim_text(cases))
    r = subprocess.run([exe, "consensus", str(p)], capture_output=True, text=True)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-2000:])
    res, cur = [], {"R": [], "J": [], "O": []}
    for l in r.stdout.split("\n"):
        t = l.split()
        if not t:
            continue
        if t[0] == "E":
            res.append(cur)
            cur = {"R": [], "J": [], "O": []}
        else:
            cur[t[0]].append(tuple(int(x) for x in t[1:]))
    assert len(res) == len(cases)
    return res


def restated(case):
    anchor, limits, known, recs, nms = case
    mism = [jr.mismatches(nm, r[3]) for r, nm in zip(recs, nms)]
    R = [(m, jr.gap_length(r[3]), 1 if jr.dropped(m, r[3], limits) else 0) for r, m in zip(recs, mism)]
    live = [r for r, x in zip(recs, R) if not x[2]]
    ok_known = [k for k in known if 1 <= k[0] <= len(LENS) and 1 <= ((k[2] - k[1]) & 0xFFFFFFFF) < (1 << 29) and -1 <= ir._i32(k[1]) < LENS[k[0] - 1]]
    state, acc = jr.first_pass(live, anchor, ok_known)
    shown = {j[:4] for r in live for j in ir.rec_juncs(r)}
    J = [k + (state[k], 1 if acc[k] else 0) for k in sorted(shown)]
    return {"R": R, "J": J, "O": jr.consensus(recs, min_anchor=anchor, known=ok_known, limits=limits, mism=mism)[0]}


def planted_sim_cases():
    cases = [(anchor, None, known, recs, [0] * len(recs)) for _l, anchor, recs, known, _j, _d in jc.KNOWN_CASES]
    for _label, rec, nm, outcomes in jc.FILTER_CASES:
        cases += [(8, limits, [], [rec, jc.rec(300, 20, 100, 20)], [nm, 0]) for limits, _q, _d in outcomes]
    # entries that can equal no record's junction: contig 0 and 3, an empty and a negative span, a span of 2^29, a left end outside the contig
    odd = [(0, 119, 620, 0), (3, 119, 620, 0), (1, 620, 620, 0), (1, 620, 119, 0), (1, 119, 119 + (1 << 29), 0), (1, 30000, 30100, 0), (2, -2 & 0xFFFFFFFF, 50, 0)]
    cases.append((12, None, odd, [jc.rec(100, 20, 500, 9)], [0]))
    return cases


def test_sim_on_the_planted_cases(exes, tmp_path):
    cases = planted_sim_cases()
    got = run_sim(exes[0], cases, tmp_path)
    for c, g in zip(cases, got):
        assert g == restated(c), c
    # and the hand-written rows, straight from the core's decisions
    for (_l, _a, _r, _k, want_j, _d), g in zip(jc.KNOWN_CASES, got):
        assert g["O"] == want_j
    assert got[-1]["O"] == [] and all(j[4] == jr.REJECTED for j in got[-1]["J"])


@pytest.mark.parametrize("min_anchor", (8, 12))
def test_sim_on_the_crowd_with_a_third_annotated(exes, tmp_path, min_anchor):
    recs = jc.crowd()
    known = jc.crowd_known(recs)
    rng = np.random.default_rng(5)
    nms = [int(x) for x in rng.integers(0, 4, len(recs))]
    cases = [(min_anchor, None, known, recs, [0] * len(recs)), (min_anchor, (2, 2, 2), known, recs, nms), (min_anchor, None, [], recs, [0] * len(recs))]
    got = run_sim(exes[0], cases, tmp_path)
    for c, g in zip(cases, got):
        assert g == restated(c)
    with_known, plain = got[0], got[2]
    assert plain["O"] == orc_rows(recs, min_anchor) and with_known["O"] != plain["O"]
    before = {j[:4]: j[4:] for j in plain["J"]}
    marked = [j for j in with_known["J"] if j[4] == jr.KNOWN]
    assert any(before[j[:4]] == (jr.REJECTED, 0) for j in marked), "an annotated junction that accept_if_valid turns down"
    assert any(before[j[:4]] == (jr.VALID, 0) for j in marked), "an annotated junction that a neighbour knocks out"
    assert 0 < sum(r[2] for r in got[1]["R"]) < len(recs)


def test_sim_under_the_sanitizers(exes, tmp_path):
    """the sanitizer build as a process of its own"""
    recs = jc.crowd(n=400)
    cases = planted_sim_cases() + [(8, (2, 2, 2), jc.crowd_known(recs), recs, [k % 4 for k in range(len(recs))])]
    assert run_sim(exes[1], cases, tmp_path) == run_sim(exes[0], cases, tmp_path)


# ---------------------------------------------------------------- (e) the --gtf-juncs reader

GTF_LINES = ["chrA\t119\t620\t+", "chrB\t300\t900\t-", "chrZ\t5\t50\t+", "chrA\t119\t620\t+", "chrA\t700\t800\t-\tjunk behind the fourth field", "chrB\t 12x\t40\t+-"]
NAMES = ["chrA", "chrB"]


def run_gtf(exe, path):
    return subprocess.run([exe, "gtf", str(path), ",".join(NAMES)], capture_output=True, text=True)


def name_id(n):
    return NAMES.index(n) + 1 if n in NAMES else 0


@pytest.mark.parametrize("which", (0, 1))
def test_gtf_juncs_reader(exes, tmp_path, which):
    p = tmp_path / "gtf.juncs"
    text = "\n".join(GTF_LINES) + "\n"
    p.write_text(text)
    r = run_gtf(exes[which], p)
    assert r.returncode == 0 and "runtime error" not in r.stderr, r.stderr
    got = [tuple(int(x) for x in l.split()[1:]) for l in r.stdout.split("\n") if l.startswith("G ")]
    assert got == [(1, 119, 620, 0), (1, 700, 800, 1), (2, 12, 40, 0), (2, 300, 900, 1)] == jr.parse_gtf_juncs(text, name_id)
    assert "Loaded 4 GFF junctions from %s.\n" % p in r.stderr
    # the last line without its newline, and an empty file
    p.write_text(text[:-1])
    assert run_gtf(exes[which], p).stdout == r.stdout
    p.write_text("")
    r = run_gtf(exes[which], p)
    assert r.returncode == 0 and r.stdout == "" and "Loaded 0 GFF junctions" in r.stderr


def test_gtf_juncs_reader_ends_the_run_on_a_short_line(exes, tmp_path):
    p = tmp_path / "gtf.juncs"
    text = "chrA\t119\t620\t+\nchrA\t700\t800\nchrB\t300\t900\t-\n"
    p.write_text(text)
    r = run_gtf(exes[0], p)
    assert r.returncode == 1 and r.stdout == "" and r.stderr.endswith("Error: malformed splice coordinate record in %s\n:(null)\n" % p)
    assert jr.parse_gtf_juncs(text, name_id) is None


def test_gtf_juncs_file_that_cannot_be_opened(exes, tmp_path):
    r = run_gtf(exes[0], tmp_path / "absent")
    assert r.returncode == 0 and r.stdout == "" and "Loaded 0 GFF junctions from %s.\n" % (tmp_path / "absent") in r.stderr


def test_symbols_are_part_of_the_abi():
    assert {"thj_juncbed_known_junctions", "thj_juncbed_read_filter"} <= set(host.ABI_SYMBOLS)
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "thj.h")).read()
    assert "int thj_juncbed_known_junctions(thj_ctx* ctx, const thj_junction* juncs, int64_t n);" in hdr
    assert "int thj_juncbed_read_filter(thj_ctx* ctx, int32_t on, int32_t read_mismatches, int32_t read_gap_length, int32_t read_edit_dist);" in hdr
    assert "#define THJ_ABI_VERSION 2" in hdr
