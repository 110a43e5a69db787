"""CPU: the record core of thj_juncbed_add_bam (tophat_amd/csrc/thj_reported_core.h, compiled for the CPU by tests/reportedsim) on the
planted records of reported_cases.py, line by line against the Python restatement of thj_junctions' host reader (reported_ref.py), in
all four combinations of "indels collected" and "fusions collected"; the outcomes and a good part of the records are also written out
by hand (reported_cases.CASES / BY_HAND)."""
import os
import subprocess

import pytest

import reported_cases as rc
import reported_ref as rr
from ingest_cases import MAX_INTRON
from locked_make import locked_make
from tophat_amd import host

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def exes():
    d = os.path.join(HERE, "reportedsim")
    locked_make(d)
    return os.path.join(d, "reportedsim"), os.path.join(d, "reportedsim_san")


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("reported"))
    return rc.write(os.path.join(d, "planted.bam"), rc.CASES, per_member=40)


def run(exe, bam, mode):
    ind, fus = rc.MODES[mode]
    r = subprocess.run([exe, bam, str(MAX_INTRON), str(ind), str(fus), ",".join(rc.KNOWN)], capture_output=True, text=True)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-2000:])
    return [l.split() for l in r.stdout.split("\n") if l]


def restated(mode):
    """per case: ("K", Kept) | ("D", None) | ("L", what)"""
    ind, fus = rc.MODES[mode]
    out = []
    for _label, _o, rec in rc.CASES:
        try:
            k = rr.parse_record(rec[4:], rc.TID2REF, rc.name_id, MAX_INTRON, ind, fus)
            out.append(("K", k) if k is not None else ("D", None))
        except rr.Loud as e:
            out.append(("L", e.what))
    return out


def test_symbol_is_part_of_the_abi():
    assert "thj_juncbed_add_bam" in host.ABI_SYMBOLS
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "thj.h")).read()
    assert "int thj_juncbed_add_bam(thj_ctx* ctx, const thj_bam_piece* piece, int32_t max_report_intron, int32_t more_follows, int64_t* n_records," in hdr


@pytest.mark.parametrize("mode", range(4))
def test_restatement_gives_the_outcomes_written_out_by_hand(mode):
    ind, _fus = rc.MODES[mode]
    for (label, outcomes, _rec), (kind, v) in zip(rc.CASES, restated(mode)):
        assert kind == outcomes[mode], "%s with %r: %s %r" % (label, rc.MODES[mode], kind, v)
        if kind == "L":
            assert v == rc.LOUD_WHAT[label], label
        if kind == "K" and label in rc.BY_HAND:
            ref, left, flags, ed, ops, ref2, letters = rc.BY_HAND[label]
            cig = [(o << 28) | n for o, n in ops] + [0] * (16 - len(ops))
            if ref2:
                cig[15] = ref2
            assert v.row() == (ref, left, flags, ed, len(ops)) + tuple(cig), label
            assert v.letters == (letters if ind else ""), label
    assert set(rc.BY_HAND) <= set(rc.LABELS) and set(rc.LOUD_WHAT) == {c[0] for c in rc.CASES if "L" in c[1]}
    # every arm is reached: each outcome in each mode, every way to end the run
    assert {c[1][mode] for c in rc.CASES} == {"K", "D", "L"}
    assert set(rc.LOUD_WHAT.values()) == set(rr.REP_BITS)


@pytest.mark.parametrize("mode", range(4))
def test_core_against_the_restatement(exes, planted, mode):
    ind, fus = rc.MODES[mode]
    got = run(exes[0], planted.path, mode)
    want = restated(mode)
    assert len(got) == len(want) == len(rc.CASES), "one output line per record, in file order"
    prev_key = None
    for (label, _o, _rec), g, (kind, v) in zip(rc.CASES, got, want):
        if kind == "D":
            assert g == ["D", "0"], label
        elif kind == "L":
            assert g[0] == "D" and int(g[1]) & rr.REP_BITS[v], "%s: report bits %s, the host reader ends the run with %s" % (label, g[1], v)
        else:
            assert g[0] == "K", label
            assert tuple(int(x) for x in g[1:22]) == v.row(), "%s: the core gives %r, the restatement %r" % (label, g[1:22], v.row())
            assert g[22] == (v.letters or "-"), label
            head = 1 if prev_key is None or prev_key != v.key else 0
            assert int(g[23]) == head, label
            if fus and label in rc.READ_RUN_HEADS:
                assert head == rc.READ_RUN_HEADS[label], label
            prev_key = v.key


def test_read_numbers_of_the_restatement():
    """parse_all numbers the runs of kept records as the host reader does after its shares are joined"""
    recs = [c[2][4:] for c in rc.CASES if c[0].startswith("read_")]
    kept, idx = rr.parse_all(recs, rc.TID2REF, rc.name_id, MAX_INTRON, 0, 1)
    assert len(kept) == 7 and idx == [0, 0, 0, 1, 2, 2, 2]


@pytest.mark.parametrize("mode", (1, 3))
def test_planted_records_under_the_sanitizers(exes, planted, mode):
    """the sanitizer build as a process of its own: a read past a record's end, or undefined arithmetic, ends it with an error"""
    assert run(exes[1], planted.path, mode) == run(exes[0], planted.path, mode)


def test_name_lookup_by_bisection(exes, tmp_path):
    """many contigs, the fusion's two among them at both ends and in the middle of the sorted order"""
    from ingest_cases import M, cw, record, write_bam
    names = ["c%03d" % (k * 7 % 101) for k in range(101)] + ["a", "zz", "c05", "c0500"]
    recs, want = [], []
    for first, second in (("a", "zz"), ("zz", "a"), ("c050", "c05"), ("c05", "c0500"), ("c000", "c100"), ("c0", "a"), ("a", "c1000")):
        recs.append(record("n", cigar=[cw(M, 25)], seq=rc.seq(25), aux=rc.fus("20M5000F10M", contigs="%s-%s" % (first, second))))
        want.append((names.index(first) + 1, names.index(second) + 1) if first in names and second in names else None)
    w = write_bam(str(tmp_path / "names.bam"), [(recs, 6)], targets=(("a", 100000),))
    r = subprocess.run([exes[0], w.path, str(MAX_INTRON), "0", "1", ",".join(names)], capture_output=True, text=True)
    assert r.returncode == 0
    got = [l.split() for l in r.stdout.split("\n") if l]
    assert [(int(g[1]), int(g[6 + 15])) if g[0] == "K" else None for g in got] == want
    assert want.count(None) == 2
