"""CPU: the accepted-hits record rewrite (thj_junctions --accepted-hits-out).  (a) tophat_amd/csrc/thj_accepted_core.h, compiled for the
CPU by tests/acceptedsim, gives the records written out by hand in accepted_cases.py, and so does the restatement (accepted_ref.py, which
goes through the reference's text); (b) on a seeded crowd the core gives the restatement's records; (c) every loud case is loud in both;
(d) the sanitizer build, run as a program of its own, is clean on all of it; (e) the MAPQ table, the sort beyond 16 entries, the ABI."""
import os
import subprocess

import pytest

import accepted_cases as ac
import accepted_ref as ar
from locked_make import locked_make
from tophat_amd import host

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ac.cases()


@pytest.fixture(scope="module")
def exes():
    d = os.path.join(HERE, "acceptedsim")
    locked_make(d)
    return os.path.join(d, "acceptedsim"), os.path.join(d, "acceptedsim_san")


def sim_text(cases):
    out = []
    for c in cases:
        cfg = c["cfg"]
        out.append("C %d %s %d\n" % (cfg["library_type"], cfg["rg"] or "-", len(cfg["names"])))
        out += ["N %d %d %s\n" % (k + 1, cfg["header"].index(n) if n in cfg["header"] else -1, n) for k, n in enumerate(cfg["names"])]
        for draw, hits in c["reads"]:
            out.append("H %d %d\n" % (draw, len(hits)))
            out += ["R %d %d %s\n" % (ref, sc, rec.hex()) for ref, sc, rec in hits]
    return "".join(out)


def run_sim(exe, cases, tmp_path, mode="rewrite"):
    p = tmp_path / "cases.txt"
    p.write_text(cases if isinstance(cases, str) else sim_text(cases))
    r = subprocess.run([exe, mode, str(p)], capture_output=True, text=True)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-2000:])
    return r.stdout


def big_order(exe, tmp_path):
    """index_vector of a read beyond 16 entries: std::sort, run by acceptedsim"""
    def order(keys):
        return [int(x) for x in run_sim(exe, "".join("%d %d\n" % k for k in keys), tmp_path, "order").split()]
    return order


def restated(c, order=None):
    out = []
    for draw, hits in c["reads"]:
        out += ar.print_sam_for_single(hits, draw, c["cfg"], order)
    return out


def as_text(records):
    return "".join("O %s\n" % r.hex() for r in records)


# ---------------------------------------------------------------- (a)

@pytest.mark.parametrize("c", CASES, ids=[c["label"] for c in CASES])
def test_restatement_gives_the_hand_written_records(c):
    assert restated(c) == c["want"]


def test_core_gives_the_hand_written_records(exes, tmp_path):
    for c in CASES:
        assert run_sim(exes[0], [c], tmp_path) == as_text(c["want"]), c["label"]


def test_the_cases_show_what_they_are_about():
    by = {c["label"]: c for c in CASES}
    assert by["one"]["want"][0][13] == 50 and b"HI" not in by["one"]["want"][0] and b"CC" not in by["one"]["want"][0]
    assert [w[13] for w in by["two_contigs"]["want"]] == [3, 3] and b"CCZchrB\0" in by["two_contigs"]["want"][0] and b"CCZ=\0" in by["same_contig"]["want"][0]
    assert [by["n%d" % n]["want"][0][13] for n in (3, 4, 5)] == [1, 1, 0]
    assert sum(bool(int.from_bytes(w[18:20], "little") & 0x100) for w in by["two_contigs"]["want"]) == 1
    # an input with a wrong bin: every input carries 4680
    assert all(int.from_bytes(h[2][10:12], "little") == 4680 for c in CASES for _d, hits in c["reads"] for h in hits)
    assert ar.mapq(1) == 50 and [ar.mapq(n) for n in range(2, 8)] == [3, 1, 1, 0, 0, 0]


# ---------------------------------------------------------------- (b)

@pytest.fixture(scope="module")
def crowd():
    return ac.crowd()


def test_core_gives_the_restatement_on_the_crowd(exes, tmp_path, crowd):
    order = big_order(exes[0], tmp_path)
    want = "".join(as_text(restated(c, order)) for c in crowd)
    assert run_sim(exes[0], crowd, tmp_path) == want
    sizes = [len(h) for c in crowd for _d, h in c["reads"]]
    assert sizes.count(17) > 5 and sizes.count(16) > 5 and sizes.count(1) > 20 and want.count("O ") == sum(sizes)


def test_sort_beyond_16(exes, tmp_path):
    """up to 16 entries ties stand in hits order; beyond that the order is std::sort's, whatever it is -- and a permutation"""
    order = big_order(exes[0], tmp_path)
    keys = [(1, 500)] * 3 + [(1, 100 * k) for k in range(13)]
    assert order(keys) == sorted(range(16), key=lambda k: keys[k]) == ar.index_vector(keys)
    keys = [(2, 7)] + [(1, 500), (1, 100), (1, 500)] + [(1, 1000 + k) for k in range(13)]
    got = order(keys)
    assert sorted(got) == list(range(17)) and [keys[k] for k in got] == sorted(keys) and ar.index_vector(keys, order) == got
    with pytest.raises(ValueError):
        ar.index_vector(keys)


# ---------------------------------------------------------------- (c)

@pytest.mark.parametrize("lc", ac.loud_cases(), ids=[x[0] for x in ac.loud_cases()])
def test_loud_cases(exes, tmp_path, lc):
    label, hits, names = lc
    c = ac.case(label, [(0, hits)], None)
    with pytest.raises(ar.Loud):
        restated(c)
    out = run_sim(exes[0], [c], tmp_path)
    assert out.startswith("L ") and names in out and "O " not in out


# ---------------------------------------------------------------- (d)

def test_sim_under_the_sanitizers(exes, tmp_path, crowd):
    """the sanitizer build as a process of its own"""
    everything = CASES + crowd + [ac.case(label, [(0, hits)], None) for label, hits, _n in ac.loud_cases()]
    assert run_sim(exes[1], everything, tmp_path) == run_sim(exes[0], everything, tmp_path)
    keys = "".join("%d %d\n" % (1, 500 if k % 3 == 0 else k) for k in range(40))
    assert run_sim(exes[1], keys, tmp_path, "order") == run_sim(exes[0], keys, tmp_path, "order")


# ---------------------------------------------------------------- (e)

def test_mapq_table(exes):
    for exe in exes:
        r = subprocess.run([exe, "mapq"], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout == "MAPQ 50 3 1 1 0 0\n"


def test_symbols_are_part_of_the_abi():
    assert {"thj_juncbed_collect_accepted", "thj_juncbed_report_bam"} <= set(host.ABI_SYMBOLS)
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "thj.h")).read()
    assert "int thj_juncbed_collect_accepted(thj_ctx* ctx, int32_t on, int32_t library_type, const char* rg_id, const int32_t* tid_of_ref, int32_t n_ref);" in hdr
    assert "int thj_juncbed_report_bam(thj_ctx* ctx, const thj_bam_piece* piece," in hdr
    assert hasattr(host.Context, "juncbed_collect_accepted") and hasattr(host.Context, "juncbed_report_bam")
