"""CPU: accepted_hits.bam for paired input.  (a) the restatement (accepted_pair_ref.py, through the reference's SAM text) gives the records
written out by hand in accepted_pair_cases.py, and so do the core's paired paths (thj_accepted_core.h: emit() with a Mate, thj_pair_core.h:
happy()) compiled for the CPU by tests/acceptedpairsim; (b) on a seeded crowd of 300 inserts the core gives the restatement's records, byte
for byte; (c) happy(), TLEN, the side rule of XS:A and the happy bit the running best is left with, over seeded crowds of grades; (d) the
loud cases are loud in both; (e) the sanitizer build, run as a program of its own, is clean on all of it; (f) the ABI names the call."""
import os
import struct
import subprocess

import numpy as np
import pytest

import accepted_pair_cases as apc
import accepted_pair_ref as apr
import best_ref as br
from locked_make import locked_make
from tophat_amd import host

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = apc.cases()


@pytest.fixture(scope="module")
def exes():
    d = os.path.join(HERE, "acceptedpairsim")
    locked_make(d)
    return os.path.join(d, "acceptedpairsim"), os.path.join(d, "acceptedpairsim_san")


def run_sim(exe, text, tmp_path, mode="rewrite"):
    p = tmp_path / "cases.txt"
    p.write_text(text)
    r = subprocess.run([exe, mode, str(p)], capture_output=True, text=True)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-2000:])
    return r.stdout


def sim_text(c, raw, cfg):
    """the inserts of a case as acceptedpairsim reads them: pair_ref's choice (watched), the records with what the grade kept of them"""
    ch, plan = apr.watched_choose(c["L"], c["R"], c["best"], c["pair"], c.get("anchor", 8), c.get("known", ()), c.get("limits"))
    sides, known, mp = {"L": c["L"], "R": c["R"]}, set(c.get("known", ())), c["best"][2]
    out = ["C %d %s %d\n" % (cfg["library_type"], cfg["rg"] or "-", len(cfg["names"]))]
    out += ["N %d %d %s\n" % (k + 1, cfg["header"].index(n) if n in cfg["header"] else -1, n) for k, n in enumerate(cfg["names"])]

    def line(tag, s, k):
        S = sides[s]
        h = apr.hit_of(S, raw[s], k, br.score(S["recs"][k], S["AS"][k], ch["js1"], known, mp))
        return "%s %d %d %d %d %d %s\n" % (tag, h["ref"], h["left"], h["right"], h["anti"], h["score"], h["d"].hex())
    for item in plan:
        if item[0] == "pairs":
            _k, _num, hits, draw, is_happy = item
            out.append("P %d %d %d\n" % (draw, len(hits), is_happy))
            for a, b in hits:
                out += [line("L", "L", a), line("R", "R", b)]
        else:
            _k, _num, s, ks, draw = item
            out.append("S %d %d %d\n" % (draw, len(ks), 1 if s == "L" else 2))
            out += [line("R", s, k) for k in ks]
    return "".join(out)


def as_text(records):
    return "".join("O %s\n" % r.hex() for r in records)


# ---------------------------------------------------------------- (a)

@pytest.mark.parametrize("c", CASES, ids=[c["label"] for c in CASES])
def test_restatement_gives_the_hand_written_records(c):
    got, _seen = apr.accepted(c, apc.raw_of(c), c["cfg"])
    assert got == c["want"]


def test_core_gives_the_hand_written_records(exes, tmp_path):
    for exe in exes:
        for c in CASES:
            assert run_sim(exe, sim_text(c, apc.raw_of(c), c["cfg"]), tmp_path) == as_text(c["want"]), c["label"]


def flag_of(r):
    return struct.unpack_from("<H", r, 4 + 14)[0]


def test_the_cases_show_what_they_are_about():
    by = {c["label"]: c["want"] for c in CASES}
    assert [flag_of(r) & 0x2 for r in by["too_far_support_10"]] == [2, 2] and [flag_of(r) & 0x2 for r in by["too_far_support_9"]] == [0, 0]
    assert [struct.unpack_from("<i", r, 4 + 28)[0] for r in by["tlen_left_contains_right"]] == [-300, 300]
    assert [struct.unpack_from("<i", r, 4 + 28)[0] for r in by["tlen_right_contains_left"]] == [300, -300]
    assert [struct.unpack_from("<ii", r, 4 + 20) for r in by["other_contig"]] == [(0, 1000), (1, 1240)]
    assert all(flag_of(r) & 0x8 and not flag_of(r) & 0x2 for r in by["single_end_way_mixed"] + by["singletons_mixed"])
    assert by["single_end_way_default_writes_nothing"] == [] and by["singletons_default_write_nothing"] == [] and by["over_the_cap_suppressed"] == []
    assert len(by["left_1_right_2"]) == 4 and by["left_1_right_2"][1][36:] != by["left_1_right_2"][3][36:]      # the left record twice, two mates
    assert [flag_of(r) & 0x100 for r in by["mix_of_draws"]] == [0x100, 0, 0, 0, 0x100, 0x100, 0, 0]


@pytest.mark.parametrize("n", range(1, 7))
def test_mapq(exes, tmp_path, n):
    c = apc.mapq_case(n)
    raw = apc.raw_of(c)
    got, _seen = apr.accepted(c, raw, c["cfg"])
    assert got == c["want"]                                     # the records written out by hand
    assert len(got) == 2 * n and all(g[4 + 9] == apc.MAPQ[n] for g in got) and all(b"NHC" + bytes([n]) in g for g in got)
    assert run_sim(exes[0], sim_text(c, raw, c["cfg"]), tmp_path) == as_text(c["want"])


# ---------------------------------------------------------------- (b)

@pytest.fixture(scope="module")
def crowd():
    c = apc.crowd()
    return c, apc.raw_of(c, apc.crowd_extra)


@pytest.mark.parametrize("lt,rg", ((2, "grp"), (3, ""), (1, "")))
def test_crowd(exes, tmp_path, crowd, lt, rg):
    c, raw = crowd
    cfg = apc.cfg_of(lt, rg)
    want, seen = apr.accepted(c, raw, cfg)
    assert seen["pairs"] > 100 and seen["sides"] > 50 and 0 < seen["happy"] < seen["pairs"] and len(want) > 500
    for exe in exes:
        assert run_sim(exe, sim_text(c, raw, cfg), tmp_path) == as_text(want)
    # what the crowd holds: secondary records, both sides alone
    flags = [flag_of(r) for r in want]
    assert any(f & 0x100 for f in flags) and any(f & 0x48 == 0x48 for f in flags) and any(f & 0x88 == 0x88 for f in flags)


def test_crowd_without_mixed_alignments(exes, tmp_path):
    c = apc.crowd(pair=(200, 20, 10000000, False, True))
    raw = apc.raw_of(c, apc.crowd_extra)
    cfg = apc.cfg_of(2)
    want, seen = apr.accepted(c, raw, cfg)
    assert seen["sides"] == 0 and seen["pairs"] > 100
    assert run_sim(exes[0], sim_text(c, raw, cfg), tmp_path) == as_text(want)
    # discordant pairs are reported: mates on two contigs
    assert any(struct.unpack_from("<i", r, 4)[0] != struct.unpack_from("<i", r, 4 + 20)[0] >= 0 for r in want)


# ---------------------------------------------------------------- (c)

def test_happy_tlen_and_the_side_rule(exes, tmp_path):
    rng = np.random.default_rng(3)
    lines, want = [], []
    for _ in range(400):
        a1, s1, x1, a2, s2, x2, tf = (int(v) for v in rng.integers(0, 2, 7))
        lines.append("H %d %d %d %d %d %d %d\n" % (a1, s1, x1, a2, s2, x2, tf))
        l = (1, 0, bool(x1), [(apr.M, 20), (11, 50), (apr.M, 20)] if s1 else [(apr.M, 40)])
        r = (1, 0, bool(x2), [(apr.M, 20), (11, 50), (apr.M, 20)] if s2 else [(apr.M, 40)])
        want.append("%d" % apr.happy(l, a1, r, a2, bool(tf)))
    for _ in range(600):
        left, pl = int(rng.integers(0, 60)), int(rng.integers(0, 60))
        right, pr = left + int(rng.integers(1, 40)), pl + int(rng.integers(1, 40))
        lines.append("T %d %d %d %d\n" % (left, right, pl, pr))
        want.append("%d" % apr.tlen(left, right, pl, pr))
    for lt in (0, 1, 2, 3):
        for anti in (0, 1):
            for side in (0, 1, 2):
                sign = apr.xs_sign(lt, bool(anti), side)
                if sign:
                    lines.append("X %d %d %d\n" % (lt, anti, side))
                    want.append(sign)
    # the running best: the first candidate in generation order that raises it leaves its happy bit, a fusion candidate too
    for _ in range(300):
        n = int(rng.integers(0, 9))
        cands = [(int(rng.integers(-6, 1)), int(rng.integers(0, 2)), int(rng.integers(0, 2))) for _ in range(n)]
        lines.append("B %d %s\n" % (n, " ".join("%d %d %d" % t for t in cands)))
        top, bit = None, -1
        for sc, _fu, hp in cands:
            if top is None or top < sc:
                top, bit = sc, hp
        want.append("%d" % bit)
    for exe in exes:
        assert run_sim(exe, "".join(lines), tmp_path, "funcs").split() == want
    assert "0" in want[:400] and "1" in want[:400] and any(int(w) < 0 for w in want[400:1000]) and any(int(w) > 0 for w in want[400:1000])


# ---------------------------------------------------------------- (d)

@pytest.mark.parametrize("lc", apc.loud_cases(), ids=[x[0] for x in apc.loud_cases()])
def test_loud_cases(exes, tmp_path, lc):
    label, c, extra, patch, header, word = lc
    raw = apc.raw_of(c, extra)
    if patch:
        patch(raw)
    cfg = apc.cfg_of(header=header)
    with pytest.raises(apr.Loud):
        apr.accepted(c, raw, cfg)
    # the sim is handed the same insert: the choice does not read the bytes
    for exe in exes:
        out = run_sim(exe, sim_text(c, raw, cfg), tmp_path)
        assert out.startswith("L ") and word in out, (label, out)


# ---------------------------------------------------------------- (f)

def test_the_abi_names_the_call():
    assert "thj_juncbed_report_pairs_bam" in host.ABI_SYMBOLS and "thj_juncbed_collect_accepted_pairs" in host.ABI_SYMBOLS
    text = open(os.path.join(HERE, "..", "include", "thj.h")).read()
    assert "int thj_juncbed_report_pairs_bam(" in text and "int thj_juncbed_collect_accepted_pairs(" in text
