"""CPU: the choice among a read's alignments (thj_juncbed_best_alignments).  (a) the restatement (best_ref.py) gives the rows written
out by hand in best_cases.py, its generator is MT19937, and with the switch off it is jbknown_ref; (b) on the crowd every mechanism
acts on at least 20 reads; (c) tophat_amd/csrc/thj_best_core.h, compiled for the CPU by tests/bestsim, gives the restatement's ranks,
first-pass duplicates, scores, keep flags and draws on the cases and the crowd, also under ASan / UBSan, and its generator is
std::mt19937's; (d) the record core's AS:i parse."""
import os
import subprocess

import pytest

import best_cases as bc
import best_ref as br
import indelbed_cases as ic
import indelbed_ref as ir
import jbknown_ref as jr
from ingest_cases import cw, record, tag, write_bam
from locked_make import locked_make
from tophat_amd import host

HERE = os.path.dirname(os.path.abspath(__file__))
LENS = [len(s) for s in bc.GENOME]
CASES = bc.cases()


def restated(c, seqs=None, **over):
    c = dict(c, **over)
    return br.consensus(c["recs"], seqs, c["anchor"], c["known"], c["limits"], c["mism"], c["best"], c["reads"], c["AS"], c["anti"])


# ---------------------------------------------------------------- (a)

def test_generator_is_mt19937():
    g = br.Mt19937(1)
    assert tuple(g() for _ in range(6)) == bc.MT_SEED1


@pytest.mark.parametrize("c", CASES, ids=[c["label"] for c in CASES])
def test_cases_by_hand(c):
    seqs = ic.make_seqs(c["recs"], 1)
    js, ins, dels = restated(c, seqs)
    assert (js, dels, len(ins)) == (c["want_j"], c["want_d"], c["want_i"])
    assert restated(c)[0] == js                                 # and without the indel sets


def test_the_cases_show_what_they_are_about():
    by = {c["label"]: c for c in CASES}
    # the choice matters: with the switch off every record counts
    for label in ("support4", "pass1_duplicates_count_once", "rights_A_B_A", "cap_2_of_5", "fusion_junction_under_the_first_contig"):
        c = by[label]
        seqs = ic.make_seqs(c["recs"], 1)
        assert restated(c, seqs, best=None) != restated(c, seqs), label
        assert restated(c, seqs, best=None) == jr.consensus(c["recs"], seqs, c["anchor"], c["known"], c["limits"], c["mism"])
    c = by["pass1_duplicates_count_once"]
    ch = br.choose(c["recs"], c["reads"], c["AS"], c["mism"], c["anti"], c["best"])
    assert ch["dup1"] == [False, False, False, True, False, False] and ch["js1"][(1, 119, 620, 0)] == [20, 20, 4]
    assert ch["score"] == [-8, -8, -8, -8, -8, -6] and ch["keep"] == [True, True, True, False, False, True]
    c = by["equal_keys_different_AS"]
    ch = br.choose(c["recs"], c["reads"], c["AS"], c["mism"], c["anti"], c["best"])
    assert ch["dup1"] == [False, True] and ch["keep"] == [False, True] and ch["score"] == [-13, -8]
    c = by["rights_A_B_A"]
    ch = br.choose(c["recs"], c["reads"], c["AS"], c["mism"], c["anti"], c["best"])
    assert ch["rank"] == [2, 1, 0] and ch["dup1"] == [False] * 3 and ch["keep"] == [False, False, True]
    c = by["cap_2_of_5"]
    ch = br.choose(c["recs"], c["reads"], c["AS"], c["mism"], c["anti"], c["best"])
    assert ch["draws"] == {3: (2, [1, 3])} and ch["stats"] == (4, 1, 1, 0)      # (the read on the rejected junction lost its record; the cap is counted apart)
    ch = br.choose(c["recs"], c["reads"], c["AS"], c["mism"], c["anti"], (1, False, 6))
    assert ch["draws"] == {3: (2, [1])}
    assert br.penalty(6, 5, 20, 9, 10) == 4 and br.penalty(5, 5, 20, 9, 10) == 3 and br.penalty(6, 4, 20, 20, 10) == 8 and br.penalty(6, 5, 10, 10, 10) == 0


# ---------------------------------------------------------------- (b)

@pytest.fixture(scope="module")
def crowd():
    c = bc.crowd()
    return c, br.choose(c["recs"], c["reads"], c["AS"], c["mism"], c["anti"], c["best"])


def mechanisms(c, ch):
    """reads on which each mechanism acts -> dict of counts"""
    recs, reads, AS, mism, anti = c["recs"], c["reads"], c["AS"], c["mism"], c["anti"]
    n = dict(dup1=0, choice=0, unique2=0, exclusion=0, over=len(ch["draws"]))
    for s, e in br.groups(reads):
        idx = list(range(s, e))
        n["dup1"] += any(ch["dup1"][i] for i in idx)
        scored = [i for i in idx if ch["score"][i] is not None]
        top = max((ch["score"][i] for i in scored), default=None)
        ties = [i for i in scored if ch["score"][i] == top]
        n["choice"] += len(ties) < len(scored)
        n["unique2"] += len(br.sort_unique(ties, recs, mism, anti)[1]) < len(ties)
        # the winner without the exclusion: some excluded record scores at least what the reported ones do
        out = [i for i in idx if ch["score"][i] is None]
        n["exclusion"] += bool(scored) and any(br.score(recs[i], AS[i], ch["js1"], set(c["known"]), c["best"][2]) > top for i in out)
    return n


def test_crowd_every_mechanism_acts(crowd):
    c, ch = crowd
    assert 2500 <= len(br.groups(c["reads"])) <= 4000
    n = mechanisms(c, ch)
    assert all(v >= 20 for v in n.values()), n
    assert n["over"] == ch["stats"][2]
    seqs = ic.make_seqs(c["recs"], 3)
    on, off = restated(c, seqs), restated(c, seqs, best=None)
    assert on[0] != off[0] and on[1] != off[1] and on[2] != off[2] and len(on[0]) > 30
    assert restated(c, seqs, best=(3, True, 6)) != on != restated(c, seqs, best=(20, False, 6))


# ---------------------------------------------------------------- (c) the CPU sim

@pytest.fixture(scope="module")
def exes():
    d = os.path.join(HERE, "bestsim")
    locked_make(d)
    return os.path.join(d, "bestsim"), os.path.join(d, "bestsim_san")


def sim_text(cases):
    out = []
    for c in cases:
        limits = c["limits"]
        out.append("A %d\nF %d %d %d %d\nC %s\nB %d %d %d\n" % ((c["anchor"], 1 if limits else 0) + tuple(limits or (0, 0, 0)) + (" ".join(str(x) for x in LENS),) +
                                                               (c["best"][0], 1 if c["best"][1] else 0, c["best"][2])))
        out += ["K %d %d %d %d\n" % tuple(k) for k in c["known"]]
        for r, rd, a, mm, an in zip(c["recs"], c["reads"], c["AS"], c["mism"], c["anti"]):
            out.append("R %d %d %d %d %d %d %d %d %d %s\n" % (rd, a, 1 if an else 0, mm, r[0], r[1], 1 if r[2] else 0, r[4] if len(r) > 4 else 0, len(r[3]),
                                                                " ".join("%d %d" % tuple(x) for x in r[3])))
        out.append("E\n")
    return "".join(out)


def run_sim(exe, cases, tmp_path):
    p = tmp_path / "cases.txt"
    p.write_text(sim_text(cases))
    r = subprocess.run([exe, "choose", str(p)], capture_output=True, text=True)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-2000:])
    return r.stdout


def expected_text(cases):
    out = []
    for c in cases:
        ch = br.choose(c["recs"], c["reads"], c["AS"], c["mism"], c["anti"], c["best"], c["anchor"], c["known"], c["limits"])
        for k in range(len(c["recs"])):
            out.append("R %d %d %s %d\n" % (-1 if ch["rank"][k] is None else ch["rank"][k], 1 if ch["dup1"][k] else 0, "x" if ch["score"][k] is None else ch["score"][k],
                                            1 if ch["keep"][k] else 0))
        out += ["W %d %d %s\n" % (s, at, " ".join(str(t) for t in tie)) for s, (at, tie) in sorted(ch["draws"].items())]
        out.append("S %d %d %d %d\nE\n" % ch["stats"])
    return "".join(out)


def variants(c):
    """the crowd as it is, with a third of its junctions annotated, with the read filter, capped harder and suppressed"""
    distinct = sorted({j[:4] for r in c["recs"] for j in ir.rec_juncs(r)})
    return [c, dict(c, known=distinct[::3]), dict(c, limits=(0, 2, 2)), dict(c, best=(1, False, 5), anchor=12), dict(c, best=(2, True, 6))]


def test_sim_generator(exes):
    for exe in exes:
        r = subprocess.run([exe, "mt"], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout == "MT ok %d %d %d %d\n" % bc.MT_SEED1[:4], (r.stdout, r.stderr[-500:])


def test_sim_on_the_cases(exes, tmp_path):
    assert run_sim(exes[0], CASES, tmp_path) == expected_text(CASES)


def test_sim_on_the_crowd(exes, tmp_path, crowd):
    vs = variants(crowd[0])
    want = expected_text(vs)
    assert run_sim(exes[0], vs, tmp_path) == want
    assert want.count("\nW ") > 100 and " x " in want and "R -1 " in want


def test_sim_under_the_sanitizers(exes, tmp_path):
    """the sanitizer build as a process of its own"""
    vs = CASES + variants(bc.crowd(seed=4, n_reads=400))
    assert run_sim(exes[1], vs, tmp_path) == expected_text(vs)


# ---------------------------------------------------------------- (d) AS:i

AS_TAGS = [("c", -7), ("C", 200), ("s", -300), ("S", 40000), ("i", -32768), ("I", 32767), ("i", -32769), ("I", 70000), None, ("i", 0)]


def test_AS_parse(exes, tmp_path):
    recs = []
    for k, t in enumerate(AS_TAGS):
        aux = tag("NM", "C", 1) + (b"" if t is None else tag("AS", t[0], t[1])) + tag("XS", "A", "+") + tag("ZZ", "f", b"\0\0\0\0")
        recs.append(record("r%d" % k, tid=0, pos=100 + k, cigar=[cw(0, 20)], seq=[1] * 20, aux=aux))
    bam = write_bam(str(tmp_path / "as.bam"), [(recs[:4], 6), (recs[4:], 0)], targets=(("chrA", 20000),)).path
    want = "".join("D 64\n" if t is None or not -32768 <= t[1] <= 32767 else "K %d\n" % t[1] for t in AS_TAGS)
    assert want.count("D 64") == 4
    for exe in exes:
        r = subprocess.run([exe, "as", bam], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout == want and "runtime error" not in r.stderr, (r.stdout, r.stderr[-500:])


def test_symbols_are_part_of_the_abi():
    assert {"thj_juncbed_best_alignments", "thj_juncbed_best_counts"} <= set(host.ABI_SYMBOLS)
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "thj.h")).read()
    assert "int thj_juncbed_best_alignments(thj_ctx* ctx, int32_t on, int32_t max_multihits, int32_t suppress_hits, int32_t bowtie2_max_penalty);" in hdr
    assert "#define THJ_ABI_VERSION 2" in hdr
