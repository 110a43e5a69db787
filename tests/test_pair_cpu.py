"""CPU: the choice among an insert's alignments (thj_juncbed_pair_alignments).  (a) the restatement (pair_ref.py) gives the rows written
down by hand in pair_cases.py, and the cases show what they are about: the paired answer differs from the single-end answer over the
same records; (b) every mechanism acts on at least 10 inserts of the crowd; (c) tophat_amd/csrc/thj_pair_core.h, compiled for the CPU by
tests/pairsim, gives the restatement's grades, lists, cap flags and draws on the cases and the crowd -- also under the address and
undefined-behaviour sanitizers, run directly; (d) the std::sort helper; (e) the interface is declared and documented."""
import os
import subprocess

import pytest

import best_ref as br
import pair_cases as pc
import pair_ref as pr
from locked_make import locked_make

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MIXED, DISC = (200, 20, 10000000, True, False), (200, 20, 10000000, False, True)
# the paired answer equals the single-end one here, and why
SAME_AS_SINGLE = {
    "rescue_by_a_rejected_junction": "single-end, the rejected junction's reads are dropped too and the far record has the better AS",
    "fusion_other_contig_discordant": "the discordant pair is the best-scoring record's", "fusion_equal_strands_discordant": "as above",
    "fusion_left_distance_negative_discordant": "as above", "fusion_beyond_fusion_min_dist_discordant": "as above", "fusion_min_dist_exact": "as above",
    "left_record_in_one_pair": "the control of left_record_in_two_pairs", "cap_suppressed": "mixed alignments: both sides take the single-end way",
    "empty_list_mixed": "as above", "best_grade_is_a_fusion_grade_mixed": "as above",
}


@pytest.fixture(scope="module")
def sims():
    d = os.path.join(HERE, "pairsim")
    locked_make(d)
    return os.path.join(d, "pairsim"), os.path.join(d, "pairsim_san")


def args(c, **over):
    c = dict(c, **over)
    return c["L"], c["R"], c["best"], c["pair"], c["anchor"], c["known"], c["limits"]


def test_restatement_gives_the_hand_rows():
    labels = set()
    for c in pc.cases():
        assert pr.consensus(*args(c)) == c["want_j"], c["label"]
        j, i, d = pr.consensus(*args(c), seqs=pc.seqs_of(c))
        assert (j, d, len(i)) == (c["want_j"], c["want_d"], c["want_i"]), c["label"]
        assert c["want_ins"] is None or i == c["want_ins"], c["label"]
        labels.add(c["label"])
    assert len(labels) == len(pc.cases()) >= 40


def test_cases_show_what_they_are_about():
    differ = 0
    for c in pc.cases():
        recs, reads, AS, mism, anti, sq = pc.as_single(c, pc.seqs_of(c))
        single = br.consensus(recs, sq, c["anchor"], c["known"], c["limits"], mism, c["best"], reads, AS, anti)
        if c["label"] in SAME_AS_SINGLE:
            continue
        assert single != pr.consensus(*args(c), seqs=pc.seqs_of(c)), c["label"]
        differ += 1
    # the insertion-order case: over the same records in record order the first record's letter C would be kept
    c = [x for x in pc.cases() if x["label"] == "insertion_letters_follow_the_pair_list"][0]
    recs, reads, AS, mism, anti, sq = pc.as_single(c, c["seqs"])
    import jbknown_ref as jr
    assert [r[2] for r in jr.consensus(recs, sq, 8, (), None, mism)[1]] == ["C"] and c["want_ins"][0][2] == "G"
    assert differ >= 30
    # pairs of cases that differ in one thing give different rows
    by = {c["label"]: c["want_j"] for c in pc.cases()}
    for a, b in (("rescue_support_10", "rescue_support_9"), ("rescue_left_at_inner1", "rescue_left_before_inner1"), ("rescue_dist_180", "rescue_dist_179"),
                 ("rescue_dist_220", "rescue_dist_221"), ("pair_duplicates_neighbours", "pair_duplicates_not_neighbours"), ("left_record_in_two_pairs", "left_record_in_one_pair"),
                 ("empty_list_mixed", "empty_list_default"), ("best_grade_is_a_fusion_grade_default", "best_grade_is_a_fusion_grade_mixed"),
                 ("lone_mates_first_pass_only", "lone_mates_four"), ("cap_draws_after_singletons_and_a_pair", "cap_pairs_above_the_ties"),
                 ("fusion_other_contig_skipped", "fusion_other_contig_discordant")):
        assert by[a] != by[b], (a, b)


def test_generator_values_used_by_hand():
    g = br.Mt19937(1)
    assert tuple(g() for _ in range(6)) == (1791095845, 4282876139, 3093770124, 4005303368, 491263, 550290313)


def test_every_mechanism_acts_on_the_crowd():
    c = pc.crowd()
    pr.SEEN = {}
    try:
        for over in ({}, {"pair": MIXED}, {"pair": DISC}, {"limits": (0, 2, 2)}):
            pr.choose(*args(c, **over))
        seen = {k: len({x[1] for x in v}) for k, v in pr.SEEN.items()}
    finally:
        pr.SEEN = None
    for what in ("too_far_full", "too_far_half", "too_close", "contained", "in_window", "rescued", "fusion_op", "fusion_contig", "fusion_strand", "fusion_distance", "not_allowed",
                 "two_scores", "side_cut", "pair_duplicates", "host_sort", "over_the_cap", "cap_draws", "cap_pairs_above_the_ties", "mixed_empty_list", "mixed_fusion_grade",
                 "mate_has_nothing_left", "no_pair_in_the_first_pass", "no_pair_unfiltered", "record_in_several_pairs"):
        assert seen.get(what, 0) >= 10, (what, seen)
    assert len(pr.inserts(c["L"], c["R"])) == 600
    # and the settings give different rows
    rows = [repr(pr.consensus(*args(c, **over))) for over in ({}, {"pair": MIXED}, {"pair": DISC}, {"limits": (0, 2, 2)}, {"best": (2, True, 6)})]
    assert len(set(rows)) == 5


def sim_input(traces, best, pair):
    """pairsim's "lists" input for the inserts pair_best traced"""
    out = []
    classes = {}
    for t in traces:
        out.append("C %d %d %d %d %d %d %d %d %d" % (pair[0], pair[1], pair[2], best[2], best[0], pair[3], pair[4], best[1], t["final"]))
        out += ["J %d %d %d %d" % j for j in t["juncs"]]
        out.append("D %d" % t["drawn"])
        for lh, rh, _g in t["cands"]:
            f = [x for h in (lh, rh) for x in (h.ref, h.left, h.right, h.score, int(h.anti), int(h.fused), classes.setdefault(h.eq, len(classes)))]
            out.append("P " + " ".join(str(x) for x in f))
        out.append("E")
    return "\n".join(out) + "\n"


def sim_want(traces):
    out = []
    for t in traces:
        out += ["G 0 0 0" if g is None else "G 1 %d %d" % (int(g[1]), g[0]) for _l, _r, g in t["cands"]]
        out.append(" ".join(["L"] + [str(k) for k in t["kept"]]))
        out += ["S %d %d %d" % (int(t["best_fusion"]), int(t["over"]), t["used"]), "E"]
    return "\n".join(out) + "\n"


def traced(c, **over):
    pr.TRACE = []
    try:
        pr.choose(*args(c, **over))
        return [t for t in pr.TRACE if t["cands"]]
    finally:
        pr.TRACE = None


def test_core_against_the_restatement(sims):
    sim, san = sims
    n = 0
    for c in pc.cases() + [pc.crowd(), dict(pc.crowd(), pair=MIXED), dict(pc.crowd(), pair=DISC, best=(2, False, 5)), dict(pc.crowd(), best=(2, True, 6))]:
        tr = traced(c)
        text = sim_input(tr, c["best"], c["pair"])
        for exe in (sim, san) if c["label"] != "crowd" or c["pair"] == MIXED else (sim,):
            r = subprocess.run([exe, "lists"], input=text, capture_output=True, text=True, timeout=120)
            assert r.returncode == 0 and not r.stderr, (c["label"], r.stderr[-500:])
            assert r.stdout == sim_want(tr), c["label"]
        n += len(tr)
    assert n > 2000


def test_sort_helper(sims):
    """what the library's host part runs for a list of more than 16: std::sort by score descending.  17 and 40 equal scores: libstdc++'s
    introsort does not keep them in generation order, and the restatement follows it"""
    for exe in sims:
        for n in (17, 40):
            out = subprocess.run([exe, "order"], input=" ".join(["-3"] * n), capture_output=True, text=True, check=True).stdout
            order = [int(x) for x in out.split()]
            assert sorted(order) == list(range(n)) and order == pr.sort_order([-3] * n)
        mixed = [-(k * 7 % 5) for k in range(40)]
        order = [int(x) for x in subprocess.run([exe, "order"], input=" ".join(map(str, mixed)), capture_output=True, text=True, check=True).stdout.split()]
        assert [mixed[k] for k in order] == sorted(mixed, reverse=True) and order == pr.sort_order(mixed)
    assert pr.sort_order([-3] * 16) == list(range(16)) and pr.sort_order([-1, 0, -1, 0]) == [1, 3, 0, 2]


def test_interface():
    from tophat_amd import host
    assert {"thj_juncbed_pair_alignments", "thj_juncbed_add_pairs", "thj_juncbed_pair_counts"} <= set(host.ABI_SYMBOLS)
    hdr = open(os.path.join(ROOT, "include", "thj.h")).read()
    assert "int thj_juncbed_add_pairs(thj_ctx* ctx, const thj_aln* left, int64_t n_left, const thj_aln* right, int64_t n_right);" in hdr
    assert "int thj_juncbed_pair_counts(thj_ctx* ctx, int64_t* counts /*[5]*/);" in hdr and "int thj_juncbed_add_pairs_seq(thj_ctx* ctx, " in hdr
    assert "thj_juncbed_add_pairs_seq" in host.ABI_SYMBOLS and callable(host.Context.juncbed_add_pairs_seq)
    assert "pair_best_alignments and everything paired" not in hdr
    main = open(os.path.join(ROOT, "tophat_amd", "csrc", "host", "thj_junctions_main.cpp")).read()
    assert "pair_best_alignments and everything paired" not in main and "--right-maps" in main and "BamMerge is not built" in main
    for f in ("juncbed_pair_alignments", "juncbed_add_pairs", "juncbed_pair_counts"):
        assert callable(getattr(host.Context, f))
