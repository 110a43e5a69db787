"""CPU: which read wins a contested insertion of stage 1 (tests/ins_conflicts.py).  The plants are checked with the oracle alone, a
read at a time; then the CPU build of the kernel logic (tests/hostsim: ins_prio, the smallest priority of a key stays) has to agree
with the oracle's counter in visiting order -- in one batch, over the two sides, and over shards whose ordinal_base runs on."""
import pytest

import ins_conflicts as ic
import orc
import sim
from tophat_amd.batch import Events, merge_events
from util import assert_events_equal

import numpy as np


@pytest.mark.parametrize("name", ic.NAMES)
def test_plants_pass_the_self_check(name):
    """every contender of every contest reports the contest's key with its own letters (the reference alone says so), and the
    wrong rules -- the last one, the smallest letters, the largest letters -- each get contests of the scenario wrong"""
    sc = ic.scenario(name)
    ic.self_check(sc)
    wrong = ic.losers_rules(sc)
    assert all(n >= sc.min_contests // 2 for n in wrong.values()), wrong
    assert wrong["last"] == len(sc.contests)
    want = ic.expected(name)
    ic.assert_first_wins(sc, want, "oracle")
    assert len(want.deletions) > 5 and len(want.insertions) > len(sc.contests) + 5       # the fillers' own events


def _sim_runs(sc, order):
    return [(sc.params(bi), sc.batches[bi].sb, sc.batches[bi].ordinal_base) for bi in order]


@pytest.mark.parametrize("name", ["paths", "wide50", "wide64", "long"])
def test_hostsim_one_batch(name, monkeypatch):
    sc = ic.scenario(name)
    want = ic.expected(name)
    for general in (False, True):       # as the kernels split the reads (flat_read for one hit a segment), and the general enumeration for all
        if general:
            monkeypatch.setenv("THJ_HOSTSIM_NO_FLAT", "1")
        got = sim.segjuncs_batches(sc.seqs, _sim_runs(sc, sc.order()))
        assert_events_equal(got, want, name)
        ic.assert_first_wins(sc, got, "hostsim")
        assert got.stats["indel_pairs"] == want.stats["indel_pairs"] and got.stats["windows"] == want.stats["windows"]


@pytest.mark.parametrize("name", ["sides", "shards", "ranks", "range", "growth"])
def test_hostsim_several_batches(name):
    """left then right, three shards of one side, the four shards of a paired run: the sightings of all batches reduced at once, the
    batches handed over in visiting order and in the opposite one -- the ordinal decides"""
    sc = ic.scenario(name)
    want = ic.expected(name)
    for order in (sc.order(), sc.order()[::-1]):
        got = sim.segjuncs_batches(sc.seqs, _sim_runs(sc, order))
        assert_events_equal(got, want, name)
        ic.assert_first_wins(sc, got, "hostsim")


def test_hostsim_needs_the_ordinal_base():
    """the same batches with every ordinal_base 0: rows of different batches tie or swap, and contests go to the wrong read -- the
    scenarios do depend on the ordinals running on"""
    sc = ic.scenario("shards")
    got = sim.segjuncs_batches(sc.seqs, [(sc.params(bi), sc.batches[bi].sb, 0) for bi in sc.order()])
    have = {(r, l, len(s)): s for r, l, s in got.insertions}
    assert sum(1 for c in sc.contests if have[c.key] != c.winner) >= 8


def test_merge_events_keeps_the_earlier_operand():
    nj = np.zeros(0, dtype=orc.JUNC_DTYPE)
    a = Events(nj, nj, [(1, 100, "AC"), (1, 200, "T")], {})
    b = Events(nj, nj, [(1, 100, "TT"), (1, 100, "TTT"), (2, 100, "GG")], {})
    assert merge_events(a, b).insertions == [(1, 100, "AC"), (1, 100, "TTT"), (1, 200, "T"), (2, 100, "GG")]
    assert merge_events(b, a).insertions == [(1, 100, "TT"), (1, 100, "TTT"), (1, 200, "T"), (2, 100, "GG")]


def test_a_read_that_sights_its_insertion_twice_brings_the_same_letters():
    """the priority's segment pair / li / ri bits order the sightings of ONE read; the planted reads that sight their insertion from
    two pairs of segments bring the same letters both times (both left hits lie on one diagonal of the read), so among the planted
    reads the ordinal alone decides the letters"""
    sc = ic.scenario("paths")
    _j, _d, raw, _st = sim.segjuncs_raw(sc.params(0), sc.seqs, sc.batches[0].sb, sc.batches[0].ordinal_base)
    by = {}
    for ref, left, ln, seq, prio in raw:
        by.setdefault(((ref, left, ln), prio >> 16), []).append((prio & 0xFFFF, seq))
    twice = {k: v for k, v in by.items() if len(v) > 1}
    planted = [(c.key, sc.ordinal(bi, rid)) for c in sc.contests if c.note.startswith("sighted twice") for bi, rid, _x in c.contenders]
    assert sum(1 for k in planted if k in twice) >= 8
    for k, v in twice.items():
        assert len({low for low, _s in v}) == len(v) and len({s for _l, s in v}) == 1, (k, v)


def test_hostsim_stage_2_after_a_contested_stage_1():
    """the CPU build of the stitch logic with the oracle's stage-1 sets: the oracle's records; the winners align through their
    insertions, the losers do not (and would with their own letters in the set)"""
    from tophat_amd.batch import events_to_span_inputs
    sc, want = ic.scenario("stitch"), ic.expected("stitch")
    g = orc.Genome(sc.seqs)
    jj, ii = events_to_span_inputs(want)
    sbs = [ic.span_batch(sc, bi) for bi in sc.order()]
    p = sc.params(0)
    recs = [sim.spanning(p, sc.seqs, sb, jj, ii)[0] for sb in sbs]
    assert recs == [orc.spanning(p, g, sb, jj, ii) for sb in sbs]
    assert ic.check_stage2(sc, sbs, recs, p, g, jj, ii) >= 8
