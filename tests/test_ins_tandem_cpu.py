"""CPU: which of ONE read's sightings wins a contested insertion of stage 1 (tests/ins_tandem.py): the low 16 bits of ins_prio -- the
segment pair, li, ri -- where tests/test_ins_conflicts_cpu.py pins the ordinal above them.  The plants are checked with the oracle
alone, a read at a time; then the CPU build of the kernel logic (tests/hostsim) has to agree with the oracle on every scenario, as
the kernels split the reads and by the general enumeration, by the loops and by the wave; its priorities are read back bit by bit;
and flat2_read's index word, which the device never materialises, is compared with indels_enumerate's (tests/flat2sim)."""
import os
import subprocess

import pytest

import ins_tandem as it
import sim
from locked_make import locked_make
from util import assert_events_equal

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("name", it.NAMES)
def test_plants_pass_the_self_check(name):
    """every sighting of every contest alone reports the contest's key with its own letters, the read with both the letters of the
    one visited first (the reference alone says so); the scenario holds the contests it promises, in both polarities; the rules
    "last visited", "smallest letters", "largest letters" each get a third of the contests wrong at the least"""
    sc = it.scenario(name)
    counts = it.self_check(sc)
    print(name, len(sc.contests), "contests:", ", ".join("%s %d" % ("/".join(k), v) for k, v in counts.items()))
    wrong = {k: len(v) for k, v in it.wrong_by_rule(sc).items()}
    print(name, "contests a wrong rule loses:", wrong)
    assert wrong["first visited"] == 0
    assert wrong["last visited"] == len(sc.contests)
    for rule in ("last visited", "smallest letters", "largest letters"):
        assert 3 * wrong[rule] >= len(sc.contests), (rule, wrong)
    want = it.expected(name)
    it.assert_first_wins(sc, want, "oracle")
    b = sc.batches[0].sb
    per_read = {int(n) for n in (b.seg_off[b.nseg::b.nseg] - b.seg_off[:-1:b.nseg])}
    if name == "two":
        assert int((b.seg_off[1:] - b.seg_off[:-1]).max()) == 2 and 6 in per_read
    if name == "paths":
        assert it.PATHS_HITS <= per_read, sorted(per_read)
    assert len(want.deletions) > 5 and len(want.insertions) > len(sc.contests) + 5       # the fillers' own events


def _lost(rule: str, *tokens):
    """(contests with these tokens in their notes, those of them that `rule` gets wrong) over all scenarios"""
    have = [c.note for n in it.NAMES for c in it.scenario(n).contests if set(tokens) <= set(c.note.split("/"))]
    lost = [x for n in it.NAMES for x in it.wrong_by_rule(it.scenario(n))[rule] if set(tokens) <= set(x.split("/"))]
    return len(have), len(lost)


def test_every_wrong_rule_loses_named_contests():
    """a re-ranking of the oracle-certified sightings (ins_tandem.RULES) under the ways the priority's low bits could be wrong: each
    loses the layout planted against it -- all of its contests, or, where the wrong priorities tie and the smaller letters decide,
    those of one polarity"""
    for rule, tokens, share in (
            ("li and ri swapped", ("same", "0,1-1,0"), 1.0),             # crossed: li says one order, ri the other
            ("li and ri swapped", ("same", "3,40-4,0"), 1.0),
            ("i dropped", ("across", "1,1-0,0"), 1.0),                   # (li, ri) alone would put the pair i + 1 first
            ("i dropped", ("across", "pairs12,13", "1,1-0,0"), 1.0),
            ("li in 5 bits, cut off", ("same", "31,5-32,0"), 1.0),
            ("li in 5 bits, carried into i", ("across", "34,0-1,0"), 1.0),       # passes the pair i + 1's (1, 0)
            ("ri in 5 bits, carried into li", ("same", "3,40-4,0"), 1.0),
            ("ri in 5 bits, carried into li", ("same", "39,40-40,0"), 1.0),
            ("ri in 5 bits, carried into li", ("same", "2,32-3,0"), 0.5),        # ties
            ("smallest letters", ("first-larger",), 1.0),
            ("largest letters", ("first-smaller",), 1.0)):
        have, lost = _lost(rule, *tokens)
        print("%-32s %-28s loses %d of %d" % (rule, "/".join(tokens), lost, have))
        assert have >= 4 and lost == int(have * share), (rule, tokens, have, lost)
    for rule in it.RULES:
        if rule != "first visited":
            assert sum(len(it.wrong_by_rule(it.scenario(n))[rule]) for n in it.NAMES) >= 4, rule


@pytest.mark.parametrize("name", it.NAMES)
def test_hostsim(name, monkeypatch):
    """the CPU build of the kernel logic on every scenario: as the kernels split the reads (flat_read for one hit a segment), the
    general enumeration for all, and wave_read_enumerate (li is the lane) for the reads of several hits a segment"""
    sc = it.scenario(name)
    want = it.expected(name)
    runs = [(sc.params(0), sc.batches[0].sb, sc.batches[0].ordinal_base)]
    for env in ({}, {"THJ_HOSTSIM_NO_FLAT": "1"}, {"THJ_HOSTSIM_WAVE": "1"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        got = sim.segjuncs_batches(sc.seqs, runs)
        assert_events_equal(got, want, "%s %s" % (name, env))
        it.assert_first_wins(sc, got, "hostsim %s" % env)
        assert got.stats["indel_pairs"] == want.stats["indel_pairs"] and got.stats["windows"] == want.stats["windows"]
        for k in env:
            monkeypatch.delenv(k)


@pytest.mark.parametrize("name", ["two", "paths"])
def test_hostsim_two_batches(name):
    """the contests' batch as two with ordinal_base running on, handed over in both orders: the oracle's events of the halves merge
    to those of the batch, and so do the CPU build's sightings"""
    import orc
    from tophat_amd.batch import merge_events
    sc, want = it.scenario(name), it.expected(name)
    g = orc.Genome(sc.seqs)
    (a, _), (b, _) = it.halves(sc)
    assert_events_equal(merge_events(orc.segjuncs(sc.params(0), g, a), orc.segjuncs(sc.params(0), g, b)), want, name)
    runs = [(sc.params(0), sb, base) for sb, base in it.halves(sc)]
    for order in (runs, runs[::-1]):
        got = sim.segjuncs_batches(sc.seqs, order)
        assert_events_equal(got, want, name)
        it.assert_first_wins(sc, got, "hostsim")


def test_hostsim_pair_and_stage_2():
    """`two` with its plain right batch; then the CPU build of the stitch logic with the oracle's stage-1 sets: the oracle's records"""
    import orc
    from tophat_amd.batch import events_to_span_inputs
    sc = it.scenario("two")
    got = sim.segjuncs_batches(sc.seqs, [(sc.params(bi), sc.batches[bi].sb, sc.batches[bi].ordinal_base) for bi in (1, 0)])
    assert_events_equal(got, it.expected_pair("two"), "pair")
    it.assert_first_wins(sc, got, "hostsim, both sides")
    want = it.expected("two")
    jj, ii = events_to_span_inputs(want)
    sb = it.span_batch(sc, 0)
    recs = sim.spanning(sc.params(0), sc.seqs, sb, jj, ii)[0]
    assert recs == orc.spanning(sc.params(0), orc.Genome(sc.seqs), sb, jj, ii) and len(recs) > 300
    rows = {rid: k for k, rid in enumerate(sb.read_id.tolist())}
    n = sum(1 for c in sc.contests if any(a.read_idx == rows[c.rid] and any((q >> 28) == 3 for q in a.cigar) for a in recs))
    print("contest reads with an alignment through an insertion:", n, "of", len(sc.contests))


@pytest.mark.parametrize("name", ["two", "paths", "long"])
def test_hostsim_priorities_bit_by_bit(name):
    """what the CPU build hands to the insertion table for a contest's read at the contest's place: exactly its two sightings, each
    with the low bits i << 12 | li << 6 | ri of the visit the oracle-certified plant says brings those letters"""
    from tophat_amd import host
    sc = it.scenario(name)
    b = sc.batches[0]
    _j, _d, raw, _st = sim.segjuncs_raw(sc.params(0), sc.seqs, b.sb, b.ordinal_base)
    by = {}
    for ref, left, ln, seq, prio in raw:
        by.setdefault(((ref, left, ln), prio >> 16), set()).add((prio & 0xFFFF, host.decode_ins_seq(seq, ln)))
    for c in sc.contests:
        want = {((i & 15) << 12 | li << 6 | ri, x) for i, li, ri, x in c.sights}
        assert by.get((c.key, sc.ordinal(c.batch, c.rid))) == want, (c.note, c.rid)


def test_flat2_read_index_words():
    """flat2_read's (a | b << 16) and hit indices of its indel tasks against indels_enumerate's on generated reads with two and more
    candidate pairs a segment pair, as sets, and against the lists themselves; plain and under the sanitizers, a process each"""
    d = os.path.join(HERE, "flat2sim")
    locked_make(d)
    seen = None
    for exe in ("flat2sim", "flat2sim_san"):
        r = subprocess.run([os.path.join(d, exe), "pairs", "15", "20000"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        line = [x for x in r.stdout.splitlines() if x.startswith("FLAT2PAIRS")][0].split()
        c = {line[k]: int(line[k + 1]) for k in range(1, len(line), 2)}
        print(exe, c)
        assert c["reads"] == 20000 and c["differ"] == 0 and min(c["two_pairs"], c["four_pairs"], c["antisense"], c["second_pair"]) >= 100
        assert seen is None or c == seen
        seen = c
