"""CPU: the spanning records of planted reads (tests/md_edges.py) from the CPU build of thj_span_core.h against the oracle.  Every
family first shows, on the oracle's records alone, that it reaches the edge it is named after -- an MD string of exactly 40 and of 41
characters, a token of every size at every offset of the MD buffer, a deletion's `^` on every offset mod 8, records on both sides
of QCAP with the quality bytes that lie at the ends of the phred range, a mismatch on either side of every 64-base piece edge --
and then requires the four modes of the twin (chain entries -> join -> finish; the generic path alone; no packed tier, no chains;
tiny packed limits) to give those records."""
import os
import re

import pytest

import md_edges as me
import sim
from tophat_amd import host

MODES = (0, 1, 2, 3)
HOST_MD = "<left to the host>"


def on_host(alns):
    """MD strings the record does not hold (thj_md_string formats them): kept when libthj_hip.so is there to do it, else masked"""
    import dataclasses
    return [dataclasses.replace(a, MD=HOST_MD) if len(a.MD) > 40 else a for a in alns]


def run_modes(case, want, monkeypatch, modes=MODES, chains=None):
    """sim.spanning in every mode == want; chains: whether hostsim_chain_reads must show the chain path in modes 0 and 3"""
    seqs, sb, p, juncs, ins, tags = case
    want = list(want)
    if not os.path.exists(host.LIB_PATH):
        monkeypatch.setattr(host, "md_on_host", lambda *a, **k: HOST_MD)
        want = on_host(want)
    n_long = sum(1 for a in want if len(a.MD) > 40 or a.MD == HOST_MD)
    for mode in modes:
        sim.lib().hostsim_chain_reads()                              # (the library's counter: read = reset)
        got, status = sim.spanning(p, seqs, sb, juncs, ins, mode)
        n_chain = sim.lib().hostsim_chain_reads()
        assert status[1] == 0 and status[2] == 0, (mode, status)
        got.sort(key=lambda a: a.read_idx)
        assert got == want, "mode %d: %s" % (mode, me.explain(got, want, tags))
        assert sum(1 for a in got if len(a.MD) > 40 or a.MD == HOST_MD) == n_long
        if chains is not None and mode in (0, 3):
            assert (n_chain > 0) == chains, (mode, n_chain)
    return n_long


def by_tag(want, tags):
    out = {}
    for a in want:
        out.setdefault(tags[a.read_idx], []).append(a)
    return out


def spliced(a):
    return any((c >> 28) == 11 for c in a.cigar)


# ------------------------------------------------------------------------------------------------ MD length ladder
def check_ladder(want, tags):
    assert {a.read_idx for a in want} == set(range(len(tags)))                      # every planted read has its record
    for anti in (False, True):
        for sp in (False, True):
            lens = {len(a.MD) for a in want if a.antisense == anti and spliced(a) == sp}
            assert lens >= set(range(3, 45)), (anti, sp, sorted(set(range(3, 45)) - lens))
    assert all(a.XM == a.MD.count("A") + a.MD.count("C") + a.MD.count("G") + a.MD.count("T") for a in want)
    # one- and two-digit runs are mixed
    assert any(re.search(r"\d\d[ACGT]\d[ACGT]", a.MD) for a in want) and any(re.search(r"[ACGT]\d[ACGT]\d\d[ACGT]", a.MD) for a in want)


def test_md_length_ladder(monkeypatch):
    (case,), (want,) = me.family("ladder"), me.expected("ladder")
    check_ladder(want, case[5])
    n_long = run_modes(case, want, monkeypatch, chains=True)
    assert n_long == sum(1 for a in want if len(a.MD) > 40) > 0


# ------------------------------------------------------------------------------------------------ word-offset sweep
def token_table(wants):
    table = {}
    for want in wants:
        for a in want:
            if len(a.MD) <= 40:                                     # the strings the record builders deliver themselves
                for t in me.md_tokens(a.MD):
                    table.setdefault(t, a.MD)
    return table


def check_sweep(wants):
    table = token_table(wants)
    every = {(o, n) for o in range(40) for n in (1, 2, 3, 4)}
    assert every - set(table) <= me.MD_UNREACHABLE, sorted(every - set(table) - me.MD_UNREACHABLE)
    assert not (set(table) & me.MD_UNREACHABLE), "a pair listed as unreachable was reached"
    # the four-character tokens are of both kinds: three digits and a letter, four letters of a deletion
    mds = [a.MD for want in wants for a in want]
    assert any(re.search(r"\d\d\d[ACGT]", m) for m in mds) and any(re.search(r"\^[ACGT]{4}", m) for m in mds)
    assert any(spliced(a) and re.search(r"\d\d\d[ACGT]", a.MD) for want in wants for a in want)


def test_md_tokeniser():
    assert me.md_tokens("100") == [(0, 3)]
    assert me.md_tokens("0A12C100T7") == [(0, 2), (2, 3), (5, 4), (9, 1)]
    assert me.md_tokens("24G0^ACGTA0T74") == [(0, 3), (3, 2), (5, 4), (9, 1), (10, 2), (12, 2)]


def test_word_offset_sweep(monkeypatch):
    cases, wants = me.family("sweep"), me.expected("sweep")
    check_sweep(wants)
    assert {sb.nseg for _s, sb, *_r in cases} == {4, 6, 10}        # 100, 150 and 250 bases
    for case, want in zip(cases, wants):
        assert {a.read_idx for a in want} == set(range(len(case[5])))
        run_modes(case, want, monkeypatch)


# ------------------------------------------------------------------------------------------------ deletions and insertions
def check_indels(want, tags):
    assert {a.read_idx for a in want} == set(range(len(tags)))
    dels = [a for a in want if a.XO and any((c >> 28) == 5 for c in a.cigar)]
    inss = [a for a in want if a.XO and any((c >> 28) == 3 for c in a.cigar)]
    assert {c & 0xFFFFFFF for a in dels for c in a.cigar if (c >> 28) == 5} == {1, 3, 4, 5, 8, 10}
    assert {c & 0xFFFFFFF for a in inss for c in a.cigar if (c >> 28) == 3} == {1, 2, 3}
    for group in (dels, inss):
        assert any(a.antisense for a in group) and any(not a.antisense for a in group)
    caret, letters4 = set(), set()
    for a in dels:
        assert re.search(r"[ACGT]0\^[ACGT]+0[ACGT]", a.MD), a.MD     # a mismatch on the base before and on the base behind
        toks = me.md_tokens(a.MD)
        at = a.MD.index("^")
        caret.add((at - 1) % 8)
        letters4 |= {o % 8 for o, n in toks if n == 4 and o > at}
    assert caret == set(range(8)) and letters4 == set(range(8)), (caret, letters4)
    # strings that pass the lead line's 24 characters and the record's 40 inside the deletion's letters
    for limit in (24, 40):
        assert any(a.MD.index("^") < limit < a.MD.index("^") + 1 + sum(c & 0xFFFFFFF for c in a.cigar if (c >> 28) == 5) for a in dels), limit
    assert any(24 < len(a.MD) <= 40 for a in dels) and any(len(a.MD) > 40 for a in dels)
    assert all(a.XM >= 3 for a in inss)                             # the mismatches next to the insertion stay mismatches


def test_deletions_and_insertions(monkeypatch):
    (case,), (want,) = me.family("indels"), me.expected("indels")
    check_indels(want, case[5])
    assert run_modes(case, want, monkeypatch, chains=True) > 0


# ------------------------------------------------------------------------------------------------ quality edges
def check_qualities(case, want):
    seqs, sb, p, juncs, ins, tags = case
    assert {a.read_idx for a in want} == set(range(len(tags)))      # the both-N reads among them: check_editdist_consistency's second clause
    t = by_tag(want, tags)
    for k in (5, 6, 7, 12):
        for g in ("plain", "spliced", "deleted"):
            for strand in ("sense", "anti"):
                for v in (0, 1):
                    a, = t["qual/k%d/q%d/%s/%s" % (k, v, g, strand)]
                    n_, = t["qual/k%d/q%d/%s/n/%s" % (k, v, g, strand)]
                    b, = t["qual/k%d/q%d/%s/bothn/%s" % (k, v, g, strand)]
                    assert (a.XM, n_.XM, b.XM) == (k, k + 3, k) and b.mismatches == k + 1 and a.mismatches == k
                    # N against a base costs penalty_for_N and no quality, N against N costs it without counting as a mismatch
                    assert n_.AS == a.AS - 3 * p.bowtie2_penalty_for_N and b.AS == a.AS - p.bowtie2_penalty_for_N
                # the qualities are planted in genome orientation: both strands pay the same
                assert t["qual/k%d/q0/%s/sense" % (k, g)][0].AS - t["qual/k%d/q0/%s/anti" % (k, g)][0].AS == 0
    # what the planted bytes cost, from the formula (bwt_map.cpp:2570-2580) and the bytes alone
    lo, hi = p.bowtie2_min_penalty, p.bowtie2_max_penalty
    pen = lambda byte: lo + (hi - lo) * min(byte - 33, 40) // 40
    orders = ((33, 73, 34, 74, 35, 34, 126, 75, 33, 126, 35, 73), (126, 35, 75, 33, 74, 75, 34, 73, 126, 33, 74, 34))
    for k in (5, 6, 7, 12):
        for v in (0, 1):
            assert t["qual/k%d/q%d/plain/sense" % (k, v)][0].AS == -sum(pen(x) for x in orders[v][:k])
    assert pen(orders[0][5]) != pen(orders[0][6]) and pen(orders[1][5]) != pen(orders[1][6])       # sixth and seventh differ
    assert set(orders[0]) == set(me.QUAL_BYTES) == set(orders[1])


def test_quality_edges(monkeypatch):
    cases, wants = me.family("qualities"), me.expected("qualities")
    assert cases[0][2].bowtie2_max_penalty == 6 and cases[1][2].bowtie2_max_penalty == 42
    for case, want in zip(cases, wants):
        check_qualities(case, want)
        run_modes(case, want, monkeypatch, chains=True)
    # a point of penalty per phred: bytes 33, 34 and 35 cost 2, 3 and 4, and 74, 75 and 126 what 73 costs
    assert len({a.AS for a in wants[1]}) > len({a.AS for a in wants[0]})


# ------------------------------------------------------------------------------------------------ piece edges
def check_piece_edges(rl, want, tags):
    assert {a.read_idx for a in want} == set(range(len(tags)))
    t = by_tag(want, tags)
    offsets = [f for f in me.PIECE_OFFSETS if f < rl - 1] + [rl - 1]
    for strand in ("sense", "anti"):
        assert t["piece/rl%d/clean/%s" % (rl, strand)][0].MD == str(rl)
        for f in offsets:
            md = t["piece/rl%d/at%d/%s" % (rl, f, strand)][0].MD
            m = re.fullmatch(r"(\d+)[ACGT](\d+)", md)
            assert m and (int(m.group(1)), int(m.group(2))) == (f, rl - 1 - f), (f, md)
        for f in offsets:
            if f % 64 == 63 and f + 1 < rl:
                md = t["piece/rl%d/pair%d/%s" % (rl, f, strand)][0].MD
                assert re.fullmatch(r"%d[ACGT]0[ACGT]%d" % (f, rl - 2 - f), md), md
        pieces = {int(k.split("piece")[-1].split("/")[0]) for k in t if "spliced_in_piece" in k and k.endswith(strand)}
        assert pieces == {pos // 64 for pos in me.boundaries(rl, 32 if rl == 512 else 25, strand == "anti") if pos // 64 <= 4}
        for k, (a,) in t.items():
            if "spliced_in_piece" in k:
                assert spliced(a)
            if "deleted_in_piece" in k:
                assert "^" in a.MD and a.XO == 1
    if rl >= 250:
        assert {0, 1, 2, 3} <= pieces                               # the fourth piece: past the prefetched ones


@pytest.mark.parametrize("rl", me.PIECE_READ_LENGTHS)
def test_piece_edges(rl, monkeypatch):
    (case,), (want,) = me.family("piece%d" % rl), me.expected("piece%d" % rl)
    check_piece_edges(rl, want, case[5])
    run_modes(case, want, monkeypatch, chains=rl // 25 <= 4)


# ------------------------------------------------------------------------------------------------ multihit copies
def check_multihit(copies, want, tags):
    per_read = {}
    for a in want:
        per_read[a.read_idx] = per_read.get(a.read_idx, 0) + 1
    assert set(per_read) == set(range(len(tags))) and set(per_read.values()) == {copies}
    for anti in (False, True):
        lens = {len(a.MD) for a in want if a.antisense == anti}
        assert lens >= {23, 24, 25, 26, 39, 40, 41, 42}, sorted(lens)
    assert len({(a.read_idx, a.MD) for a in want}) > len(per_read)      # the copies of a read differ


@pytest.mark.parametrize("copies", [3, 12])
def test_multihit_copies(copies, monkeypatch):
    (case,), (want,) = me.family("multihit%d" % copies), me.expected("multihit%d" % copies)
    check_multihit(copies, want, case[5])
    run_modes(case, want, monkeypatch)


# ------------------------------------------------------------------------------------------------ the fusion tier's walk
@pytest.mark.parametrize("name", ["ladder"] + ["piece%d" % rl for rl in me.PIECE_READ_LENGTHS])
def test_fusion_walk_on_the_same_edges(name, monkeypatch):
    """--fusion-search with an empty fusion list: the plain records, built by the fusion tier's walk (f_sam_extra)"""
    import dataclasses
    import numpy as np
    import orc
    (case,) = me.family(name)
    seqs, sb, p, juncs, ins, tags = case
    pf = dataclasses.replace(p, fusion_search=1)
    none = np.zeros(0, dtype=orc.SPAN_FUSION_DTYPE)
    want = orc.spanning_fusion(pf, orc.Genome(seqs), sb, juncs, ins, none, True)
    assert want == list(me.expected(name)[0])
    if not os.path.exists(host.LIB_PATH):
        monkeypatch.setattr(host, "md_on_host", lambda *a, **k: HOST_MD)
        want = on_host(want)
    got, status = sim.spanning_fusion(pf, seqs, sb, juncs, ins, none, True)      # (tier 0 skipped: every read through the fusion tier)
    assert status[1] == 0 and status[2] == 0 and status[3] == sb.n_reads, status
    got.sort(key=lambda a: a.read_idx)
    assert got == want, me.explain(got, want, tags)
