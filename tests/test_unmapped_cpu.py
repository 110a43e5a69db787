"""CPU: the unmapped-read files and the align-summary counters -- the restatement (unmapped_ref.py: the reference's loop over the hit
streams and the read streams) against the hand-worked cases (unmapped_cases.py), and the product's core (thj_unmapped_core.h compiled
for the CPU, tests/unmappedsim: the closed form the kernels run) against both, byte for byte; the seeded crowds with their self-check;
the same program under the address and undefined-behaviour sanitizers; align_summary.txt's text."""
import os
import subprocess

import best_ref as br
import indelbed_ref as ir
import pair_ref as pr
import unmapped_cases as uc
import unmapped_ref as ur
from locked_make import locked_make

HERE = os.path.dirname(os.path.abspath(__file__))
SIMDIR = os.path.join(HERE, "unmappedsim")


def sim(name="unmappedsim"):
    locked_make(SIMDIR)
    return os.path.join(SIMDIR, name)


def n_best(S, idx, ctx):
    """what is left of a read at its best score, before the cap (read_best_alignments, :141-163)"""
    cand = [k for k in idx if ctx["live"][S["tag"]][k] and ir.kept(S["recs"][k], ctx["accepted"])]
    sc = {k: br.score(S["recs"][k], S["AS"][k], ctx["js1"], ctx["known"], ctx["best"][2]) for k in cand}
    top = max(sc.values(), default=None)
    return len(br.sort_unique([k for k in cand if sc[k] == top], S["recs"], S["mism"], S["anti"])[1])


def code_of(n, max_multihits, suppress):
    over = n > max_multihits
    left = (0 if suppress else max_multihits) if over else n
    return (1 if left > 0 else 0) | (4 if left > 1 else 0) | (16 if over else 0)


def sim_lines(c, L, R, ctx):
    """what the finish leaves on the device, as the sim takes it: the read codes and, per insert, what um::insert_word is given"""
    max_multihits, suppress, _mp = ctx["best"]
    out = ["C %d %d" % (1 if R is not None else 0, 1 if R is not None and ctx["pair"][3] else 0)]
    if R is None:
        for s, e in br.groups(L["reads"]):
            out.append("G %d 0 %d 0" % (c["numbers"][L["reads"][s]], code_of(n_best(L, list(range(s, e)), ctx), max_multihits, suppress)))
        return out
    mixed, discordant = ctx["pair"][3], ctx["pair"][4]
    for num, li, ri in pr.inserts(L, R):
        lid = [k for k in li if ctx["live"]["L"][k] and ir.kept(L["recs"][k], ctx["accepted"])]
        rid = [k for k in ri if ctx["live"]["R"][k] and ir.kept(R["recs"][k], ctx["accepted"])]
        gone_l, gone_r = any(not ctx["live"]["L"][k] for k in li), any(not ctx["live"]["R"][k] for k in ri)
        n_list, best_fusion, best_conc = 0, False, False
        if lid and rid:
            lsc = {k: br.score(L["recs"][k], L["AS"][k], ctx["js1"], ctx["known"], ctx["best"][2]) for k in lid}
            rsc = {k: br.score(R["recs"][k], R["AS"][k], ctx["js1"], ctx["known"], ctx["best"][2]) for k in rid}
            pr.TRACE = []
            hits, best_fusion, over = pr.pair_best(L, R, lid, rid, lsc, rsc, ctx["js1"], ctx["keys1"], ctx["pair"], ctx["best"], True, br.Mt19937(1))
            trace, pr.TRACE = pr.TRACE[-1], None
            n_list = max_multihits + 1 if over else len(hits)
            best_conc = ur.concordant(trace["cands"], ctx)
        v = [bool(li), bool(ri), bool(lid), bool(rid), gone_l, gone_r, n_list, best_fusion, best_conc, max_multihits, suppress, mixed, discordant]
        out.append("I %d %s %d %d" % (c["numbers"][num], " ".join(str(int(x)) for x in v), code_of(n_best(L, li, ctx), max_multihits, suppress) if li else 0,
                                      code_of(n_best(R, ri, ctx), max_multihits, suppress) if ri else 0))
    return out


def run_sim(exe, tmp_path, head, files):
    """files = [(side, [records with their block_size fields])] -> ({side: [records]}, counters) or ("L", text)"""
    lines = list(head)
    for side, recs in files:
        lines.append("S %d" % side)
        lines += ["R " + r[4:].hex() for r in recs]
    p = tmp_path / "sim.txt"
    p.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, "run", str(p)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    outs, stats = {0: [], 1: []}, None
    for ln in r.stdout.splitlines():
        if ln.startswith("L "):
            return "L", ln.split(" ", 2)[2]
        if ln.startswith("O "):
            _o, side, hx = ln.split()
            outs[int(side)].append(bytes.fromhex(hx))
        if ln.startswith("T "):
            stats = [int(x) for x in ln.split()[1:]]
    return outs, stats


def ref_single(c, best=None, file=None):
    return ur.walk(c, None, [r[4:] for r in (file or c["file"])], None, c["numbers"], best or c["best"], None, c["anchor"], c["known"], c["limits"])


def ref_paired(c, best=None, pair=None):
    return ur.walk(c["L"], c["R"], [r[4:] for r in c["left_file"]], [r[4:] for r in c["right_file"]], c["numbers"], best or c["best"], pair or c["pair"], c["anchor"], c["known"],
                   c["limits"], c["max_report_intron"])


def sim_single(exe, tmp_path, c, best=None, file=None):
    L, _R, ctx = ur.make_ctx(c, None, best or c["best"], None, c["anchor"], c["known"], c["limits"])
    return run_sim(exe, tmp_path, sim_lines(c, L, None, ctx), [(0, file or c["file"])])


def sim_paired(exe, tmp_path, c, best=None, pair=None):
    L, R, ctx = ur.make_ctx(c["L"], c["R"], best or c["best"], pair or c["pair"], c["anchor"], c["known"], c["limits"], c["max_report_intron"])
    return run_sim(exe, tmp_path, sim_lines(c, L, R, ctx), [(0, c["left_file"]), (1, c["right_file"])])


def by_number(file):
    return {int(r[36:36 + r[12] - 1]): r for r in file}


def test_record_shapes(tmp_path):
    cs = uc.shape_cases()
    for label, raw, want in cs:
        assert ur.write_unmapped_record(ur.QRead(raw[4:])) == want, label
    empty = dict(recs=[], reads=[], AS=[], mism=[], anti=[], numbers=[], known=[], limits=None, anchor=8, best=(20, False, 6))
    file = [raw for _l, raw, _w in cs]
    outs, stats = run_sim(sim(), tmp_path, sim_lines(empty, dict(empty, tag="L"), None, dict(best=empty["best"])), [(0, file)])
    assert outs[0] == [w for _l, _r, w in cs]
    assert stats == [0, len(cs)] + [0] * 13
    left, _right, rstats = ref_single(empty, file=file)
    assert left == outs[0] and rstats == stats


def test_single_end_outcomes(tmp_path):
    c = uc.single_case()
    recs = by_number(c["file"])
    for suppress, (written, stats) in c["want"].items():
        best = (2, suppress, 6)
        want = [ur.write_unmapped_record(ur.QRead(recs[k][4:])) for k in written]      # (the records' bytes are pinned by the shapes above)
        left, _r, got = ref_single(c, best)
        assert (left, got) == (want, stats), suppress
        outs, sstats = sim_single(sim(), tmp_path, c, best)
        assert (outs[0], sstats) == (want, stats), suppress


def test_paired_outcomes(tmp_path):
    c = uc.paired_case()
    lrec, rrec = by_number(c["left_file"]), by_number(c["right_file"])
    for (mixed, discordant, best), (lw, rw, stats) in c["want"].items():
        pair = c["pair"][:3] + (mixed, discordant)
        want_l = [ur.write_unmapped_record(ur.QRead(lrec[k][4:])) for k in lw]
        want_r = [ur.write_unmapped_record(ur.QRead(rrec[k][4:])) for k in rw]
        left, right, got = ref_paired(c, best, pair)
        assert (left, right, got) == (want_l, want_r, stats), (mixed, discordant, best)
        outs, sstats = sim_paired(sim(), tmp_path, c, best, pair)
        assert (outs[0], outs[1], sstats) == (want_l, want_r, stats), (mixed, discordant, best)


def test_insert_word_rows():
    """um::insert_word by hand: has_l has_r live_l live_r gone_l gone_r n_list best_fusion best_conc max_multihits suppress mixed discordant"""
    W = dict(HAS_L=1, HAS_R=2, PAIRED=4, ANY=8, MULTI=16, OVER=32, EMPTY=64, DISC=128, AMBIG=256, RL=512, RR=1024)
    rows = [
        ((1, 0, 1, 0, 0, 0, 0, 0, 0, 20, 0, 0, 0), W["HAS_L"] | W["RL"]),                                            # a left singleton
        ((0, 1, 0, 0, 0, 0, 0, 0, 0, 20, 0, 1, 0), W["HAS_R"] | W["RR"]),                                            # a right one with nothing live: still through write_singleton_alignments
        ((1, 1, 1, 1, 0, 0, 1, 0, 1, 20, 0, 0, 0), 3 | W["PAIRED"] | W["ANY"]),
        ((1, 1, 1, 1, 0, 0, 2, 0, 0, 20, 0, 0, 0), 3 | W["PAIRED"] | W["ANY"] | W["MULTI"] | W["DISC"]),
        ((1, 1, 1, 1, 0, 0, 3, 0, 1, 2, 0, 0, 0), 3 | W["PAIRED"] | W["ANY"] | W["MULTI"] | W["OVER"]),
        ((1, 1, 1, 1, 0, 0, 3, 0, 1, 2, 1, 0, 0), 3 | W["PAIRED"] | W["ANY"] | W["MULTI"] | W["OVER"] | W["EMPTY"]),
        ((1, 1, 1, 1, 0, 0, 3, 0, 1, 2, 1, 1, 0), 3 | W["RL"] | W["RR"]),                                            # mixed: the emptied list gives the pairs up
        ((1, 1, 1, 1, 0, 0, 0, 1, 0, 20, 0, 0, 0), 3 | W["PAIRED"] | W["EMPTY"]),                                    # every candidate a skipped fusion pair
        ((1, 1, 1, 1, 0, 0, 1, 1, 0, 20, 0, 1, 0), 3 | W["DISC"] | W["RL"] | W["RR"]),                               # mixed, a fusion best grade: counted discordant, then the sides
        ((1, 1, 1, 1, 0, 0, 1, 1, 0, 20, 0, 1, 1), 3 | W["PAIRED"] | W["ANY"] | W["DISC"]),
        ((1, 1, 1, 0, 0, 0, 0, 0, 0, 20, 0, 0, 0), 3 | W["RL"]),                                                     # the right group is empty after the exclusion: :2581-2584
        ((1, 1, 1, 0, 0, 1, 0, 0, 0, 20, 0, 0, 0), 3 | W["AMBIG"] | W["PAIRED"] | W["EMPTY"]),                       # only records over the limits there
        ((1, 1, 0, 0, 0, 0, 0, 0, 0, 20, 0, 1, 0), 3),
    ]
    exe = sim()
    for args, want in rows:
        r = subprocess.run([exe, "word"] + [str(x) for x in args], capture_output=True, text=True)
        assert r.returncode == 0 and int(r.stdout) == want, (args, int(r.stdout), want)
    for n, cap, sup, want in ((0, 2, 0, 0), (1, 2, 0, 1), (2, 2, 0, 5), (3, 2, 0, 21), (3, 2, 1, 16), (2, 1, 0, 17)):
        r = subprocess.run([exe, "code", str(n), str(cap), str(sup)], capture_output=True, text=True)
        assert int(r.stdout) == want, (n, cap, sup)


def test_loud_cases(tmp_path):
    for label, file, text in uc.loud_cases():
        got = run_sim(sim(), tmp_path, ["C 0 0"], [(0, file)])
        assert got[0] == "L" and text in got[1], (label, got)
    # a read without mate bits on an insert one of whose sides has only records over the limits left
    got = run_sim(sim(), tmp_path, ["C 1 0", "I 7 1 1 1 0 0 1 0 0 0 20 0 0 0 1 0"], [(0, [uc.rd(7, flag=4)])])
    assert got[0] == "L" and "not built" in got[1], got
    outs, stats = run_sim(sim(), tmp_path, ["C 1 0", "I 7 1 1 1 0 0 1 0 0 0 20 0 0 0 1 0"], [(0, [uc.rd(7, flag=0x45)])])      # with mate bits: the same answer either way
    assert len(outs[0]) == 1 and stats[uc.UM_L] == 1 and sum(stats) == 1


SINGLE_CLASSES = ("no_group_unmapped", "no_group_ZT_M", "read_aligned", "read_multi", "read_over_the_cap", "read_nothing_left")
PAIRED_CLASSES = ("no_group_unmapped", "no_group_ZT_M", "pairs_one", "pairs_multi", "pairs_over_the_cap", "pairs_none", "discordant_pair", "alone_without_mixed")
MIXED_CLASSES = ("mixed_gives_up_the_pairs", "read_aligned", "read_multi", "pairs_one", "side_empty_after_exclusion")


def check_classes(seen, classes, crowd_size):
    for k in classes:
        assert seen.get(k, 0) > 0, (k, seen)
    assert max(seen.values()) <= crowd_size // 2, seen


def test_single_crowd(tmp_path):
    c = uc.single_crowd()
    ur.SEEN = {}
    try:
        left, _r, stats = ref_single(c)
        seen = dict(ur.SEEN)
        ur.SEEN = {}
        left_s, _r, stats_s = ref_single(c, best=(2, True, 6))
        assert ur.SEEN.get("read_over_the_cap_suppressed", 0) > 0
    finally:
        ur.SEEN = None
    check_classes(seen, SINGLE_CLASSES, len(c["file"]))
    for best, (wl, ws) in (((2, False, 6), (left, stats)), ((2, True, 6), (left_s, stats_s))):
        outs, sstats = sim_single(sim(), tmp_path, c, best)
        assert outs[0] == wl and sstats == ws, best
    assert 0 < len(left) < len(c["file"]) and len(left_s) > len(left)


def test_paired_crowd(tmp_path):
    c = uc.paired_crowd()
    n = len(c["left_file"]) + len(c["right_file"])
    for pair, best, classes in (((200, 20, 10000000, False, False), (2, False, 6), PAIRED_CLASSES), ((200, 20, 10000000, True, False), (2, False, 6), MIXED_CLASSES),
                                ((200, 20, 900, False, True), (2, True, 6), ("pairs_suppressed", "discordant_pair")), ((150, 30, 10000000, True, True), (1, True, 5), ("read_over_the_cap_suppressed",))):
        ur.SEEN = {}
        try:
            left, right, stats = ref_paired(c, best, pair)
            seen = dict(ur.SEEN)
        finally:
            ur.SEEN = None
        check_classes(seen, classes, n)
        outs, sstats = sim_paired(sim(), tmp_path, c, best, pair)
        assert (outs[0], outs[1], sstats) == (left, right, stats), (pair, best)
    # reads without mate bits: the unpaired counters fill
    c = uc.paired_crowd(mate_bits=False)
    ur.SEEN = {}
    try:
        left, right, stats = ref_paired(c, (2, False, 6), (200, 20, 10000000, True, False))
        assert ur.SEEN.get("matenum0_in_a_paired_run", 0) > 0
    finally:
        ur.SEEN = None
    assert stats[uc.AL_U] > 0 and stats[uc.UM_U] > 0
    outs, sstats = sim_paired(sim(), tmp_path, c, (2, False, 6), (200, 20, 10000000, True, False))
    assert (outs[0], outs[1], sstats) == (left, right, stats)


def test_sanitized_program(tmp_path):
    """the same core under -fsanitize=address,undefined, run as a program of its own: the shapes, the loud records, a crowd"""
    exe = sim("unmappedsim_san")
    cs = uc.shape_cases()
    outs, _stats = run_sim(exe, tmp_path, ["C 0 0"], [(0, [raw for _l, raw, _w in cs])])
    assert outs[0] == [w for _l, _r, w in cs]
    for label, file, text in uc.loud_cases():
        got = run_sim(exe, tmp_path, ["C 0 0"], [(0, file)])
        assert got[0] == "L" and text in got[1], label
    c = uc.paired_crowd(n_inserts=120)
    left, right, stats = ref_paired(c, (2, False, 6), (200, 20, 10000000, True, False))
    outs, sstats = sim_paired(exe, tmp_path, c, (2, False, 6), (200, 20, 10000000, True, False))
    assert (outs[0], outs[1], sstats) == (left, right, stats)


def test_align_summary_text():
    """print_alnStats' text by hand"""
    s = [0] * 15
    s[uc.AL_L], s[uc.UM_L], s[uc.MULTI_L], s[uc.XMULTI_L] = 3, 4, 2, 2
    assert ur.align_summary(s, 2) == ("Reads:\n          Input     :         7\n           Mapped   :         3 (42.9% of input)\n"
                                      "            of these:         2 (66.7%) have multiple alignments (2 have >2)\n42.9% overall read mapping rate.\n")
    assert ur.align_summary([0] * 15, 20) == "Reads:\n          Input     :         0\n           Mapped   :         0 (-nan% of input)\n-nan% overall read mapping rate.\n"
    p = uc.paired_case()["want"][(False, False, (20, False, 6))][2]
    assert ur.align_summary(p, 20) == (
        "Left reads:\n          Input     :         7\n           Mapped   :         4 (57.1% of input)\n            of these:         1 (25.0%) have multiple alignments (1 have >20)\n"
        "Right reads:\n          Input     :         6\n           Mapped   :         4 (66.7% of input)\n            of these:         1 (25.0%) have multiple alignments (0 have >20)\n"
        "Unpaired reads:\n          Input     :         2\n           Mapped   :         0 ( 0.0% of input)\n"
        "53.3% overall read mapping rate.\n\nAligned pairs:         4\n     of these:         1 (25.0%) have multiple alignments\n"
        "                       1 (25.0%) are discordant alignments\n50.0% concordant pair alignment rate.\n")
