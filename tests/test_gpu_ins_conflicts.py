"""GPU: which read wins a contested insertion of stage 1 -- the planted contests of tests/ins_conflicts.py through the kernels, the
table growth, the merge of two contexts, the exchange step, stage 2's sets and the executable.  Every result is compared with the
oracle's events bit for bit (its insertions are numbered by a counter in visiting order; batch.merge_events keeps the earlier
batch's), and every contest's place must carry the letters of the contender visited first."""
import os
import subprocess
import threading

import pytest

import ins_conflicts as ic
import orc
from tophat_amd import host
from tophat_amd.batch import events_to_span_inputs, merge_events
from util import assert_events_equal

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tophat_amd", "bin")


@pytest.fixture(scope="module")
def lib():
    return host.load_lib()   # fails loudly when the extension is missing


def _ctx(sc):
    ctx = host.Context(0)
    ctx.upload_genome(host.pack_genome(sc.seqs))
    return ctx


def _runs(ctx, sc, order):
    return [(sc.params(bi), ctx.upload_batch(sc.batches[bi].sb, ordinal_base=sc.batches[bi].ordinal_base)) for bi in order]


def _check(sc, got, want, what):
    assert_events_equal(got, want, "%s %s" % (sc.name, what))
    ic.assert_first_wins(sc, got, what)


@pytest.mark.parametrize("name", ["paths", "wide50", "wide64", "long"])
def test_one_batch(lib, name):
    """every kind of contest in one batch.  The counters show the indel pairs and the un-queued workgroups; which kernel a read takes is
    decided by its hits alone (one a segment: thj_k_sj_flat -> thj_k_sj_tasks; up to 8, up to 32, more: thj_k_sj_general's two
    instances, thj_k_segjuncs_shared) -- the planted reads have 4, 5, 8, 10, 12, 14, 24, 26 and 44"""
    sc, want = ic.scenario(name), ic.expected(name)
    assert len(sc.contests) >= sc.min_contests
    with _ctx(sc) as ctx:
        got = ctx.segjuncs(_runs(ctx, sc, sc.order()))
    print(name, "contests", len(sc.contests), {k: got.stats[k] for k in ("windows", "indel_pairs", "overflow_blocks", "hits_read")})
    _check(sc, got, want, "one batch")
    assert got.stats["indel_pairs"] == want.stats["indel_pairs"] and got.stats["windows"] == want.stats["windows"]
    assert got.stats["hits_read"] == len(sc.batches[0].sb.hits)
    if name == "paths":
        assert got.stats["overflow_blocks"] >= 1
        per_read = [int(n) for n in (sc.batches[0].sb.seg_off[4::4] - sc.batches[0].sb.seg_off[:-1:4])]
        assert {4, 5, 8, 10, 12, 14, 24, 26, 44} <= set(per_read)


def test_left_before_right(lib):
    """a right read at a low row of its batch against a left read at a high row of its own, as the executable and the benchmark run a
    pass (thj_segjuncs_run_async a side, and both sides as one thj_segjuncs_run_pair_async call): the left read wins"""
    sc, want = ic.scenario("sides"), ic.expected("sides")
    assert sum(1 for c in sc.contests if c.note.startswith("right-low/left-high")) >= 8
    with _ctx(sc) as ctx:
        runs = _runs(ctx, sc, sc.order())
        _check(sc, ctx.segjuncs(runs), want, "left, right")
        for a, b in ((0, 1), (1, 0)):
            ctx.reset()
            ctx.run_pair(runs[a][0], runs[a][1], runs[b][0], runs[b][1])
            _check(sc, ctx.download(ctx.finish()), want, "pair call %d%d" % (a, b))


def test_successive_batches_and_their_launch_order(lib):
    """three batches of one context with ordinal_base running on, launched in every order: the ordinal decides, not the launch"""
    sc, want = ic.scenario("shards"), ic.expected("shards")
    with _ctx(sc) as ctx:
        runs = _runs(ctx, sc, sc.order())
        for order in ((0, 1, 2), (2, 1, 0), (1, 2, 0), (2, 0, 1)):
            _check(sc, ctx.segjuncs([runs[i] for i in order]), want, "launch order %s" % (order,))


def test_across_table_growth(lib):
    """tables of 1 024 slots (the least): the batch between the contenders' holds some 570 insertions, so the insertion table passes 40 % and is
    rehashed into a larger one before the last batch or when the pass ends (thj_k_rehash_ins) -- the first contender's priority must
    come through"""
    sc, want = ic.scenario("growth"), ic.expected("growth")
    first = orc.segjuncs(sc.params(0), orc.Genome(sc.seqs), sc.batches[0].sb)
    assert len(first.insertions) * 5 < 1024 * 2 < len(want.insertions) * 5
    with _ctx(sc) as ctx:
        ctx.configure(64, 16)
        runs = _runs(ctx, sc, sc.order())
        _check(sc, ctx.segjuncs(runs), want, "growth")
        _check(sc, ctx.segjuncs(runs[::-1]), want, "growth, launched backwards")      # (the tables are large now: nothing grows)
        ctx.configure(64, 16)
        ctx.reset()
        for p, h in runs:                  # every batch's counters have arrived when the next one starts: the table grows between batches
            ctx.run(p, h)
            ctx.sync()
        _check(sc, ctx.download(ctx.finish()), want, "growth between batches")


def test_overflowing_batch_is_run_again(lib):
    """the second contender's own batch brings 1 350 insertions: the 1 024 slots run full, the pass says so, and the same batches on
    larger tables give the oracle's events -- the first contender's letters at every contest"""
    sc, want = ic.scenario("replay"), ic.expected("replay")
    assert len(want.insertions) > 1024
    with _ctx(sc) as ctx:
        ctx.configure(64, 16)
        runs = _runs(ctx, sc, sc.order())
        with pytest.raises(host.ThjError, match="event table overflow"):
            ctx.segjuncs(runs)
        ctx.configure(8192, 8192)
        _check(sc, ctx.segjuncs(runs), want, "run again")
        _check(sc, ctx.segjuncs(runs[::-1]), want, "run again, launched backwards")


def _rank_runs(ctxs, sc):
    out = [[], []]
    for bi in sc.order():
        b = sc.batches[bi]
        out[b.rank].append((sc.params(bi), ctxs[b.rank].upload_batch(b.sb, ordinal_base=b.ordinal_base)))
    return out


def test_merge_of_two_contexts(lib):
    """a paired run sharded by read id over two contexts (test_gpu_merge.py's steps): each folds the other's sorted keys and insertion
    values in, both end with the single-context result.  A right read on context 0 meets a left read on context 1: the left read
    wins on both, although it lives on the higher rank"""
    sc, want = ic.scenario("ranks"), ic.expected("ranks")
    assert sum(1 for c in sc.contests if c.note.startswith("right on rank 0/left on rank 1")) >= 8
    with _ctx(sc) as one:
        _check(sc, one.segjuncs(_runs(one, sc, sc.order())), want, "one context")
    with _ctx(sc) as a, _ctx(sc) as b:
        ctxs = (a, b)
        runs = _rank_runs(ctxs, sc)
        local = []
        for ctx, mine in zip(ctxs, runs):
            ctx.reset()
            for p, h in mine:
                ctx.run(p, h)
            local.append(ctx.finish())
        assert all(0 < c.n_insertions < len(want.insertions) for c in local)
        state = []
        for ctx in ctxs:
            ctx.sync()
            state.append((ctx.device_keys(0), ctx.device_keys(1), ctx.device_insertions()))
        for me, other in ((0, 1), (1, 0)):
            (jp, jn), (dp, dn), (ik, iv, inn) = state[other]
            ctxs[me].merge_keys(0, jp, jn)
            ctxs[me].merge_keys(1, dp, dn)
            ctxs[me].merge_insertions(ik, iv, inn)
        for ctx in ctxs:
            ctx.sync()
        for r, ctx in enumerate(ctxs):
            _check(sc, ctx.download(ctx.finish()), want, "context %d after the merge" % r)


def _in_threads(fns):
    err = []

    def wrap(f):
        try:
            f()
        except BaseException as e:      # noqa: BLE001
            err.append(e)
    th = [threading.Thread(target=wrap, args=(f,)) for f in fns]
    for t in th:
        t.start()
    for t in th:
        t.join(300)
    assert not any(t.is_alive() for t in th), "a rank hung in the exchange step"
    if err:
        raise err[0]


@pytest.mark.parametrize("caps", [None, "4,2,2"], ids=["plain", "tiny_sections"])
def test_exchange_step(lib, caps, monkeypatch):
    """the same contests through thj_events_allgather_async (two contexts, the loopback transport, two passes as test_gpu_comm.py runs
    them); with message sections of 4 / 2 / 2 keys the insertion section repeats"""
    sc, want = ic.scenario("ranks"), ic.expected("ranks")
    if caps:
        monkeypatch.setenv("THJ_XCHG_CAPS", caps)
    got, info = [None, None], [None, None]
    with _ctx(sc) as a, _ctx(sc) as b:
        ctxs = (a, b)
        runs = _rank_runs(ctxs, sc)
        comms = host.Comm.create_local(ctxs)

        def rank(r):
            def go():
                for _ in range(2):
                    ctxs[r].reset()
                    for p, h in runs[r]:
                        ctxs[r].run(p, h)
                    comms[r].events_allgather()
                    got[r] = ctxs[r].download(ctxs[r].finish())
                info[r] = comms[r].info()
            return go
        _in_threads([rank(0), rank(1)])
        for c in comms:
            c.close()
    for r in (0, 1):
        _check(sc, got[r], want, "rank %d" % r)
    if caps:
        assert info[0]["repeats"] >= 1 and info[0]["repeats"] == info[1]["repeats"]
    else:
        assert info[0]["repeats"] == 0


def test_ordinal_range(lib):
    """a batch whose ordinals end just below 2^29 against a batch at ordinal 0: the low one wins; a batch that would reach 2^29 is refused"""
    sc, want = ic.scenario("range"), ic.expected("range")
    hi = max(range(len(sc.batches)), key=lambda i: sc.batches[i].ordinal_base)
    n = sc.batches[hi].n_reads
    assert sc.batches[hi].ordinal_base == (1 << 29) - n - 1
    with _ctx(sc) as ctx:
        runs = _runs(ctx, sc, sc.order())
        _check(sc, ctx.segjuncs(runs), want, "top of the range")
        _check(sc, ctx.segjuncs(runs[::-1]), want, "top of the range, launched backwards")
        h = ctx.upload_batch(sc.batches[hi].sb, ordinal_base=(1 << 29) - n)
        ctx.reset()
        with pytest.raises(host.ThjError, match=r"batch too large: read ordinals must stay below 2\^29"):
            ctx.run(sc.params(hi), h)


def test_into_stage_2(lib):
    """thj_span_sets_from_segjuncs after a contested stage 1, then the contenders' own batches stitched: the oracle's spanning records
    from the oracle's stage-1 events.  A loser's alignment does not show mismatches against the winner's letters: long_spanning_reads
    joins two segments through an insertion of its set only where the read's bases equal the set's letters
    (long_spanning_reads.cpp:1010-1306), so a loser has NO alignment through the insertion -- with its own letters in the set it
    would have one.  Every loser without N is checked for exactly that (ins_conflicts.check_stage2)."""
    sc, want = ic.scenario("stitch"), ic.expected("stitch")
    g = orc.Genome(sc.seqs)
    jj, ii = events_to_span_inputs(want)
    sbs = [ic.span_batch(sc, bi) for bi in sc.order()]
    p = sc.params(0)
    want_recs = [orc.spanning(p, g, sb, jj, ii) for sb in sbs]
    with _ctx(sc) as ctx:
        ev = ctx.segjuncs(_runs(ctx, sc, sc.order()))
        _check(sc, ev, want, "stage 1")
        ctx.span_sets_from_segjuncs()
        got_recs = [ctx.spanning(p, [ctx.upload_span_batch(sb)]) for sb in sbs]
    assert got_recs == want_recs and all(len(w) > 300 for w in want_recs)
    n_losers = ic.check_stage2(sc, sbs, got_recs, p, g, jj, ii)
    assert n_losers >= 8


def test_the_executable(lib, tmp_path):
    """a paired scenario as files through segment_juncs: one shard and one worker; five shards, three workers and batches of 200
    reads; eight contexts and sixteen shards with the exchange step -- segment.insertions byte for byte the same, equal to the
    oracle's file, the first contender's letters on every contest's line"""
    import pathlib
    from golden_util import events_text
    from tophat_amd.batch import build_seg_batch
    from tophat_amd.samtext import parse_sam_hits, read_fastq
    sc = ic.scenario("sides")
    d = str(tmp_path / "case")
    paths, names = ic.write_files(sc, d)
    ref_ids = {n: i + 1 for i, n in enumerate(names)}
    sides = {sd: dict(reads=read_fastq(paths["%s_fq" % sd]), segs=[list(parse_sam_hits(f, ref_ids, 500000)) for f in paths["%s_segs" % sd]]) for sd in ("left", "right")}
    og = orc.Genome(sc.seqs)
    want = None
    for sd, bi, other in (("left", 0, "right"), ("right", 1, "left")):
        b = build_seg_batch(sides[sd]["segs"], sides[sd]["reads"], [], sides[other]["segs"][-1])
        assert b.n_reads == sc.batches[bi].n_reads
        e = orc.segjuncs(sc.params(bi), og, b)
        want = e if want is None else merge_events(want, e)
    ic.assert_first_wins(sc, want, "oracle on the files")
    wt = events_text(want, names, pathlib.Path(d))
    texts = {}
    for tag, env in (("one", {"THJ_SHARDS": "1", "THJ_WORKERS": "1"}), ("many", {"THJ_SHARDS": "5", "THJ_WORKERS": "3", "THJ_BATCH_READS": "200"}),
                     ("ctx8", {"THJ_CTX_PER_GPU": "8", "THJ_SHARDS": "16"})):
        out = {k: str(tmp_path / ("%s.%s" % (tag, k))) for k in ("juncs", "insertions", "deletions", "fusions")}
        cmd = [os.path.join(BIN, "segment_juncs"), "--no-coverage-search", "--no-microexon-search", "--segment-length", str(sc.L), "--sam-header", paths["hdr"],
               paths["ref"], out["juncs"], out["insertions"], out["deletions"], out["fusions"],
               paths["left_fq"], paths["left_map"], ",".join(paths["left_segs"]), paths["right_fq"], paths["right_map"], ",".join(paths["right_segs"])]
        r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, **env))
        assert r.returncode == 0, r.stderr[-2000:]
        texts[tag] = {k: open(out[k]).read() for k in ("juncs", "insertions", "deletions")}
        for k in ("insertions", "deletions", "juncs"):
            assert texts[tag][k] == wt[k], (tag, k)
        lines = set(texts[tag]["insertions"].splitlines())
        for c in sc.contests:
            assert "%s\t%d\t%d\t%s" % (names[c.key[0] - 1], c.key[1], c.key[1], c.winner) in lines, (tag, c)
    assert texts["one"] == texts["many"] == texts["ctx8"]
