"""GPU: the planted reads of tests/md_edges.py (test_md_edges_cpu.py shows on the oracle's records that each family reaches its edge)
through the stitch kernels against the oracle -- contig_finish, joined_extras (chain entries -> join -> finish), sam_extra (packed
and lean tiers) and, with --fusion-search, f_sam_extra -- and the record slots reused by passes of different batches: a record that
needs no tail line written over one that did, a read without a record over one that had one, for the download (device and host
compaction) and for the resident consumers (the junction, insertion and deletion consensus)."""
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest

import indelbed_ref as ir
import md_edges as me
import orc
from tophat_amd import host

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_FUSIONS = np.zeros(0, dtype=host.SPAN_FUSION_DTYPE)


def gpu_records(ctx, case):
    seqs, sb, p, juncs, ins, tags = case
    ctx.upload_genome(host.pack_genome(seqs))
    ctx.upload_span_sets(juncs, ins)
    return ctx.spanning(p, [ctx.upload_span_batch(sb)])


def check(got, want, tags, what=""):
    assert got == list(want), "%s%s" % (what, me.explain(got, list(want), tags))


def test_gpu_md_length_ladder():
    (case,), (want,) = me.family("ladder"), me.expected("ladder")
    with host.Context(0) as ctx:
        got = gpu_records(ctx, case)
        chains = ctx.span_chain_count()
    assert chains > 0                                   # the spliced half: thj_k_chains / tier 0 -> join -> finish
    check(got, want, case[5])
    assert {len(a.MD) for a in got} >= set(range(3, 45))


def test_gpu_word_offset_sweep():
    cases, wants = me.family("sweep"), me.expected("sweep")
    with host.Context(0) as ctx:
        for case, want in zip(cases, wants):
            check(gpu_records(ctx, case), want, case[5], "%d segments: " % case[1].nseg)


def test_gpu_deletions_and_insertions():
    (case,), (want,) = me.family("indels"), me.expected("indels")
    with host.Context(0) as ctx:
        got = gpu_records(ctx, case)
        chains = ctx.span_chain_count()
    assert chains > 0
    check(got, want, case[5])
    assert any("^" in a.MD for a in got) and any(a.XO and "^" not in a.MD for a in got)


def test_gpu_quality_edges():
    cases, wants = me.family("qualities"), me.expected("qualities")
    with host.Context(0) as ctx:
        for case, want in zip(cases, wants):
            got = gpu_records(ctx, case)
            assert ctx.span_chain_count() > 0
            check(got, want, case[5], "max penalty %d: " % case[2].bowtie2_max_penalty)
    assert {a.XM for a in wants[0]} >= {5, 6, 7, 12}


@pytest.mark.parametrize("rl", me.PIECE_READ_LENGTHS)
def test_gpu_piece_edges(rl):
    """(250, 257 and 512 bases are batches of their own: the wide instances of the kernels)"""
    (case,), (want,) = me.family("piece%d" % rl), me.expected("piece%d" % rl)
    with host.Context(0) as ctx:
        got = gpu_records(ctx, case)
        chains = ctx.span_chain_count()
    if rl == 100:
        assert chains > 0                               # four segments: the spliced and deleted reads travel as chain entries
    check(got, want, case[5])


@pytest.mark.parametrize("copies", [3, 12])
def test_gpu_multihit_copies(copies):
    (case,), (want,) = me.family("multihit%d" % copies), me.expected("multihit%d" % copies)
    with host.Context(0) as ctx:
        got = gpu_records(ctx, case)
        groups, tiers = ctx.span_chain_groups(), ctx.span_tier_counts()
    if copies == 3:
        assert groups > 0, (groups, tiers)              # the multihit reads' chains as chain entries (thj_k_chains)
    else:
        assert tiers[1] > 0, tiers                      # reads to the packed multihit kernel
    check(got, want, case[5])


def test_gpu_fusion_walk_on_the_same_edges():
    """--fusion-search with an empty fusion list: the records are the plain ones, built by the fusion tier's walk (f_sam_extra)"""
    names = ["ladder"] + ["piece%d" % rl for rl in me.PIECE_READ_LENGTHS]
    with host.Context(0) as ctx:
        for name in names:
            (case,) = me.family(name)
            seqs, sb, p, juncs, ins, tags = case
            pf = dataclasses.replace(p, fusion_search=1)
            want = orc.spanning_fusion(pf, orc.Genome(seqs), sb, juncs, ins, np.zeros(0, dtype=orc.SPAN_FUSION_DTYPE), True)
            assert want == list(me.expected(name)[0]), name          # no fusion to find: what the plain walk gives
            ctx.upload_genome(host.pack_genome(seqs))
            ctx.upload_span_sets(juncs, ins)
            ctx.upload_span_fusions(NO_FUSIONS)
            check(ctx.spanning(pf, [ctx.upload_span_batch(sb)]), want, tags, name + ": ")


# ------------------------------------------------------------------------------------------------ slots reused by another batch
N_SLOT_READS = 48


def slot_batches():
    """three batches of N_SLOT_READS reads over one genome.  A: every record needs the slot's tail line (MD of 25..40 characters,
    5 and 7 cigar ops) or leaves its MD to the host (255).  B: every other read has a record that fits the lead line (MD of 24
    or fewer, 4 ops or fewer: plain, one intron, one deletion, one insertion), the others have none (their junction is not in the set).
    C: 5 and 7 ops again, at other places of the genome: junctions in ops 4 and up."""
    lad = me.ladder_patterns(1)
    A, B, C = [], [], []
    for i in range(N_SLOT_READS):
        anti = bool((i // 2) & 1)
        kind = i % 6
        if kind == 0:
            A.append(me.Read("slotA/md%d" % (25 + i % 16), anti=anti, subs=lad[25 + i % 16][0]))
        elif kind == 1:
            A.append(me.Read("slotA/md_on_host", anti=anti, subs=lad[41 + i % 4][0], gaps=((2, "N", 90, anti),) if i % 4 < 2 else ()))
        elif kind == 2:
            A.append(me.Read("slotA/7ops", anti=anti, subs=(3, 60), gaps=((1, "N", 70 + i, 0), (2, "N", 120, 0), (3, "N", 95, 0))))
        elif kind == 3:
            A.append(me.Read("slotA/7ops_del", anti=anti, subs=(24, 25), gaps=((1, "N", 80, 1), (2, "D", 3), (3, "N", 101 + i, 1))))
        elif kind == 4:
            A.append(me.Read("slotA/5ops", anti=anti, subs=lad[30][0], gaps=((1, "N", 66, anti), (3, "N", 140 + i, anti))))
        else:
            A.append(me.Read("slotA/5ops_ins", anti=anti, subs=(49, 52), gaps=((1, "N", 75, 0), (2, "I", 2))))
        if i % 2:
            B.append(me.Read("slotB/none", anti=anti, subs=(5,), gaps=((2, "N", 85, 0),), hide=True))
        else:
            k = (i // 2) % 6
            B.append([me.Read("slotB/plain_md3", anti=anti),
                      me.Read("slotB/plain_md24", anti=anti, subs=lad[24][0]),
                      me.Read("slotB/intron", anti=anti, subs=(7, 70), gaps=((2, "N", 110 + i, anti),)),
                      me.Read("slotB/deletion", anti=anti, subs=(24,), gaps=((1, "D", 2),)),
                      me.Read("slotB/insertion", anti=anti, subs=(80,), gaps=((3, "i", 3),)),
                      me.Read("slotB/two_introns_no", anti=anti, gaps=((1, "N", 60, 0), (3, "N", 61, 0)), hide=True)][k])
        C.append(me.Read("slotC/7ops" if i % 2 else "slotC/5ops", anti=anti, subs=(i,),
                         gaps=((1, "N", 200 + i, i & 1), (2, "N", 150, i & 1), (3, "N", 77, i & 1)) if i % 2 else ((2, "N", 64 + i, 0), (3, "N", 300, 0))))
    return me.build([A, B, C], seed=707)


def raw_pass(ctx, p, batch, sb, seqs):
    """one pass -> (the API records as downloaded, the Aln list)"""
    for _attempt in range(4):
        ctx.span_reset()
        ctx.span_run(p, batch)
        try:
            n = ctx.span_finish()
            break
        except host.ThjError as e:
            if "(-7)" not in str(e):
                raise
    raw = ctx.span_download(n)
    return raw, host.alns_from_array(raw, host.span_md_resolver(seqs, [sb], ctx.lib))


def unused_fields_are_zero(raw):
    """thj_aln: cigar ops past n_cigar and MD characters past md_len read as zero (md_len 255: the string is the host's)"""
    b = raw.view(np.uint8).reshape(-1, 128)
    for k in range(len(raw)):
        nc, ml = int(raw["n_cigar"][k]), int(raw["md_len"][k])
        fused = any((int(c) >> 28) in (7, 8, 9, 10) for c in raw["cigar"][k][:nc])
        assert not raw["cigar"][k][nc:15 if fused else 16].any(), ("cigar", k, raw["cigar"][k])
        if ml != host.MD_ON_HOST:
            assert not b[k, 88 + ml:128].any(), ("md", k, bytes(b[k, 88:128]))


def slot_expected():
    """the three batches and the oracle's records of each; the batches are what they are meant to be"""
    seqs, (sbA, sbB, sbC), p, juncs, ins, (tA, tB, tC) = slot_batches()
    g = orc.Genome(seqs)
    wA, wB, wC = (orc.spanning(p, g, sb, juncs, ins) for sb in (sbA, sbB, sbC))
    # the batches are what they are meant to be
    assert {a.read_idx for a in wA} == set(range(N_SLOT_READS))
    assert all(len(a.cigar) > 4 or len(a.MD) > 24 for a in wA) and any(len(a.MD) > 40 for a in wA) and {len(a.cigar) for a in wA} >= {1, 3, 5, 7}
    assert {a.read_idx for a in wB} == {i for i in range(N_SLOT_READS) if i % 2 == 0 and (i // 2) % 6 != 5}
    assert all(len(a.cigar) <= 4 and len(a.MD) <= 24 for a in wB) and {len(a.cigar) for a in wB} == {1, 3}
    assert {a.read_idx for a in wC} == set(range(N_SLOT_READS)) and {len(a.cigar) for a in wC} == {5, 7}
    return seqs, (sbA, sbB, sbC), p, juncs, ins, (tA, tB, tC), (wA, wB, wC)


def slot_sequence(ctx, consumers=True):
    seqs, (sbA, sbB, sbC), p, juncs, ins, (tA, tB, tC), (wA, wB, wC) = slot_expected()
    ctx.upload_genome(host.pack_genome(seqs))
    ctx.upload_span_sets(juncs, ins)
    hA, hB, hC = (ctx.upload_span_batch(sb) for sb in (sbA, sbB, sbC))
    for rnd in (0, 1):
        raw, got = raw_pass(ctx, p, hA, sbA, seqs)
        check(got, wA, tA, "A, round %d: " % rnd)
        unused_fields_are_zero(raw)
        raw, got = raw_pass(ctx, p, hB, sbB, seqs)
        check(got, wB, tB, "B over A, round %d: " % rnd)
        unused_fields_are_zero(raw)
    if not consumers:
        return len(wA), len(wB)
    # the resident consumers see B's records alone: none of A's junctions and indels, in the slots B left and in the tails B did not touch
    want_j = orc.junction_consensus(orc.jrecs_from_alns(wB))
    ctx.juncbed_reset()
    ctx.juncbed_add_span()
    js = ctx.juncbed_finish(8)
    assert ir.junc_rows(js) == ir.junc_rows(want_j) and len(want_j) >= 3
    want3 = consensus_of(wB, sbB)
    assert len(want3[1]) >= 2 and len(want3[2]) >= 2
    ctx.juncbed_reset()
    ctx.juncbed_collect_indels(True)
    ctx.juncbed_add_span_seq(hB)
    js = ctx.juncbed_finish(8)
    i1, d1 = ctx.juncbed_indels()
    assert (ir.junc_rows(js), ir.ins_rows(i1), ir.del_rows(d1)) == want3
    # C after B: cigar ops 4.. (JbCigar's tail indexing) over tails that hold A's junctions
    raw, got = raw_pass(ctx, p, hC, sbC, seqs)
    check(got, wC, tC, "C over B over A: ")
    unused_fields_are_zero(raw)
    want3 = consensus_of(wC, sbC)
    assert len(want3[0]) >= N_SLOT_READS
    ctx.juncbed_reset()
    ctx.juncbed_add_span()
    assert ir.junc_rows(ctx.juncbed_finish(8)) == want3[0]
    ctx.juncbed_reset()
    ctx.juncbed_collect_indels(True)
    ctx.juncbed_add_span_seq(hC)
    js = ctx.juncbed_finish(8)
    i1, d1 = ctx.juncbed_indels()
    assert (ir.junc_rows(js), ir.ins_rows(i1), ir.del_rows(d1)) == want3
    return len(wA), len(wB)


_RC = str.maketrans("ACGTN", "TGCAN")


def consensus_of(alns, sb):
    """tests/indelbed_ref.py's (junction, insertion, deletion) rows of these records"""
    recs = [(a.ref_id, a.left, a.antisense_splice, [(c >> 28, c & 0x0FFFFFFF) for c in a.cigar], a.ref_id2) for a in alns]
    sq = []
    for a in alns:
        s = bytes(sb.bases[sb.read_off[a.read_idx]:sb.read_off[a.read_idx + 1]]).decode()
        sq.append(s.translate(_RC)[::-1] if a.antisense else s)
    return ir.consensus(recs, sq)


def test_gpu_slots_reused_by_a_batch_that_needs_no_tail():
    with host.Context(0) as ctx:
        n_a, n_b = slot_sequence(ctx)
    assert n_a == N_SLOT_READS and 0 < n_b < N_SLOT_READS // 2


def test_gpu_slots_reused_with_the_host_download():
    """the download's host path (the variable is read once a process: a fresh one)"""
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_gpu_md_edges as t\nfrom tophat_amd import host\n"
            "with host.Context(0) as ctx:\n    print('SLOTS', *t.slot_sequence(ctx, consumers=False))\n") % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, THJ_DOWNLOAD_ON_HOST="1"), timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "SLOTS %d" % N_SLOT_READS in r.stdout


def pool_cases():
    lad = me.ladder_patterns(1)
    tail = [me.Read("pool/md%d" % T, anti=bool(k & 1), subs=lad[T][0]) for k, T in enumerate(range(27, 39))]
    lead = [me.Read("pool/md%d" % T, anti=bool(k & 1), subs=lad[T][0]) for k, T in enumerate(range(3, 15))]
    cases = [me.build_repeat(specs, 12, 808) for specs in (tail, lead)]
    assert cases[0][0] == cases[1][0]                   # one genome
    wants = [orc.spanning(c[2], orc.Genome(c[0]), c[1], c[3], c[4]) for c in cases]
    assert all(len(a.MD) > 24 for a in wants[0]) and all(len(a.MD) <= 24 for a in wants[1]) and len(wants[0]) == len(wants[1]) == 144
    return cases, wants


def test_gpu_extra_record_pool_reused():
    """the second and later records of a multihit read lie in the extra-record pool: a pass whose records need the tail line, then one
    over the same genome whose records do not, twice"""
    cases, wants = pool_cases()
    with host.Context(0) as ctx:
        ctx.upload_genome(host.pack_genome(cases[0][0]))
        ctx.upload_span_sets(cases[0][3], [])
        hs = [ctx.upload_span_batch(c[1]) for c in cases]
        for rnd in (0, 1):
            for k in (0, 1):
                raw, got = raw_pass(ctx, cases[k][2], hs[k], cases[k][1], cases[k][0])
                assert ctx.span_tier_counts()[1] > 0
                check(got, wants[k], cases[k][5], "variant %d, round %d: " % (k, rnd))
                unused_fields_are_zero(raw)
