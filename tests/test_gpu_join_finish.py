"""GPU parity of the chain entries' join and finish (thj_k_join_finish -> thj_k_join_closure -> thj_k_finish) against the oracle:
groups of a multihit read whose chains all abut, all need the closure search, or some of each; single chains of reads of 50 to 250
bases (one, two and more plane words)."""
import numpy as np
import pytest

import orc
from tophat_amd import host
from tophat_amd.batch import JUNC_DTYPE, SPAN_HIT_DTYPE, SpanBatch
from tophat_amd.params import Params

from test_hostsim_spanning import span_inputs

pytestmark = pytest.mark.gpu


def gapped_repeat_batch(copies, gapped, n_reads=300, seed=7):
    """reads of a `copies`-fold tandem repeat; copy c in `gapped` carries one extra base at unit position P, and every read covers P
    at a boundary of its segments -- so the chain of such a copy has a one-base gap (a deletion the closure search looks at) and
    the others abut (the deletions come back as junctions, so those chains join).  Reads that do not cover P make groups with nothing
    deferred."""
    rng = np.random.default_rng(seed)
    unit = "".join(rng.choice(list("ACGT"), size=400))
    P = 200
    flank = "".join(rng.choice(list("ACGT"), size=3000))
    starts, seq = [], flank
    for c in range(copies):
        starts.append(len(seq))
        seq += unit[:P] + ("A" if unit[P] != "A" else "C") + unit[P:] if c in gapped else unit
    seq += flank
    L, nseg, rl = 25, 4, 100
    hits, seg_off, bases, quals, read_off = [], [0], bytearray(), bytearray(), [0]
    for r in range(n_reads):
        off = P - L * int(rng.integers(1, nseg)) if r % 2 == 0 else int(rng.integers(0, 400 - rl))
        for s in range(nseg):
            for c in range(copies):
                pos = off + s * L
                left = starts[c] + pos + (1 if c in gapped and pos >= P else 0)
                ln = L if s < nseg - 1 else rl - s * L
                if c in gapped and pos < P < pos + ln:
                    continue                    # (reads with P inside a segment: that copy's segment has no exact hit)
                hits.append((1, left, 2 if s == nseg - 1 else 0, 0, 0, 1, [(1 << 28) | ln, 0, 0, 0, 0]))
            seg_off.append(len(hits))
        bases += unit[off:off + rl].encode()
        quals += bytes(rng.integers(35, 74, size=rl).astype(np.uint8))
        read_off.append(len(bases))
    sb = SpanBatch(nseg, np.arange(1, n_reads + 1, dtype=np.uint32), np.array(read_off, dtype=np.int64),
                   np.frombuffer(bytes(bases), dtype=np.uint8).copy(), np.frombuffer(bytes(quals), dtype=np.uint8).copy(),
                   np.array(seg_off, dtype=np.uint32), np.array(hits, dtype=SPAN_HIT_DTYPE))
    dels = np.array([(1, starts[c] + P - 1, starts[c] + P + 1, 0) for c in sorted(gapped)], dtype=JUNC_DTYPE)
    return seq, sb, dels


@pytest.mark.parametrize("copies,gapped", [(2, (1,)), (3, (0,)), (4, (2,)), (4, (0, 1, 2, 3)), (3, ()), (2, (0, 1))],
                         ids=lambda v: str(v).replace(" ", ""))
def test_groups_partly_all_and_not_deferred(copies, gapped):
    p = Params(max_report_intron=300, max_segment_intron=300)
    seq, sb, dels = gapped_repeat_batch(copies, set(gapped), seed=11 + copies + len(gapped))
    want = orc.spanning(p, orc.Genome([seq]), sb, dels, [])
    with host.Context(0) as ctx:
        ctx.upload_genome(host.pack_genome([seq]))
        ctx.upload_span_sets(dels, [])
        got = ctx.spanning(p, [ctx.upload_span_batch(sb)])
        groups = ctx.span_chain_groups()
    assert len(want) >= sb.n_reads // 2
    assert not gapped or any(len(a.cigar) == 3 for a in want)          # (some gapped chains joined)
    assert got == want
    assert groups > 0


@pytest.mark.parametrize("read_len,seg_len", [(50, 13), (100, 25), (150, 38), (250, 63)])
def test_single_chains_by_read_length(read_len, seg_len):
    """deletions, splices at segment boundaries and Ns: single chains of both kinds, at one to four plane words"""
    cfg = dict(seed=30 + read_len, read_len=read_len, seg_len=seg_len, extra=dict(read_mismatches=4, read_edit_dist=4, read_gap_length=3),
               gen=dict(boundary_bias=0.7, spliced_seg_frac=0.6, indel_frac=0.25, n_frac=0.1, err=0.01))
    case, p, seqs, g, sb, juncs, ins = span_inputs(cfg, n_reads=900)
    want = orc.spanning(p, g, sb, juncs, ins)
    with host.Context(0) as ctx:
        ctx.upload_genome(host.pack_genome(seqs))
        ctx.upload_span_sets(juncs, ins)
        got = ctx.spanning(p, [ctx.upload_span_batch(sb)])
        chains = ctx.span_chain_count()
    assert len(want) > 100
    assert got == want
    assert chains > 0
