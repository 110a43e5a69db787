"""GPU: the planted reads of load_group_cases.py through the stitch kernels against the oracle, record by record -- the reads whose
genome pieces, hit records, planes and chain entries tier 0 (thj_k_stitch_contig), the chain join (thj_k_join_finish) and the finish
(thj_k_finish) load unconditionally and in groups: read lengths on either side of a 64-base piece and of a plane word, one to six
segments, both strands, alignments on the first and the last base of a contig, junctions inside a segment hit and on a segment
boundary, a deletion, four and five MATCH pieces, chain lists of 1, 255, 256 and 257 entries and a group of two chains.
(test_loadsim_cpu.py shows that the batches are what they are meant to be, and that no load leaves its array.)"""
import pytest

import load_group_cases as lg
from tophat_amd import host

pytestmark = pytest.mark.gpu


def gpu_records(ctx, case):
    seqs, sb, p, juncs, ins, _tags = case
    ctx.upload_genome(host.pack_genome(seqs))
    ctx.upload_span_sets(juncs, ins)
    return ctx.spanning(p, [ctx.upload_span_batch(sb)])


@pytest.mark.parametrize("name", lg.NAMES)
def test_gpu_load_groups(name):
    case, want = lg.case(name), list(lg.expected(name))
    with host.Context(0) as ctx:
        got = gpu_records(ctx, case)
        chains, groups = ctx.span_chain_count(), ctx.span_chain_groups()
    assert got == want, lg.me.explain(got, want, case[5])
    if name.startswith("list"):
        assert chains == int(name[4:])                   # the chain list of exactly that many entries
    elif name in ("seg4", "long3"):
        assert chains > 0                                # spliced reads of at most four segments travel as chain entries
    elif name == "twocopy":
        assert groups == case[1].n_reads                 # region B's dense list: a group of two chains a read
    else:
        assert chains == 0                               # batches of five and six segments: the <8> tier-0 instance, no chain entries
