"""GPU: the spanning records with base qualities that vary (test_md_as_quals_cpu's batches) through the stitch kernels, against the
oracle -- tier 0, the chain entries' join and finish, and the packed multihit tier."""
import numpy as np
import pytest

import orc
from tophat_amd import host
from tophat_amd.batch import JUNC_DTYPE
from tophat_amd.params import Params

from test_md_as_quals_cpu import QUAL_CASES, mutated_repeat_batch, qual_inputs

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("cfg", QUAL_CASES, ids=lambda c: "seed%d_rl%d" % (c["seed"], c["read_len"]))
def test_gpu_records_with_random_quals_match_oracle(cfg):
    case, p, seqs, g, sb, juncs, ins = qual_inputs(cfg, 1500)
    want = orc.spanning(p, g, sb, juncs, ins)
    with host.Context(0) as ctx:
        ctx.upload_genome(host.pack_genome(seqs))
        ctx.upload_span_sets(juncs, ins)
        got = ctx.spanning(p, [ctx.upload_span_batch(sb)])
        if cfg["read_len"] == 100:
            assert ctx.span_chain_count() > 0               # reads through thj_k_chains -> thj_k_join -> thj_k_finish
    assert len(want) > 50
    assert got == want


def test_gpu_packed_tier_with_random_quals():
    nj = np.zeros(0, dtype=JUNC_DTYPE)
    seq, sb = mutated_repeat_batch(copies=12, n_reads=30, seed=41)
    p = Params(read_mismatches=8, read_edit_dist=8)
    want = orc.spanning(p, orc.Genome([seq]), sb, nj, [])
    with host.Context(0) as ctx:
        ctx.upload_genome(host.pack_genome([seq]))
        ctx.upload_span_sets(nj, [])
        got = ctx.spanning(p, [ctx.upload_span_batch(sb)])
        tiers = ctx.span_tier_counts()
    assert tiers[1] > 0, tiers                              # reads to the multihit kernel
    assert got == want
