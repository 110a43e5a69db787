"""GPU: thj_bam_stream_sort -- the context's BAM stream in the order `samtools sort` (0.1.18) gives the file.  Every case goes
bam_stream_upload -> bam_stream_sort -> bam_stream_download and is compared byte for byte with the order of the restatement of the
reference's loop (bamsort_ref.py) applied to the input records: the orders its own binary wrote (tests/golden/samtools_sort) and the
hand rows (bamsort_cases.py); record counts around the wave and the scan's tile (0, 1, 2, 63, 64, 65, 1025) with one block and with
max_mem 300; one (tid, pos) of 5000 records with random strands over 8 blocks; distinct positions in falling order; sizes of 37..40
bytes so that every source and destination alignment occurs, with one record of 65000 bytes; unmapped records and records without a
position among mapped ones; contig numbers up to 2^31 - 1; max_mem equal to the total; and the contract."""
import json
import os
import random

import pytest

import bamsort_cases as bc
import bamsort_ref as bs
from tophat_amd import host

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "samtools_sort")
ONE_BLOCK = 10 ** 12


@pytest.fixture(scope="module")
def ctx():
    with host.Context(0) as c:
        yield c


def check(ctx, recs, max_mem, label=""):
    """-> (the restatement's order, its block count) after the device's stream, sizes and block count were held against them"""
    raw = bs.records_bytes(recs)
    order, nb = bs.order(recs, max_mem)
    want = [raw[k] for k in order]
    ctx.bam_stream_upload(b"".join(raw))
    sizes, got_nb = ctx.bam_stream_sort([len(x) for x in raw], max_mem)
    got = ctx.bam_stream_download(sum(len(x) for x in raw))
    assert got_nb == nb, label
    assert sizes == [len(w) for w in want], label
    assert got == b"".join(want), label
    return order, nb


def minted():
    man = json.load(open(os.path.join(GOLD, "MANIFEST.json")))
    for name in sorted(man["cases"]):
        c = json.load(open(os.path.join(GOLD, name + ".json")))
        yield name, c["max_mem"], [tuple(r) for r in c["records"]], c["order"]


def test_the_reference_binarys_orders(ctx):
    differ = 0
    for name, max_mem, recs, want in minted():
        order, _nb = check(ctx, recs, max_mem, name)
        assert order == want, name
        differ += want != bs.plain_order(recs)
    assert differ >= 2


def test_hand_rows(ctx):
    for c in bc.cases():
        assert check(ctx, c["recs"], c["max_mem"], c["label"]) == (c["want"], c["blocks"]), c["label"]


@pytest.mark.parametrize("max_mem", (ONE_BLOCK, 300))
@pytest.mark.parametrize("n", (0, 1, 2, 63, 64, 65, 1025))
def test_record_counts(ctx, n, max_mem):
    r = random.Random(n)
    recs = [(r.randrange(3), r.randrange(8), r.randrange(2), r.randrange(40, 120)) for _ in range(n)]
    _order, nb = check(ctx, recs, max_mem)
    assert nb == 1 if max_mem == ONE_BLOCK or n < 3 else nb > 1


def test_one_position_across_blocks_and_workgroups(ctx):
    r = random.Random(5)
    recs = [(1, 777, r.randrange(2), 60 + k % 5) for k in range(5000)]
    order, nb = check(ctx, recs, 40000)
    assert nb >= 7 and order != list(range(5000))


def test_distinct_positions_falling(ctx):
    recs = [(k // 1500, 100000 - 3 * (k % 1500), k % 2, 50 + k % 7) for k in range(3000)]
    for max_mem in (ONE_BLOCK, 20000):
        order, _nb = check(ctx, recs, max_mem)
        assert order == bs.plain_order(recs) and order[0] == 1499


def test_every_alignment_and_a_long_record(ctx):
    r = random.Random(9)
    recs = [(r.randrange(2), r.randrange(40), r.randrange(2), r.choice((37, 38, 39, 40))) for _ in range(600)]
    recs.insert(301, (0, 20, 1, 65000))
    raw = bs.records_bytes(recs)
    for max_mem in (ONE_BLOCK, 5000):
        order, _nb = check(ctx, recs, max_mem)
        # every (source offset mod 4, destination offset mod 4) pair occurs
        src, at = [], 0
        for x in raw:
            src.append(at % 4); at += len(x)
        pairs, at = set(), 0
        for k in order:
            pairs.add((src[k], at % 4)); at += len(raw[k])
        assert len(pairs) == 16


def test_unmapped_and_positionless_records(ctx):
    r = random.Random(11)
    recs = [r.choice(((-1, -1), (0, -1), (1, -1), (0, 0), (1, 5), (2, 0))) + (r.randrange(2), r.randrange(45, 70)) for _ in range(500)]
    for max_mem in (ONE_BLOCK, 3000):
        order, _nb = check(ctx, recs, max_mem)
        assert recs[order[0]][:2] == (0, -1) and recs[order[-1]][:2] == (-1, -1)


def test_large_contig_numbers(ctx):
    r = random.Random(13)
    tids = (0, 1, 2 ** 16, 2 ** 30, 2 ** 31 - 2, 2 ** 31 - 1)
    recs = [(r.choice(tids), r.choice((0, 3, 2 ** 31 - 2)), r.randrange(2), r.randrange(40, 80)) for _ in range(400)]
    for max_mem in (ONE_BLOCK, 2500):
        order, _nb = check(ctx, recs, max_mem)
        assert recs[order[-1]][0] == 2 ** 31 - 1
    check(ctx, recs + [(-1, -1, 0, 50)], 2500)


def test_max_mem_is_the_total(ctx):
    r = random.Random(17)
    recs = [(0, r.randrange(3), r.randrange(2), r.randrange(40, 80)) for _ in range(200)]
    total = sum(x[3] for x in recs)
    assert check(ctx, recs, total)[1] == 2 and check(ctx, recs, total + 1)[1] == 1
    assert check(ctx, recs, 1)[1] == 201                                # every record a block of its own


def test_contract(ctx):
    recs = [(0, 9, 0, 50), (0, 3, 1, 60), (0, 3, 0, 44)]
    raw = bs.records_bytes(recs)
    stream = b"".join(raw)
    sizes = [len(x) for x in raw]

    def refused(data, given, words, max_mem=1000):
        ctx.bam_stream_upload(data)
        with pytest.raises(host.ThjError) as e:
            ctx.bam_stream_sort(given, max_mem)
        assert "failed (-1)" in str(e.value) and words in str(e.value), str(e.value)      # THJ_EINVAL
        assert ctx.bam_stream_download(len(data)) == data                 # the stream is unchanged

    # a size that disagrees with the record's block_size (the total still matches the stream)
    refused(stream, [51, 59, 44], "does not fill its size")
    # a block_size below 32
    short = bytearray(stream)
    short[0:4] = (31).to_bytes(4, "little")
    refused(bytes(short), sizes, "does not fill its size")
    refused(stream, [50, 60], "add up to")
    refused(stream, [50, 60, 20, 24], "has a size of")
    refused(stream, sizes, "bad argument", max_mem=0)
    below = bs.make_record(0, -2, 0, 50)
    refused(below, [50], "position below -1")
    # a sorted stream sorted again with one block stays as it is
    order, _nb = check(ctx, recs, ONE_BLOCK)
    again = [recs[k] for k in order]
    raw2 = [raw[k] for k in order]
    ctx.bam_stream_upload(b"".join(raw2))
    s2, nb2 = ctx.bam_stream_sort([len(x) for x in raw2])
    assert nb2 == 1 and s2 == [len(x) for x in raw2] and ctx.bam_stream_download(len(stream)) == b"".join(raw2) and bs.order(again, ONE_BLOCK)[0] == [0, 1, 2]
    # nothing to sort
    ctx.bam_stream_upload(b"")
    assert ctx.bam_stream_sort([]) == ([], 1)
