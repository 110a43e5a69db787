"""Test-only inputs for the `samtools sort` order (thj_bam_stream_sort) whose expected order is written out by hand, and the seeded crowd.
A record is (tid, pos, strand, size); `want` lists input record numbers in output order, `blocks` what the reference would have written.

How the hand rows come about (bam_sort.c): blocks end with the record that brings their bytes to max_mem; each is sorted stably by
(tid, pos + 1); with more than one block a heap hands out the least head by (tid, pos + 1, strand), ties to the lower block."""
import random

F, R = 0, 1


def cases():
    same = [(0, 5, R, 50), (0, 5, F, 50), (0, 5, F, 50), (0, 5, R, 50)]
    return [
        # one block: a plain stable sort, the strand plays no part
        dict(label="one_block_ties_keep_input_order", max_mem=1000, recs=[(0, 5, F, 50), (0, 3, R, 50), (0, 5, R, 50), (0, 3, F, 50)], want=[1, 3, 0, 2], blocks=1),
        dict(label="same_position_one_block", max_mem=1000, recs=same, want=[0, 1, 2, 3], blocks=1),
        # blocks {0, 1} {2, 3} and the empty remainder.  Heads 0 (reverse) and 2 (forward): 2; then 3 (reverse) ties with 0, block 0 first: 0;
        # its next head 1 is forward and below 3: 1; then 3
        dict(label="reverse_before_forward_in_a_block", max_mem=100, recs=same, want=[2, 0, 1, 3], blocks=3),
        # blocks {0, 1} {2, 3} {4}: every block's forward head goes first, in block order, then the reverse ones
        dict(label="forward_heads_of_every_block_first", max_mem=100, recs=[(0, 5, F, 50), (0, 5, R, 50), (0, 5, F, 50), (0, 5, R, 50), (0, 5, F, 50)], want=[0, 2, 4, 1, 3], blocks=3),
        # tid -1 has a high word of ones: last; pos -1 a low word of 0: first of its contig
        dict(label="unmapped_last_no_position_first", max_mem=1000, recs=[(-1, -1, F, 40), (1, 0, F, 40), (0, -1, R, 40), (0, 0, F, 40)], want=[2, 3, 1, 0], blocks=1),
        # blocks sorted to [1, 0] and [3, 2]: heads 1 (pos 2, reverse) and 3 (pos 1): 3; then 2 (pos 2, forward) below 1: 2; 1; 0.
        # The plain stable sort gives 3, 1, 2, 0
        dict(label="strand_orders_across_blocks", max_mem=100, recs=[(0, 7, F, 50), (0, 2, R, 50), (0, 2, F, 50), (0, 1, R, 50)], want=[3, 2, 1, 0], blocks=3),
        # the bytes reach max_mem exactly with the last record: the block ends, an empty one follows and the two are merged
        dict(label="max_mem_is_the_total", max_mem=100, recs=[(0, 3, R, 40), (0, 3, F, 60)], want=[0, 1], blocks=2),
        dict(label="max_mem_one_above_the_total", max_mem=101, recs=[(0, 3, R, 40), (0, 3, F, 60)], want=[0, 1], blocks=1),
        # block {0, 1, 2} and the remainder {3}: once a block's reverse record is out the block's later records of the position follow it
        dict(label="a_block_drains_behind_its_reverse_record", max_mem=150, recs=[(0, 5, R, 50), (0, 5, F, 50), (0, 5, F, 50), (0, 5, F, 50)], want=[3, 0, 1, 2], blocks=2),
        # a record larger than max_mem is a block of its own
        dict(label="a_record_above_max_mem", max_mem=60, recs=[(0, 9, F, 200), (0, 1, R, 40), (0, 1, F, 40), (0, 1, F, 40)], want=[3, 1, 2, 0], blocks=3),
    ]


def crowd(seed=7, n_inputs=400):
    """seeded inputs of 0..60 records over few positions, so that ties abound: (label, max_mem, recs)"""
    r = random.Random(seed)
    out = []
    for k in range(n_inputs):
        n = r.randrange(0, 61)
        recs = [(r.choice((-1, 0, 0, 1, 2)), r.choice((-1, 0, 1, 1, 2, 3)), r.randrange(2), r.choice((37, 38, 39, 40, 64, 100, 150))) for _ in range(n)]
        total = sum(x[3] for x in recs)
        max_mem = r.choice((100, 150, 300, 700, 10 ** 9, max(1, total), max(1, total) + 1))
        out.append(("crowd_%d" % k, max_mem, recs))
    return out
