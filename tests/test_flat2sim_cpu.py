"""CPU: flat2_read (thj_core.h), stage 1's straight-line enumeration of a read with at most two hits in every segment, against the
loops it stands for -- gaps_prepare, and unless that asks for the rescue indels_enumerate and gaps_enumerate.  tests/flat2sim
generates 120 000 reads from a seed over a small set of coordinates (two contigs, both strands, 1-4 segments of 0-2 hits, read
lengths 20-100, 0-3 mate hits, bowtie2 off and on with max_seg_multihits 1-3) and compares per read the two task multisets word for
word, the counts, the rescue verdict and `size`; it fails when a read differs or when one of its categories has fewer than a hundred
reads.  The program runs plain and under the address and undefined-behaviour sanitizers, a process of its own each time."""
import os
import subprocess

import pytest

from locked_make import locked_make

HERE = os.path.dirname(os.path.abspath(__file__))
CATEGORIES = ("abutting_partner", "s1_window", "s2_window", "both_candidates", "second_hit_window", "deletion_pair", "insertion_pair",
              "antisense_pair", "rescue", "max_seg_multihits_return", "single_segment_return")
SEED, READS = 15, 120000


@pytest.fixture(scope="module")
def exes():
    d = os.path.join(HERE, "flat2sim")
    locked_make(d)
    return os.path.join(d, "flat2sim"), os.path.join(d, "flat2sim_san")


def run_sim(exe):
    r = subprocess.run([exe, str(SEED), str(READS)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    line = [x for x in r.stdout.splitlines() if x.startswith("FLAT2SIM")][0].split()
    return {line[k]: int(line[k + 1]) for k in range(1, len(line), 2)}


def test_flat2_read_equals_the_loops(exes):
    counts = None
    for exe in exes:
        c = run_sim(exe)
        print(os.path.basename(exe), c)
        assert c["reads"] == READS and c["differ"] == 0
        for k in CATEGORIES:
            assert c[k] >= 100, (k, c[k])
        assert counts is None or c == counts
        counts = c
