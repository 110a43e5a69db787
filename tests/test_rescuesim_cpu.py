"""CPU: flat_rescue_read (thj_core.h), the per-read body of thj_k_sj_rescue_flat -- the packed entry thj_k_sj_flat writes, the mate
hits, the flank scans of the mate hits that suit the first-segment hit, flat_rescue -- against what it stands for: rescue_scan for
every mate hit, then flat_rescue, as tests/hostsim does it.  tests/rescuesim generates 60 000 reads from a seed over a small set of
coordinates (two contigs, both strands, 2-4 kept segments with one hit in the first, read lengths 50-100, 0-3 mate hits, two
settings of the inner distance, bowtie2 off and on), hands the new function the packed entry and every array in a heap block of its
exact size, and compares per read the task words, the pair count and the window count; it fails when a read differs or when one of
its categories has fewer than a hundred reads.  The program runs plain and under the address and undefined-behaviour sanitizers, a
process of its own each time."""
import os
import subprocess

import pytest

from locked_make import locked_make

HERE = os.path.dirname(os.path.abspath(__file__))
CATEGORIES = ("compatible_pair", "other_contig", "same_strand", "break_then_good", "flank_clipped", "abutting_pseudo_hit",
              "below_min_intron", "at_or_above_max_intron", "size2_window", "size3_window", "antisense_first_hit", "two_mates_windows")
SEED, READS = 16, 60000


@pytest.fixture(scope="module")
def exes():
    d = os.path.join(HERE, "rescuesim")
    locked_make(d)
    return os.path.join(d, "rescuesim"), os.path.join(d, "rescuesim_san")


def run_sim(exe):
    r = subprocess.run([exe, str(SEED), str(READS)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    line = [x for x in r.stdout.splitlines() if x.startswith("RESCUESIM")][0].split()
    return {line[k]: int(line[k + 1]) for k in range(1, len(line), 2)}


def test_flat_rescue_read_equals_scan_then_flat_rescue(exes):
    counts = None
    for exe in exes:
        c = run_sim(exe)
        print(os.path.basename(exe), c)
        assert c["reads"] == READS and c["differ"] == 0
        for k in CATEGORIES:
            assert c[k] >= 100, (k, c[k])
        assert counts is None or c == counts
        counts = c
