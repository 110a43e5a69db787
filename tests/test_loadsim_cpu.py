"""CPU: the unconditional loads of tier 0, the chain join and the finish of a joined hit stay inside their arrays.  tests/loadsim compiles
span_read_contig_pre / contig_finish, chain_entry_fetch and joined_extras (thj_span_core.h) for the CPU and runs them over the planted
reads of load_group_cases.py with every array in a heap block of exactly its size; the program runs plain and under the address and
undefined-behaviour sanitizers -- a process of its own each time -- and its records are the oracle's.  The planted batches are what
they are meant to be: the oracle reports the reads that the families exist for."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import load_group_cases as lg
import sim
from locked_make import locked_make
from tophat_amd import host
from tophat_amd.batch import JUNC_DTYPE

HERE = os.path.dirname(os.path.abspath(__file__))
MAGIC = 0x4C4F4144


@pytest.fixture(scope="module")
def exes():
    d = os.path.join(HERE, "loadsim")
    locked_make(d)
    return os.path.join(d, "loadsim"), os.path.join(d, "loadsim_san")


def write_case(path, name):
    seqs, sb, p, juncs, ins, _tags = lg.case(name)
    assert not ins
    l = sim.lib()
    g = host.pack_genome(seqs, lib=l)
    d = host.pack_span_batch(sb, lib=l)
    j = np.ascontiguousarray(juncs, dtype=JUNC_DTYPE)
    with open(path, "wb") as f:
        f.write(struct.pack("<6i3q", MAGIC, g.n_contigs, d["n_reads"], d["nseg"], d["W"], d["qual_stride"], len(g.blocks), len(d["hits"]), len(j)))
        f.write(bytes(p.as_ctypes()))
        f.write(g.blocks.tobytes())
        f.write(g.contig_blk.astype(np.uint32).tobytes())
        f.write(g.lens.astype(np.int32).tobytes())
        seg_off = np.ascontiguousarray(d["seg_off"], dtype=np.uint32)
        assert len(seg_off) == d["n_reads"] * d["nseg"] + 1
        f.write(seg_off.tobytes())
        assert d["hits"].dtype.itemsize == 32
        f.write(d["hits"].tobytes())
        assert len(d["planes"]) == d["n_reads"] * 3 * d["W"] and len(d["quals"]) == d["n_reads"] * d["qual_stride"]
        f.write(d["planes"].tobytes())
        f.write(np.ascontiguousarray(d["read_len"], dtype=np.uint16).tobytes())
        f.write(d["quals"].tobytes())
        f.write(j.tobytes())
    return seqs, sb


def run_sim(exe, case_file, out_file):
    r = subprocess.run([exe, case_file, out_file], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    line = [x for x in r.stdout.splitlines() if x.startswith("LOADSIM")][0].split()
    return {line[k]: int(line[k + 1]) for k in range(1, len(line), 2)}


@pytest.mark.parametrize("name", lg.NAMES)
def test_loads_stay_in_their_arrays(name, exes, tmp_path):
    cf = str(tmp_path / "case.bin")
    seqs, sb = write_case(cf, name)
    want = list(lg.expected(name))
    tags = lg.case(name)[5]
    counts = None
    for exe in exes:
        of = str(tmp_path / (os.path.basename(exe) + ".rec"))
        c = run_sim(exe, cf, of)
        raw = np.fromfile(of, dtype=host.ALN_DTYPE)
        got = host.alns_from_array(raw, host.span_md_resolver(list(seqs), [sb], sim.lib()))
        assert got == want, "%s: %s" % (os.path.basename(exe), lg.me.explain(got, want, tags))
        assert counts is None or c == counts
        counts = c
    if name.startswith("list"):
        assert counts["chain"] == int(name[4:]) and counts["tier0"] == 0
    if name == "twocopy":
        assert counts["groups"] == sb.n_reads
    if name in ("seg4", "long3"):
        assert counts["chain"] > 0 and counts["tier0"] > 0


def test_the_planted_reads_are_what_they_are_meant_to_be():
    by = {}
    for name in lg.NAMES:
        tags = lg.case(name)[5]
        want = lg.expected(name)
        rec = {}
        for a in want:
            rec.setdefault(a.read_idx, []).append(a)
        if name == "twocopy":
            assert all(len(rec.get(r, [])) == 2 for r in range(len(tags))), name
            continue
        assert sorted(rec) == list(range(len(tags))), (name, [tags[r] for r in range(len(tags)) if r not in rec][:8])
        for r, (a,) in rec.items():
            by[(name, tags[r])] = a
    seqs = lg.case("seg4")[0]
    assert len(seqs) >= 4
    every = [a for a in by.values()]
    assert any(a.left == 0 for a in every)                                                      # base 0 of a contig
    ends = {a.ref_id for a in every if a.left + sum(c & 0x0FFFFFFF for c in a.cigar if (c >> 28) in (1, 5, 11)) == len(seqs[a.ref_id - 1])}
    assert len(seqs) in ends and any(r < len(seqs) for r in ends)                               # the last base of an inner and of the last contig
    n_ops = {len(a.cigar) for a in every}
    assert {1, 3, 5} <= n_ops
    assert max(a.XM for a in every) >= 7 and any("^" in a.MD for a in every)
    for rl in (50, 64, 65, 100):
        for k in (0, 1, 2) if rl == 100 else (0, 1):       # (a read of two segments: its middle segment is its last)
            for strand in ("sense", "anti"):
                assert len(by[("seg4", "seg4/rl%d/junction_in_hit%d/%s" % (rl, k, strand))].cigar) == 3
    assert all(len(by[("long3", "long3/rl150/two_junctions/%s" % s)].cigar) == 5 for s in ("sense", "anti"))
