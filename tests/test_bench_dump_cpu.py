"""CPU: bench.py --dump-outputs writes what the timed path's caller receives -- the event sets and the spanning records of the
last step -- as float32 / float64 .npy files under 64 MB in all, the records as the same seeded sample from run to run; and the
options of a plain run (no GPU: a stand-in for host.Context hands out canned outputs)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class _Counts:
    def __init__(self, nj, nd, ni):
        self.n_juncs, self.n_deletions, self.n_insertions = nj, nd, ni


class _FakeCtx:
    """the two calls dump_outputs makes, with outputs shaped as the library's"""

    def __init__(self, n_juncs, n_dels, n_recs, seed=5):
        from tophat_amd.batch import JUNC_DTYPE, Events
        from tophat_amd.host import ALN_DTYPE
        g = np.random.default_rng(seed)
        j = np.zeros(n_juncs, dtype=JUNC_DTYPE)
        j["ref_id"], j["left"], j["right"] = 1, np.arange(n_juncs) * 10, np.arange(n_juncs) * 10 + 500
        d = np.zeros(n_dels, dtype=JUNC_DTYPE)
        d["ref_id"], d["left"], d["right"] = 1, np.arange(n_dels) * 7, np.arange(n_dels) * 7 + 2
        self.events = Events(j, d, [(1, 40, "AC"), (1, 90, "G")], {})
        r = np.zeros(n_recs, dtype=ALN_DTYPE)
        r["read_idx"] = np.arange(n_recs)
        r["ref_id"], r["left"], r["n_cigar"], r["md_len"] = 1, g.integers(0, 1 << 26, n_recs), g.integers(1, 4, n_recs), 3
        r["cigar"] = g.integers(1, 1 << 20, (n_recs, 16))          # past n_cigar: bytes a record does not use
        r["md"] = b"10A5" + b"\xff" * 36
        self.recs = r

    def download(self, cnt):
        return self.events

    def span_download(self, n):
        return self.recs[:n]


def _dump(tmp, ctx):
    import bench
    bench.dump_outputs(str(tmp), ctx, _Counts(len(ctx.events.juncs), len(ctx.events.deletions), 2), len(ctx.recs), 0, 0)
    return {f[:-4]: np.load(os.path.join(str(tmp), f)) for f in sorted(os.listdir(str(tmp)))}


def test_dump_is_float_small_and_repeatable(tmp_path):
    import bench
    ctx = _FakeCtx(3000, 600_000, 200_000)
    a = _dump(tmp_path / "a", ctx)
    b = _dump(tmp_path / "b", _FakeCtx(3000, 600_000, 200_000))
    assert set(a) == {"junctions", "deletions", "insertions", "insertion_bases", "records", "records_md", "record_field_sums", "counts"}
    assert all(x.dtype in (np.float32, np.float64) for x in a.values())
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert a["junctions"].shape == (3000, 4) and a["junctions"][5, 1] == 50.0
    assert a["deletions"].shape == (bench.DUMP_EVENT_ROWS, 4)                      # a sample of the larger set, rows in order
    assert (np.diff(a["deletions"][:, 1]) > 0).all()
    assert a["insertions"].tolist() == [[1, 40, 2], [1, 90, 1]] and a["insertion_bases"].tolist() == [ord(c) for c in "ACG"]
    rec = a["records"]
    assert rec.shape == (bench.DUMP_RECORD_ROWS, len(bench.ALN_FIELDS) + 16)
    idx = rec[:, 0].astype(np.int64)                                               # read_idx = the record's index here
    assert (np.diff(idx) > 0).all() and np.array_equal(rec[:, 2], ctx.recs["left"][idx].astype(np.float64))
    n_cigar = rec[:, bench.ALN_FIELDS.index("n_cigar")].astype(np.int64)
    cig = rec[:, len(bench.ALN_FIELDS):]
    assert (cig[np.arange(16)[None, :] >= n_cigar[:, None]] == 0).all() and (cig[np.arange(16)[None, :] < n_cigar[:, None]] > 0).all()
    assert (a["records_md"][:, :3] == np.array([ord("1"), ord("0"), ord("A")], dtype=np.float32)).all() and not a["records_md"][:, 3:].any()
    assert a["record_field_sums"][0] == float(np.arange(200_000).sum())
    assert a["counts"].tolist() == [3000, 600_000, 2, 200_000, 0, 0]


@pytest.mark.parametrize("argv,full,dump", [([], False, None), (["--full"], True, None), (["--dump-outputs", "out"], False, "out")])
def test_plain_run_options(monkeypatch, argv, full, dump):
    import bench
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"] + argv)
    a = bench.parse_args()
    assert a.full is full and a.dump_outputs == dump and a.steps == 7 and a.warmup == 2


def test_dump_writes_no_empty_output(tmp_path):
    """a step without insertions or deletions (the default workload has no insertions): those outputs are left out -- counts.npy
    says the sets were empty -- and files of the same names from an earlier run do not stay behind"""
    ctx = _FakeCtx(50, 0, 1000)
    ctx.events.insertions = []
    d = tmp_path / "d"
    d.mkdir()
    np.save(str(d / "insertions.npy"), np.ones((2, 3)))
    out = _dump(d, ctx)
    assert set(out) == {"junctions", "records", "records_md", "record_field_sums", "counts"}
    assert all(x.size > 0 for x in out.values())
    assert out["counts"].tolist() == [50, 0, 2, 1000, 0, 0] and out["records"].shape == (1000, 29)
