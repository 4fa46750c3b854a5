"""bench.py's plain run and --dump-outputs.

CPU: dump_outputs on a stand-in batch -- the files hold the per-read counts of
every read and, for a seeded sample of reads, exactly the lists fetch()
returned; the same call writes the same bytes; the size cap holds.  The
benchmark's genome generator draws in threads what it drew in one, byte for
byte.

GPU: one plain `bench.py --gpus 1 --steps 3 --warmup 1 --dump-outputs DIR` on
a 1 Mbp genome: the line says 3 steps and a consistent ms_per_step, carries
none of the --full records, and the dumped lists are the C restatement's for
the same reads.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("intv_per_read", "calls_per_read", "sample_reads", "intv", "intv_off", "call_n", "call_off")


class _Batch:
    """Stand-in for smemgpu.Batch: fetch() returns seeded lists (0-3 smem_next2 calls of 1-8 intervals per read)"""

    def __init__(self, n_reads: int, seed: int):
        from smemgpu.lib import Results
        rng = np.random.default_rng(seed)
        n_calls = rng.integers(0, 4, size=n_reads)
        call_n = rng.integers(1, 9, size=int(n_calls.sum())).astype(np.uint32)
        call_off = np.concatenate([[0], np.cumsum(n_calls)]).astype(np.uint64)
        per_read = np.array([call_n[int(a):int(b)].sum() for a, b in zip(call_off[:-1], call_off[1:])])
        intv_off = np.concatenate([[0], np.cumsum(per_read)]).astype(np.uint64)
        # x0, x1, x2 up to 2 x 3.1e9 and info = (start << 32) | end, as the kernel writes them
        intv = rng.integers(0, 6_203_609_478, size=(int(intv_off[-1]), 4)).astype(np.uint64)
        intv[:, 3] = (rng.integers(0, 250, size=intv.shape[0]).astype(np.uint64) << np.uint64(32)) | np.uint64(250)
        self.res = Results(intv, intv_off, call_n, call_off)
        self.masks = []

    def fetch(self, mask=None):
        self.masks.append(mask)
        return self.res


def _load(d):
    return {k: np.load(os.path.join(d, k + ".npy")) for k in NAMES}


def test_dump_outputs_holds_the_fetched_lists(built, tmp_path):
    import bench
    from smemgpu.lib import FETCH_INTV
    b = _Batch(5000, seed=3)
    bench.dump_outputs(str(tmp_path / "a"), b, seed=1)
    assert b.masks == [FETCH_INTV]
    got = _load(tmp_path / "a")
    assert all(got[k].dtype == (np.float32 if k.endswith("per_read") else np.float64) for k in NAMES)
    res = b.res
    assert np.array_equal(got["intv_per_read"], np.diff(res.intv_off.astype(np.int64)))
    assert np.array_equal(got["calls_per_read"], np.diff(res.call_off.astype(np.int64)))
    pick = got["sample_reads"].astype(np.int64)
    assert pick.size == 5000 and np.array_equal(pick, np.arange(5000))   # fewer reads than DUMP_READS: all of them
    assert np.array_equal(got["intv"].astype(np.uint64), res.intv)        # float64 holds every value exactly
    assert np.array_equal(got["call_n"], res.call_n)
    assert np.array_equal(got["intv_off"], res.intv_off) and np.array_equal(got["call_off"], res.call_off)
    # same inputs, same bytes
    bench.dump_outputs(str(tmp_path / "b"), _Batch(5000, seed=3), seed=1)
    for k in NAMES:
        with open(tmp_path / "a" / (k + ".npy"), "rb") as fa, open(tmp_path / "b" / (k + ".npy"), "rb") as fb:
            assert fa.read() == fb.read(), k


def test_dump_outputs_samples_within_its_size_cap(built, tmp_path, monkeypatch):
    import bench
    b = _Batch(5000, seed=4)
    monkeypatch.setattr(bench, "DUMP_BYTES", 200_000)
    monkeypatch.setattr(bench, "DUMP_READS", 1000)
    bench.dump_outputs(str(tmp_path), b, seed=7)
    files = [os.path.join(tmp_path, k + ".npy") for k in NAMES]
    assert sum(os.path.getsize(f) for f in files) <= 200_000
    got = _load(tmp_path)
    pick = got["sample_reads"].astype(np.int64)
    assert 0 < pick.size < 1000 and np.all(np.diff(pick) > 0)
    # the sample is a prefix of a seeded order of the reads, whatever the outputs are
    order = np.random.default_rng([7, 0x44554d50]).permutation(5000)
    assert np.array_equal(pick, np.sort(order[:pick.size]))
    res = b.res
    io, co = res.intv_off.astype(np.int64), res.call_off.astype(np.int64)
    for j, r in enumerate(pick):
        a, e = int(got["intv_off"][j]), int(got["intv_off"][j + 1])
        assert np.array_equal(got["intv"][a:e].astype(np.uint64), res.intv[io[r]:io[r + 1]])
        a, e = int(got["call_off"][j]), int(got["call_off"][j + 1])
        assert np.array_equal(got["call_n"][a:e], res.call_n[co[r]:co[r + 1]])


def test_plain_is_the_default_and_steps_are_checked(built):
    import bench
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 3)
    assert bench.parse(["--full", "--dump-outputs", "x"]).full
    with pytest.raises(SystemExit):
        bench.parse(["--steps", "0"])


def test_threaded_genome_draws_are_the_serial_ones():
    """make_genome_human_like's threaded helpers draw what the single calls
    they stand for draw, and leave the generator in the same state."""
    from concurrent.futures import ThreadPoolExecutor
    from smemgpu import synth
    with ThreadPoolExecutor(max_workers=synth.WORKERS) as pool:
        n = (1 << 24) + 13   # a tail past the last whole 64-bit step
        a, b = np.random.default_rng(11), np.random.default_rng(11)
        assert np.array_equal(synth._random_codes(a, n, pool), b.integers(0, 4, size=n, dtype=np.uint8))
        assert a.integers(0, 1 << 20, size=5).tolist() == b.integers(0, 1 << 20, size=5).tolist()
        # a 32-bit draw first: its unused half must survive the threaded step
        a.integers(0, 1 << 31, dtype=np.uint32), b.integers(0, 1 << 31, dtype=np.uint32)
        rows, F = 5001, 301
        div = np.linspace(0.02, 0.3, rows)
        ca, cb = np.zeros((rows, F), dtype=np.uint8), np.zeros((rows, F), dtype=np.uint8)
        synth._diverge(ca, div, a, pool)
        synth._diverge(cb, div, b, None)
        assert np.array_equal(ca, cb) and ca.any()
        assert a.integers(0, 4, size=9, dtype=np.uint8).tolist() == b.integers(0, 4, size=9, dtype=np.uint8).tolist()


def test_human_like_genome_bytes_are_pinned():
    """The benchmark's inputs do not move: 64 Mbp (large enough for the
    threaded steps) hashes to what the generator gave before it was threaded."""
    import hashlib
    from smemgpu import synth
    g = synth.make_genome_human_like(64_000_000, seed=3, n_chrom=5)
    assert g.chrom_starts.tolist() == [0, 29457327, 34805814, 35240143, 54300916, 64000000]
    assert hashlib.sha256(g.codes.tobytes()).hexdigest() == \
        "eb9676c0648f8fd0de476844ba3a539412d8c0be94ed6bc28055b810358fb816"


@pytest.mark.gpu
def test_plain_run_dumps_the_last_step(gpu_device, tmp_path):
    import bench
    import smemgpu
    from oracle import oracle
    from smemgpu import synth
    argv = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--genome-mbp", "1", "--genome-profile", "uniform",
            "--reads", "3000", "--cache", str(tmp_path / "cache"), "--dump-outputs", str(tmp_path / "out")]
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["metric"] == bench.METRIC and line["unit"] == "reads/s" and line["higher_is_better"] is True
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(3000 / (line["ms_per_step"] * 1e-3), rel=0.01)
    assert line["full"] is False
    for k in ("roofline", "cpu_baseline", "parity_sample", "streaming", "sa_lookup", "chaining", "alignment",
              "sw_extension", "e2e", "uniform", "human_like"):
        assert k not in line
    # the same genome, index and reads here; the restatement's lists for them
    a = bench.parse(argv)
    g = bench.make_genome(a)
    idx = smemgpu.Index.build(g.codes)
    reads = bench.make_reads(a, 0, g.codes, 1)
    oi = oracle.OracleIndex(words=idx.words, primary=idx.primary, L2=idx.L2)
    want, _, _ = oracle.seed(oi, reads.codes, reads.offs, min_seed_len=a.min_seed_len)
    oi.close()
    want = synth.read_smgo(want)
    got = _load(tmp_path / "out")
    assert np.array_equal(got["sample_reads"], np.arange(3000))
    assert np.array_equal(got["intv_per_read"], [sum(c.shape[0] for c in calls) for calls in want])
    assert np.array_equal(got["calls_per_read"], [len(calls) for calls in want])
    assert np.array_equal(got["call_n"], [c.shape[0] for calls in want for c in calls])
    assert np.array_equal(got["intv"].astype(np.uint64), np.concatenate([c for calls in want for c in calls]))
