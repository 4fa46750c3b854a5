"""The seeding kernel's raw log: only kept records are logged, each tagged
with its smem_next2 call's ordinal and a match / sub-match bit, and written
in pairs as whole 64-B lines.

Bar: bit-exact SMGO streams against the oracle, as tests/test_gpu_parity.py.
The cases aim at what the format can get wrong: odd and even slot strides
and the overflow pass at small capacities, the capacity boundary itself
(a read overflows exactly when its final interval count exceeds intv_cap),
reads that end on an odd record count (the lone flush), more smem_next2
calls in a read than an 8-bit ordinal holds, and re-seeding calls whose
sub-matches are partly kept and partly dropped.
"""
import numpy as np
import pytest

from oracle import oracle

pytestmark = pytest.mark.gpu

OPTS = {
    "default": dict(min_seed_len=19, split_factor=1.5, split_width=10, start_width=1),
    "k14s20": dict(min_seed_len=14, split_factor=1.5, split_width=20, start_width=1),
    "reseed": dict(min_seed_len=19, split_factor=1.0, split_width=500, start_width=1),
}


@pytest.fixture(scope="module")
def world(gpu_device):
    import smemgpu
    from smemgpu import synth
    genome = synth.make_genome(400_000, seed=21)
    idx = smemgpu.Index.build(genome.codes)
    ref = oracle.OracleIndex(words=idx.words, primary=idx.primary, L2=idx.L2)
    truth = {}  # (read set, option set) -> (reads, SMGO stream, per-read counts): computed once, never changed

    def want(kind, optname):
        key = (kind, optname)
        if key not in truth:
            reads = _reads(genome.codes, kind)
            stream, per, _ = oracle.seed(ref, reads.codes, reads.offs, threads=4, **OPTS[optname])
            truth[key] = (reads, stream, per)
        return truth[key]

    yield dict(genome=genome, idx=idx, ref=ref, want=want, device=gpu_device)
    ref.close()


def _one(arr):
    from smemgpu import synth
    arr = np.asarray(arr, np.uint8)
    return synth.Reads(np.array([arr.size], np.int32), arr, np.array([0, arr.size], np.int64))


def _reads(g, kind):
    from smemgpu import synth
    if kind == "mixed":  # lengths 1-320 with 2 % N, short reads, diverged and random 101-mers
        return synth.concat_reads([
            synth.make_reads(g, 500, (1, 320), seed=7, n_rate=0.02),
            synth.make_reads(g, 200, (15, 40), seed=8),
            synth.make_reads(g, 200, 101, seed=9, sub_rate=0.05, random_frac=0.3),
        ])
    if kind == "long":  # an N at every 10th base (one call per 9-base stretch), a clean 3000-mer, ordinary reads
        clean = g[50_000:53_000].copy()
        holed = np.where(np.arange(3000) % 10 == 9, 4, g[120_000:123_000]).astype(np.uint8)
        return synth.concat_reads([_one(holed), _one(clean), synth.make_reads(g, 200, 150, seed=10)])
    if kind == "150bp5":
        return synth.make_reads(g, 2000, 150, seed=11, sub_rate=0.05)
    raise ValueError(kind)


def _run(world, reads, optname, intv_cap=0):
    """One batch on a Gpu of its own (the capacity is a property of the Gpu): results and stats."""
    import smemgpu
    gpu = smemgpu.Gpu(world["idx"], device=world["device"], intv_cap=intv_cap)
    try:
        b = gpu.batch(reads.n, reads.codes.size, int(reads.lens.max()))
        b.set_reads(reads.codes, reads.offs)
        b.run(smemgpu.Options(**OPTS[optname]))
        st = b.stats()
        res = b.fetch()
        b.close()
        return res, st
    finally:
        gpu.close()


def _assert_stream(res, want):
    got = res.to_smgo()
    if got != want:
        from smemgpu import synth
        a, b = synth.read_smgo(got), synth.read_smgo(want)
        bad = [i for i in range(len(b)) if len(a[i]) != len(b[i]) or any(
            x.shape != y.shape or (x != y).any() for x, y in zip(a[i], b[i]))]
        pytest.fail(f"{len(bad)} reads differ, first {bad[:5]}")


@pytest.mark.parametrize("optname", ["default", "reseed"])
@pytest.mark.parametrize("intv_cap", [2, 3, 4, 5, 8, 9])
def test_pair_alignment_and_overflow_small_caps(world, intv_cap, optname):
    """Odd and even capacities (the slot stride is the capacity rounded up to
    even, the threshold the capacity itself): main and overflow pass bit-exact."""
    reads, want, _ = world["want"]("mixed", optname)
    res, st = _run(world, reads, optname, intv_cap=intv_cap)
    _assert_stream(res, want)
    if intv_cap in (2, 3):
        assert st["n_overflow"] > 0


def test_capacity_boundary(world):
    """A read overflows exactly when its final interval count exceeds intv_cap."""
    reads, want, per = world["want"]("mixed", "default")
    cnt = np.asarray(per["n_intv"]).astype(np.int64)
    M = int(cnt.max())
    # the lone-flush path (odd counts), the all-pairs path (even) and the single record are all in the batch
    assert (cnt % 2 == 1).any() and ((cnt % 2 == 0) & (cnt > 0)).any() and (cnt == 1).any()
    assert M >= 2
    res, st = _run(world, reads, "default", intv_cap=M)
    assert st["n_overflow"] == 0
    _assert_stream(res, want)
    res, st = _run(world, reads, "default", intv_cap=M - 1)
    assert st["n_overflow"] == int((cnt == M).sum())
    _assert_stream(res, want)


@pytest.mark.parametrize("optname", ["default", "k14s20"])
def test_call_ordinals(world, optname):
    """~300 smem_next2 calls in one read (past an 8-bit ordinal) and a clean
    3000-mer (forward lists past the LDS ring), beside ordinary reads."""
    from smemgpu import synth
    reads, want, per = world["want"]("long", optname)
    assert int(per["n_calls"][0]) > 256
    res, _ = _run(world, reads, optname)
    _assert_stream(res, want)
    lists = synth.read_smgo(want)
    call_n = np.array([a.shape[0] for calls in lists for a in calls], dtype=np.uint32)
    call_off = np.concatenate([[0], np.cumsum([len(calls) for calls in lists])]).astype(np.uint64)
    assert np.array_equal(res.call_off, call_off)
    assert np.array_equal(res.call_n, call_n)


def test_reseed_kept_and_dropped_submatches(world):
    """150 bp reads at 5 % substitutions under the `reseed` options: many
    re-seeding calls, whose sub-matches the merge partly keeps and partly drops."""
    from smemgpu import synth
    reads, want, _ = world["want"]("150bp5", "reseed")
    assert max(a.shape[0] for calls in synth.read_smgo(want) for a in calls) > 1
    res, _ = _run(world, reads, "reseed")
    _assert_stream(res, want)
