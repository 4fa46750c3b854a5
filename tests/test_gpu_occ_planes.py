"""Occ64 with bit-plane symbols and the extend's counts in 32 bits, on the device (DESIGN.md §5 "Bit-plane symbols
and 32-bit counts"): bit for bit against the restatement.

Three small genomes whose lengths are 0, 1 and 63 mod 64 (the index holds both strands, so the BWT's own symbol
count is even: 0, 2 and 62 mod 64, printed with primary mod 64), each with a repeat family so that the re-seeding
option set has work.  A few hundred 150-bp reads with 2 % substitutions and some N.  Each genome is seeded
 * by the default kernel (instantiation 68: the 32-bit extend),
 * with SMEM_GPU_OCC_WIDE=1 (71: the same kernel with 64-bit counts),
 * by the plain kernel, 49 by number,
 * under a re-seeding option set, by 68 and by 71,
and bwt_sa of the seeds is looked up on a handle whose SA was densified on the device, by the hop + chase passes and
by one walk per row: sa_walk_kernel and both densify kernels read the symbol at a row from the two planes.
"""
import numpy as np
import pytest

from oracle import oracle

pytestmark = pytest.mark.gpu

OPTS = {
    "default": dict(min_seed_len=19, split_factor=1.5, split_width=10, start_width=1),
    "reseed": dict(min_seed_len=19, split_factor=1.0, split_width=500, start_width=1),
}
LENGTHS = {"mod64_0": 313 * 64, "mod64_1": 313 * 64 + 1, "mod64_63": 313 * 64 - 1}


def _genome(n, seed):
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 4, n).astype(np.uint8)
    unit = g[300:420].copy()
    for c in range(1, 12):            # a family of 12 copies: re-seeded with min_intv = 13
        g[300 + 900 * c:420 + 900 * c] = unit
    return g


@pytest.fixture(scope="module", params=list(LENGTHS))
def world(request, gpu_device):
    import smemgpu
    from smemgpu import synth
    name = request.param
    g = _genome(LENGTHS[name], 100 + len(name) + LENGTHS[name] % 64)
    idx, sa = smemgpu.Index.build_sa(g, sa_intv=32)
    reads = synth.concat_reads([
        synth.make_reads(g, 300, 150, seed=9, sub_rate=0.02, n_rate=0.004),
        synth.make_reads(g[250:11_000], 60, 150, seed=10, sub_rate=0.02, n_rate=0.0),   # over the repeat family
    ])
    ref = oracle.OracleIndex(words=idx.words, primary=idx.primary, L2=idx.L2)
    osa = oracle.OracleSA(sa=sa.samples, sa_intv=32, seq_len=idx.seq_len)
    print(f"[occ_planes] {name}: genome {g.size} (mod 64 = {g.size % 64}), BWT symbols {idx.seq_len} "
          f"(mod 64 = {idx.seq_len % 64}), primary mod 64 = {idx.primary % 64}, {reads.n} reads, "
          f"{int((reads.codes > 3).sum())} N")
    w = dict(name=name, g=g, idx=idx, sa=sa, reads=reads, ref=ref, osa=osa,
             want={o: oracle.seed(ref, reads.codes, reads.offs, threads=4, **OPTS[o])[0] for o in OPTS})
    yield w
    osa.close()
    ref.close()


def _diff(got, want):
    from smemgpu import synth
    a, b = synth.read_smgo(got), synth.read_smgo(want)
    bad = [i for i in range(len(b)) if len(a[i]) != len(b[i]) or any(
        x.shape != y.shape or (x != y).any() for x, y in zip(a[i], b[i]))]
    return f"{len(bad)} reads differ, first {bad[:8]}"


def _seed(gpu, reads, optname):
    import smemgpu
    return smemgpu.seed(gpu, reads.codes, reads.offs, smemgpu.Options(**OPTS[optname]))


def _sa_matches(gpu, w):
    reads = w["reads"]
    gpu.load_sa(w["sa"])
    b = gpu.batch(reads.n, reads.codes.size, int(reads.lens.max()))
    try:
        b.set_reads(reads.codes, reads.offs)
        b.run()
        b.sa(19, 10000)
        res = b.fetch()
        counts, k = oracle.sa_queries([res.read_calls(i) for i in range(reads.n)], 19, 10000)
        assert k.size > reads.n                  # the lookups have work, repeats included
        assert np.array_equal(res.sa_pos, w["osa"].lookup(w["ref"], k))
        assert [res.read_sa(i).size for i in range(reads.n)] == counts.tolist()
    finally:
        b.close()


def test_default_kernel_plain_kernel_and_sa(world, gpu_device, monkeypatch):
    import smemgpu
    monkeypatch.delenv("SMEM_GPU_OCC_WIDE", raising=False)
    monkeypatch.setenv("SMEM_GPU_DENSIFY", "hop")
    w = world
    assert smemgpu.load().smem_occ_narrow_ok(w["idx"].L2.ctypes.data) == 1
    gpu = smemgpu.Gpu(w["idx"], device=gpu_device)
    try:
        assert gpu.seed_kernel == 68
        for o in OPTS:                                     # 68 under the defaults and the re-seeding set
            got = _seed(gpu, w["reads"], o).to_smgo()
            assert got == w["want"][o], (w["name"], 68, o, _diff(got, w["want"][o]))
        _sa_matches(gpu, w)                                # SA densified by hop + chase
        gpu.set_variant(49)
        assert gpu.seed_kernel == 49
        got = _seed(gpu, w["reads"], "default").to_smgo()
        assert got == w["want"]["default"], (w["name"], 49, _diff(got, w["want"]["default"]))
    finally:
        gpu.close()


def test_wide_kernel_and_sa_by_walk(world, gpu_device, monkeypatch):
    import smemgpu
    monkeypatch.setenv("SMEM_GPU_OCC_WIDE", "1")
    monkeypatch.setenv("SMEM_GPU_DENSIFY", "walk")
    w = world
    gpu = smemgpu.Gpu(w["idx"], device=gpu_device)
    try:
        assert gpu.seed_kernel == 71                       # the other instantiation runs
        for o in OPTS:
            got = _seed(gpu, w["reads"], o).to_smgo()
            assert got == w["want"][o], (w["name"], 71, o, _diff(got, w["want"][o]))
        _sa_matches(gpu, w)                                # SA densified by one walk per row
        gpu.set_variant(68)                                # 68 by number on a wide handle: still 71
        assert gpu.seed_kernel == 71
    finally:
        gpu.close()
    monkeypatch.setenv("SMEM_GPU_OCC_WIDE", "0")           # 0 forces nothing
    gpu = smemgpu.Gpu(w["idx"], device=gpu_device)
    try:
        assert gpu.seed_kernel == 68
    finally:
        gpu.close()
