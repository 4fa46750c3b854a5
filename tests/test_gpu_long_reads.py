"""Reads of 321 bp to 70 kbp through seeding, SA lookup and chaining on the GPU.

Bar: bit-exact, every comparison -- the interval lists against `oracle.seed`,
the positions against `OracleSA.lookup`, the chains against `oracle.chain`
(tests/test_long_reads.py pins all three to the compiled reference at these
lengths), and the g1 fixture against the reference's own streams
(tests/golden/long/).

One 300 kbp index with the planted homopolymer, dinucleotide run and repeat
family of tests/test_gpu_seed_phases.py, and the synthetic set of
tests/long_reads.py: 124 reads, 410 kbp -- two each of 321, 1000, 4095, 4096,
4097, 8191 and 8192 bp, one of 20 kbp, a chimera of 70 kbp plus three short
pieces, three reads of 70 kbp, the gap read, the reads across the two runs,
reads of 0 and 1 bp and 100 reads of 150 bp.  What these inputs reach (query
offsets past 2^16, more than 2048 intervals and 512 calls in a read, chains of
200 seeds, a chain weight past 2^16, max_chain_gap deciding) is asserted on
the CPU by tests/test_long_reads.py::test_inputs_reach_the_paths.
"""
import ctypes as C

import numpy as np
import pytest

import long_reads as LR
from tests import golden_data
from test_gpu_parity import OPTS
from test_gpu_product import _collect, _pack
from test_gpu_seed_phases import _assert_stream
from test_gpu_stream import _joined

pytestmark = pytest.mark.gpu

CHAIN_OPTS = {
    "std": dict(),
    "gap20000": dict(max_chain_gap=20000),
    "w5gap1000": dict(w=5, max_chain_gap=1000),
}
CHAIN_ENVS = {
    "default": dict(),
    "all-wave": dict(SMEM_CHAIN_HEAVY_MIN="0"),
    "all-lane": dict(SMEM_CHAIN_HEAVY_MIN="100000"),
    "serial-sort": dict(SMEM_CHAIN_SERIAL_SORT="1"),
    "lds-overflow": dict(SMEM_CHAIN_LDS="2048"),
    "tree-only": dict(SMEM_CHAIN_TREE_ONLY="1"),
}


@pytest.fixture(scope="module")
def world(gpu_device):
    import smemgpu
    w = LR.world()
    gpu = smemgpu.Gpu(w["idx"], device=gpu_device)
    gpu.load_sa(w["sa"])
    gpu.load_pac(_pack(w["g"]), int(w["g"].size))
    yield dict(w, gpu=gpu, device=gpu_device)
    gpu.close()


def _want(world, key, reads, optname="default"):
    return LR.seed_truth(LR.world(), key, reads, **OPTS[optname])


def _seed(gpu, reads, optname="default", max_len=None):
    """one batch made for exactly these reads -> (results, stats)"""
    import smemgpu
    b = gpu.batch(max(1, reads.n), max(16, reads.codes.size), max_len or max(1, int(reads.lens.max())))
    try:
        b.set_reads(reads.codes, reads.offs)
        b.run(smemgpu.Options(**OPTS[optname]))
        st = b.stats()
        return b.fetch(), st
    finally:
        b.close()


def _default_cap(max_len):
    return max(32, max_len // 2 + 32)   # smem_batch_create's output capacity per read


# ------------------------------------------------------------------ seeding
@pytest.mark.parametrize("optname", list(OPTS))
def test_seed_whole_set(world, optname):
    """The whole set in one batch: one read of 70 kbp sets the capacity and the arena size of 100 reads
    of 150 bp.  (Under `noexact` the four reads of 70 kbp have more intervals than that capacity,
    40,937-42,177 against 35,381, and go through the overflow pass; under the other sets no read does.)"""
    reads = world["reads"]
    want, per, _ = _want(world, "all", reads, optname)
    res, st = _seed(world["gpu"], reads, optname)
    fits = bool((per["n_intv"] <= _default_cap(int(reads.lens.max()))).all())
    assert fits == (optname != "noexact")
    assert (st["n_overflow"] == 0) == fits
    _assert_stream(res, want)


def test_seed_default_capacity_holds(world):
    """Under the default options no read of the set needs more than the default capacity (the CPU test
    asserts that of the inputs), so none goes through the overflow pass."""
    reads = world["reads"]
    want, per, _ = _want(world, "all", reads)
    assert (per["n_intv"] <= _default_cap(int(reads.lens.max()))).all()
    res, st = _seed(world["gpu"], reads)
    assert st["n_overflow"] == 0
    _assert_stream(res, want)


def test_seed_reverse_order(world):
    """The same reads last to first: the short reads are claimed first and the longest reads last."""
    reads = world["reads"]
    rev = reads.subset(np.arange(reads.n - 1, -1, -1))
    want, _, _ = _want(world, "reversed", rev)
    res, st = _seed(world["gpu"], rev)
    assert st["n_overflow"] == 0
    _assert_stream(res, want)


def _classes():
    """length -> how the synthetic set names it; the read of 0 bp goes with the read of 1 bp (a batch's
    max_len is at least 1)"""
    return sorted(set(LR.CLASS_LENGTHS) | {1, 150, 2000, 5000, LR.LONG_LEN, 27000, 70000, "chimera"}, key=str)


@pytest.mark.parametrize("cls", _classes(), ids=str)
def test_seed_length_class_alone(world, cls):
    """Each length alone in a batch created with exactly its own max_len: cap_list = max_len + 2 and
    the capacity max_len / 2 + 32 take that length's values."""
    reads, names = world["reads"], world["names"]
    if cls == "chimera":
        pick = [names.index("chimera")]
    else:
        pick = [i for i in range(reads.n) if int(reads.lens[i]) == cls or (cls == 1 and reads.lens[i] == 0)]
    assert pick
    sub = reads.subset(pick)
    max_len = int(sub.lens.max())
    assert max_len == (cls if cls != "chimera" else int(reads.lens[pick[0]]))
    want, per, _ = _want(world, ("class", cls), sub)
    assert (per["n_intv"] <= _default_cap(max_len)).all()
    res, st = _seed(world["gpu"], sub, max_len=max_len)
    assert st["n_overflow"] == 0
    _assert_stream(res, want)


@pytest.fixture(scope="module")
def g1(gpu_device, tmp_path_factory):
    import smemgpu
    p = golden_data.files("g1", str(tmp_path_factory.mktemp("g1long")))
    gpu = smemgpu.Gpu(smemgpu.Index.read(p["bwt"]), device=gpu_device)
    gpu.load_sa(smemgpu.SA.read(p["sa"]))
    reads, names = golden_data.long_reads()
    yield dict(gpu=gpu, reads=reads, names=names, case=golden_data.long_case())
    gpu.close()


def test_fixture_every_stage(g1):
    """The r5 reads on the g1 index: lists, positions and chains (unfiltered, filtered) equal the
    compiled reference's streams."""
    import smemgpu
    reads, case = g1["reads"], g1["case"]
    b = g1["gpu"].batch(reads.n, reads.codes.size, int(reads.lens.max()))
    try:
        b.set_reads(reads.codes, reads.offs)
        b.run(smemgpu.Options(**case["opt"]))
        b.sa(case["opt"]["min_seed_len"], case["max_occ"])
        res = b.fetch()
        assert res.to_smgo() == golden_data.long_smgo()
        assert res.to_smsa() == golden_data.long_smsa()
        assert b.stats()["n_occ"] == case["n_occ"]
        for filt in (0, 1):
            ch = next(c for c in case["chains"] if c["filter"] == filt)
            b.chain(golden_data.l_pac("g1"), w=ch["w"], max_chain_gap=ch["max_chain_gap"],
                    mask_level=ch["mask_level"], drop_ratio=ch["drop_ratio"], filter=bool(filt))
            assert b.fetch().to_smch() == golden_data.long_smch(filt), filt
    finally:
        b.close()


# ----------------------------------------------------------------- overflow
@pytest.mark.parametrize("intv_cap", [2, 64])
def test_overflow_rounds(world, intv_cap):
    """A capacity of 2 (64) records: the reads of thousands of intervals go through the overflow pass,
    whose rounds hold 8, 32, 128, 512, 2048 and 8192 (256, 1024, 4096 and 16384) records: six (four)
    rounds for the read of more than 2048 (4096) intervals."""
    import smemgpu
    reads = world["reads"]
    want, per, _ = _want(world, "all", reads)
    assert int(per["n_intv"].max()) > intv_cap * 4 ** (5 if intv_cap == 2 else 3)
    gpu = smemgpu.Gpu(world["idx"], device=world["device"], intv_cap=intv_cap)
    try:
        res, st = _seed(gpu, reads)
    finally:
        gpu.close()
    assert st["n_overflow"] > 0
    _assert_stream(res, want)


# -------------------------------------------------------------- slot growth
def test_collect_slot_regrown(world):
    """One handle, one smem_gpu_collect_ex slot: 150 bp reads, then the whole set (the slot's batch is
    re-created for the longer max_len), then the 150 bp reads again on the grown batch."""
    import smemgpu
    from smemgpu.lib import _results_of
    lib = smemgpu.load()
    reads = world["reads"]
    fill = reads.subset([i for i in range(reads.n) if reads.lens[i] == 150])
    want_fill, _, _ = _want(world, ("class", 150), fill)
    want_all, _, _ = _want(world, "all", reads)
    gpu = smemgpu.Gpu(world["idx"], device=world["device"])
    try:
        for rd, want in ((fill, want_fill), (reads, want_all), (fill, want_fill)):
            rc, bh, keep = _collect(lib, gpu._h, 0, rd, 0, rd.n)
            assert rc == 0, smemgpu.lib.ERRORS.get(rc, rc)
            _assert_stream(_results_of(lib, bh, rd.n), want)
        assert gpu.memory()["batches"] == 1
    finally:
        gpu.close()


def test_batch_create_max_len_limit(world):
    import smemgpu
    with pytest.raises(smemgpu.SmemError, match="SMEM_E_ARG"):
        world["gpu"].batch(1, 64, (1 << 24) + 1)


# ---------------------------------------------------------------- streaming
def _upto(reads, n):
    return reads.subset([i for i in range(reads.n) if reads.lens[i] <= n])


@pytest.mark.parametrize("packed", [True, False], ids=["packed", "unpacked"])
@pytest.mark.parametrize("chunk", [1, 7])
def test_stream_up_to_8191(world, chunk, packed):
    """The reads of at most 8191 bp through smem_gpu_seed_stream; packed, the 13-bit query fields carry
    a begin with bit 12 set and the end 8191."""
    import smemgpu
    sub = _upto(world["reads"], 8191)
    assert int(sub.lens.max()) == 8191
    want, _, _ = _want(world, "upto8191", sub)
    st, chunks = world["gpu"].seed_stream(sub.codes, sub.offs, smemgpu.Options(), chunk_reads=chunk, workers=3,
                                          collect=True, packed=packed)
    assert st["n_reads"] == sub.n and st["n_chunks"] == (sub.n + chunk - 1) // chunk
    got = _joined(chunks, sub.n)
    assert got.to_smgo() == want
    if packed:
        assert (got.intv[:, 3] >> np.uint64(32)).max() >= 4096
        assert ((got.intv[:, 3] & np.uint64(0xFFFFFFFF)) == 8191).any()


def test_stream_8192_packed_refused(world):
    """One read of 8192 bp more: packed mode refuses the call before any chunk is delivered; unpacked
    takes the same set."""
    import smemgpu
    from smemgpu.lib import CHUNK_FN, StreamStats
    lib = smemgpu.load()
    reads = world["reads"]
    first_8192 = next(i for i in range(reads.n) if reads.lens[i] == 8192)
    sub = reads.subset([i for i in range(reads.n) if reads.lens[i] <= 8191 or i == first_8192])
    assert int(sub.lens.max()) == 8192 and int((sub.lens == 8192).sum()) == 1
    delivered = []

    def on_chunk(ctx, chunk, first, n, bh):
        delivered.append(int(chunk))
        return 0

    cb = CHUNK_FN(on_chunk)
    codes = np.ascontiguousarray(sub.codes, dtype=np.uint8)
    offs = np.ascontiguousarray(sub.offs, dtype=np.uint64)
    o, st = smemgpu.Options().c(), StreamStats()
    rc = lib.smem_gpu_seed_stream(world["gpu"]._h, sub.n, codes.ctypes.data, offs.ctypes.data, C.byref(o), 7, 3,
                                  2, C.cast(cb, C.c_void_p), None, C.byref(st))   # 2: SMEM_STREAM_PACKED
    assert smemgpu.lib.ERRORS.get(rc) == "SMEM_E_ARG" and delivered == []
    want, _, _ = _want(world, "upto8191plus", sub)
    _, chunks = world["gpu"].seed_stream(sub.codes, sub.offs, smemgpu.Options(), chunk_reads=7, workers=3,
                                         collect=True, packed=False)
    assert _joined(chunks, sub.n).to_smgo() == want


def test_stream_whole_set_unpacked(world):
    import smemgpu
    reads = world["reads"]
    want, _, _ = _want(world, "all", reads)
    _, chunks = world["gpu"].seed_stream(reads.codes, reads.offs, smemgpu.Options(), chunk_reads=7, workers=3,
                                         collect=True, packed=False)
    assert _joined(chunks, reads.n).to_smgo() == want


# ---------------------------------------------------------------- SA lookup
@pytest.mark.parametrize("raw", [False, True], ids=["dense", "raw"])
@pytest.mark.parametrize("max_occ", [500, 10000])
def test_sa_lookup(world, max_occ, raw, monkeypatch):
    """bwt_sa of every seed occurrence of the whole set: positions and per-read counts, from the
    densified SA and (SMEM_GPU_SA_RAW=1) from the walk to the uploaded samples."""
    import smemgpu
    if raw:
        monkeypatch.setenv("SMEM_GPU_SA_RAW", "1")
    reads = world["reads"]
    gpu = smemgpu.Gpu(world["idx"], device=world["device"])
    try:
        gpu.load_sa(world["sa"])
        b = gpu.batch(reads.n, reads.codes.size, int(reads.lens.max()))
        b.set_reads(reads.codes, reads.offs)
        b.run()
        b.sa(19, max_occ)
        res = b.fetch()
        b.close()
    finally:
        gpu.close()
    counts, pos = LR.sa_truth(world["oi"], world["osa"], [res.read_calls(i) for i in range(reads.n)], 19, max_occ)
    assert np.array_equal(res.sa_pos, np.concatenate(pos))
    assert [res.read_sa(i).size for i in range(reads.n)] == counts.tolist()


# ----------------------------------------------------------------- chaining
@pytest.fixture(scope="module")
def chained(world):
    """the whole set seeded and looked up once (max_occ 10000) on one batch, its lists compared with the
    restatement's; the restatement's chains per (option set, filter), made once"""
    from test_gpu_chain import _oracle_chains
    reads = world["reads"]
    b = world["gpu"].batch(reads.n, reads.codes.size, int(reads.lens.max()))
    b.set_reads(reads.codes, reads.offs)
    b.run()
    b.sa(19, 10000)
    res = b.fetch()
    want, _, _ = _want(world, "all", reads)
    _assert_stream(res, want)
    truth = {}

    def chains(oname, filt):
        if (oname, filt) not in truth:
            truth[(oname, filt)] = _oracle_chains(res, reads.n, world["l_pac"], 19, 10000, filter=filt,
                                                  **CHAIN_OPTS[oname])
        return truth[(oname, filt)]

    yield dict(b=b, chains=chains)
    b.close()


@pytest.mark.parametrize("env", list(CHAIN_ENVS))
@pytest.mark.parametrize("oname", list(CHAIN_OPTS))
def test_chain_vs_oracle(world, chained, monkeypatch, oname, env):
    """mem_chain and mem_chain_flt of the whole set on every chaining path.  The chimera's chain weight
    is past 2^16: on the wave paths (default, all-wave) its filter sort takes the serial branch that
    the packed 16-bit key cannot serve."""
    for k, v in CHAIN_ENVS[env].items():
        monkeypatch.setenv(k, v)
    b = chained["b"]
    for filt in (0, 1):
        b.chain(world["l_pac"], filter=bool(filt), **CHAIN_OPTS[oname])
        res = b.fetch(4)   # FETCH_CHAINS
        assert res.to_smch() == chained["chains"](oname, filt), filt


def test_chain2aln_refused_chains_kept(world, chained):
    """chains -> regions takes reads up to 1024 bp: this batch is refused, and its chains stay as they
    were."""
    import smemgpu
    from oracle import oracle
    b = chained["b"]
    b.chain(world["l_pac"], filter=True)
    before = b.fetch(4).to_smch()
    assert before == chained["chains"]("std", 1)
    with pytest.raises(smemgpu.SmemError, match="1024"):
        b.chain2aln(oracle.aln_opt())
    assert b.fetch(4).to_smch() == before
