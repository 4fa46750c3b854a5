"""Chains -> alignment regions: the loop of
mem_align1_core over every read's chains (software/bwamem.c:1452-1460),
mem_chain2aln_short (software/bwamem.c:805-852, ksw_align2) and, when it
declines, mem_chain2aln (software/bwamem.c:1040-1188, ksw_extend2 both ways).

Bar: bit-exact — per read, every region's rb / re / qb / qe / score / truesc /
csub / w / seedcov in the reference's order.  The restatement
(oracle/aln_oracle.c) is pinned to the compiled reference's own regions
(tests/golden/*.smrg.gz, `ref_harness aln`) over the reference's own
filtered chains (the matching *.smch.gz); the GPU path (smem_chain2aln,
through the C ABI) is checked against the same fixtures and against the
restatement on larger repeat-rich genomes with chains from the GPU chain stage.

Non-default extension options (bwa mem -d / -L / -B / -O / -E / -A / -w / -k):
`ref_harness aln` takes the nine scoring fields, and the read sets r3 / r4
(tests/aln_reads.py: indels, unrelated stretches, mismatched ends, unrelated
tails) pin the restatement and the GPU to the reference under 16 option sets;
test_option_fixtures_bite holds those fixtures to deciding something; fresh
problems of the same mix, the ends of the forward-reverse text and the
145-160-column gap queue run against the restatement on all three routes.
"""
import numpy as np
import pytest

from oracle import oracle
from tests import aln_reads, golden_data

FIX = golden_data.aln_fixtures()
OPT_FIX = [f for f in FIX if "reads" in f]   # the r3 / r4 read sets under each option set of tests/aln_reads.py
FIELDS = ["rb", "re", "qb", "qe", "score", "truesc", "sub", "csub", "sub_n", "w", "seedcov", "secondary"]


def _case_inputs(fix):
    chains, chain_off, seeds = golden_data.smch_parse(golden_data.aln_chains(fix))
    reads = golden_data.aln_reads(fix)
    assert chain_off.size == reads.n + 1
    return reads, chains, chain_off, seeds


def _fix_opt(fix):
    """the fixture's mem_opt_t fields: every one from the manifest where it
    carries them (the r3 / r4 option sets), else w and min_seed_len"""
    if "opt" in fix:
        return oracle.aln_opt(**fix["opt"])
    return oracle.aln_opt(w=fix["w"], min_seed_len=fix["min_seed_len"])


def _assert_same(got, got_off, want, want_off):
    assert np.array_equal(np.asarray(got_off, dtype=np.uint64), np.asarray(want_off, dtype=np.uint64))
    for f in FIELDS:
        bad = np.nonzero(got[f] != want[f])[0]
        assert bad.size == 0, f"field {f}: {bad.size} regions differ, first {bad[:5]}"


def test_aln_fixtures_present():
    assert len(FIX) >= 4
    assert {f["genome"] for f in FIX} == {"g1", "g2"}


@pytest.mark.parametrize("fix", FIX, ids=[f["file"].split(".")[0] for f in FIX])
def test_aln_oracle_vs_reference(fix):
    """restatement == the reference's mem_chain2aln loop, region for region"""
    reads, chains, chain_off, seeds = _case_inputs(fix)
    want, want_off = golden_data.smrg_parse(golden_data.smrg(fix))
    assert want.size > 0
    got, got_off = oracle.aln(golden_data.pac(fix["genome"]), golden_data.l_pac(fix["genome"]), reads.codes,
                              reads.offs, chains, chain_off, seeds, _fix_opt(fix))
    _assert_same(got, got_off, want, want_off)


def _per_read(fix, n):
    """the fixture's regions of its first n reads, one bytes object per read"""
    regs, off = golden_data.smrg_parse(golden_data.smrg(fix))
    cols = regs[["rb", "re", "qb", "qe", "score", "truesc", "w"]]
    return [cols[int(off[i]):int(off[i + 1])].tobytes() for i in range(n)]


def test_option_fixtures_bite():
    """Judged by the reference's own files only: under every option set at
    least 20 reads have a region list that differs from the `default` fixture
    of the same reads (another count, or another rb / re / qb / qe / score /
    truesc / w); d0 and d20 differ from default (z-drop decides on these
    reads, which it never does on r1 / r2), and L0_9 and L9_0 differ from each
    other on at least 20 reads (a 5' / 3' swap cannot pass)."""
    for rname in ("r3", "r4"):
        by = {f["name"]: f for f in OPT_FIX if f["reads"] == rname}
        assert set(by) == set(aln_reads.OPTION_SETS), (rname, sorted(set(aln_reads.OPTION_SETS) - set(by)))

        def differ(a, b):
            n = min(by[a]["n_reads"], by[b]["n_reads"])
            return sum(x != y for x, y in zip(_per_read(by[a], n), _per_read(by[b], n)))

        for name in by:
            assert by[name]["opt"] == aln_reads.full_options(name)
            if name != "default":
                d = differ(name, "default")
                print(f"{rname} {name}: {d} reads differ from default")
                assert d >= 20, (rname, name, d)
        d = differ("L0_9", "L9_0")
        print(f"{rname} L0_9 / L9_0: {d} reads differ")
        assert d >= 20, (rname, d)


_HEAVY = [(None, "default"), ("1", "all_heavy"), ("1000:2", "seed_heavy"), ("1+nocand", "all_heavy_bin_hash")]


@pytest.mark.gpu
@pytest.mark.parametrize("fix,heavy", [pytest.param(f, h, id=f["file"].split(".")[0] + "-" + hid)
                                       for f in FIX for h, hid in (_HEAVY[:2] if "reads" in f else _HEAVY)])
def test_aln_gpu_vs_reference(gpu_device, fix, heavy, monkeypatch):
    """heavy = "1": every read takes the heavy-read path (regions computed
    ahead per chain, then the read's walk), SMEM_ALN_HEAVY_MIN.  The r3 / r4
    option fixtures run at default and "1": the light reads' lane engine
    (RegionPol) and the one-wave-per-seed copy (seed_region) each read
    pen_clip5 / pen_clip3 / zdrop / w on their own."""
    _heavy_env(monkeypatch, heavy)
    import smemgpu
    from smemgpu import synth
    reads, chains, chain_off, seeds = _case_inputs(fix)
    want, want_off = golden_data.smrg_parse(golden_data.smrg(fix))
    idx = smemgpu.Index.read(golden_data.files(fix["genome"], _tmpdir())["bwt"])
    gpu = smemgpu.Gpu(idx, device=gpu_device)
    try:
        raw, off, ms = gpu.chain2aln(golden_data.pac(fix["genome"]), golden_data.l_pac(fix["genome"]), reads.codes,
                                     reads.offs, chains, chain_off, seeds, _fix_opt(fix))
    finally:
        gpu.close()
    got = np.frombuffer(raw.tobytes(), dtype=golden_data.ALNREG_DT)
    _assert_same(got, off, want, want_off)
    del synth


def _heavy_env(monkeypatch, heavy):
    """heavy = "min[:seeds]": SMEM_ALN_HEAVY_MIN / SMEM_ALN_HEAVY_SEEDS, the
    chain / seed counts from which a read takes the heavy-read path; its walk
    then tests containment through the candidate index, or, with "+nocand"
    (SMEM_ALN_CAND=0), always through the region bin hash (SMEM_ALN_HASH_MIN
    = 1).  A "/1"
    suffix: the light and heavy reads' kernels one after the other on the
    batch's stream (SMEM_ALN_STREAMS=1) instead of side by side."""
    while heavy and "+" in heavy:
        heavy, _, opt = heavy.rpartition("+")
        if opt == "inline":
            # the heavy-read walk inlined into its kernel (the round-2 hang's
            # shape), every loop iteration counted against a guard: a walk that
            # would spin fails the call instead of hanging
            monkeypatch.setenv("SMEM_ALN_WALK_INLINE", "1")
        elif opt == "nolane":
            # no regions computed ahead one seed per lane (SMEM_ALN_LANE=0)
            monkeypatch.setenv("SMEM_ALN_LANE", "0")
        elif opt == "nocand":
            # the heavy walk without the candidate index (the bin hash of the
            # regions made so far)
            monkeypatch.setenv("SMEM_ALN_CAND", "0")
        elif opt.startswith("giants"):
            # the giant split's size (SMEM_ALN_GIANTS; 0: off): the heaviest heavy reads'
            # passes, candidate index and walk on the batch's third stream
            monkeypatch.setenv("SMEM_ALN_GIANTS", opt[len("giants"):])
        elif opt.startswith("gfirst"):
            # whose passes wait for the giants' (SMEM_ALN_GIANT_FIRST 0 / 1 / 2)
            monkeypatch.setenv("SMEM_ALN_GIANT_FIRST", opt[len("gfirst"):])
    if heavy and "/" in heavy:
        heavy, _, streams = heavy.partition("/")
        monkeypatch.setenv("SMEM_ALN_STREAMS", streams)
    if heavy:
        m, _, sd = heavy.partition(":")
        monkeypatch.setenv("SMEM_ALN_HEAVY_MIN", m)
        if sd:
            monkeypatch.setenv("SMEM_ALN_HEAVY_SEEDS", sd)
        monkeypatch.setenv("SMEM_ALN_HASH_MIN", "1")  # every heavy walk through the bin hash


def _tmpdir():
    import tempfile
    return tempfile.mkdtemp()


def _pack(codes):
    """2-bit forward strand as bns_fasta2bntseq packs it (software/bntseq.c:303-309)"""
    c = np.asarray(codes, dtype=np.uint8)
    c = np.where(c > 3, 0, c).astype(np.uint8)
    pad = (-c.size) % 4
    c = np.concatenate([c, np.zeros(pad, dtype=np.uint8)]).reshape(-1, 4)
    return (c[:, 0] << 6 | c[:, 1] << 4 | c[:, 2] << 2 | c[:, 3]).astype(np.uint8)


def test_pack_matches_reference_pac():
    """the test-side packer gives bwa_index's .pac on the golden genomes (no N)"""
    import gzip
    import os
    for g in ("g1", "g2"):
        with gzip.open(os.path.join(golden_data.GOLDEN, g + ".fa.gz"), "rb") as fh:
            codes = golden_data.fasta_codes(fh.read())
        assert np.array_equal(_pack(codes), golden_data.pac(g))


@pytest.mark.gpu
@pytest.mark.parametrize("w,a,heavy", [(100, 1, None), (20, 1, None), (100, 2, None), (100, 1, "1"), (100, 2, "1"),
                                       (20, 1, "3"), (100, 1, "0"), (100, 1, "1000:3"), (100, 1, "3/1"),
                                       (100, 1, "1+inline"), (100, 2, "3+inline"), (100, 1, "0+nolane"),
                                       (100, 1, "1+nolane"), (100, 2, "3+nolane"), (100, 1, "1+nocand"),
                                       (100, 2, "3+nocand"), (100, 1, "1+giants0"), (100, 1, "1+giants7"),
                                       (100, 2, "3+giants64+gfirst0"), (100, 1, "1+giants100000+gfirst1")])
def test_aln_gpu_vs_oracle_repeat_dense(gpu_device, w, a, heavy, monkeypatch):
    """600 kbp, 60 % diverged repeat copies; 4000 reads of 70..700 bp (both
    kernel instantiations) with substitutions and Ns; chains from the GPU
    chain stage; GPU regions == restatement, through the host API
    (smem_chain2aln, explicit .pac and resident .pac) and the device-resident
    batch stage (smem_batch_chain2aln over the chains left in HBM).  a = 2
    (-A 2 scaling, b 8, gaps 12 + 2) sends the short path's longer queries
    through ksw_align2's 16-bit branch.  heavy: SMEM_ALN_HEAVY_MIN (1: every
    read through the heavy-read path, 3: reads with 3+ chains, 0: none,
    1000:3 reads with 3+ seeds); giants<N>: the giant split's size (0: off,
    100000: every heavy read), gfirst<K>: whose passes wait for the giants'."""
    _heavy_env(monkeypatch, heavy)
    import smemgpu
    from smemgpu import synth
    g = synth.make_genome(600_000, seed=91, repeat_frac=0.6, n_families=5, exact_frac=0.01, tandem_frac=0.01)
    idx, sa = smemgpu.Index.build_sa(g.codes, sa_intv=32)
    gpu = smemgpu.Gpu(idx, device=gpu_device)
    try:
        gpu.load_sa(sa)
        reads = synth.concat_reads([synth.make_reads(g.codes, 2000, 150, seed=92, sub_rate=0.02),
                                    synth.make_reads(g.codes, 1000, (70, 250), seed=93, n_rate=0.01, sub_rate=0.03),
                                    synth.make_reads(g.codes, 600, (257, 700), seed=94, sub_rate=0.02),
                                    synth.make_reads(g.codes, 400, 101, seed=95, random_frac=0.3)])
        opt = oracle.aln_opt(w=w) if a == 1 else oracle.aln_opt(w=w, a=2, b=8, o_del=12, e_del=2, o_ins=12, e_ins=2)
        pac = _pack(g.codes)
        l_pac = int(g.codes.size)
        gpu.load_pac(pac, l_pac)
        b = gpu.batch(reads.n, reads.codes.size, int(reads.lens.max()))
        try:
            b.set_reads(reads.codes, reads.offs)
            b.run(smemgpu.Options())
            b.sa(19, 10000)
            b.chain(l_pac, w=w)
            b.chain2aln(opt)   # device-resident: chains, seeds, reads and .pac already in HBM
            res = b.fetch()
            chains, chain_off, seeds = res.chains, res.chain_off, res.seeds
            assert b.stats()["n_regs"] == int(res.reg_off[-1])
        finally:
            b.close()
        raw, off, ms = gpu.chain2aln(pac, l_pac, reads.codes, reads.offs, chains, chain_off, seeds, opt)
        raw2, off2, _ = gpu.chain2aln(None, l_pac, reads.codes, reads.offs, chains, chain_off, seeds, opt)
    finally:
        gpu.close()
    want, want_off = oracle.aln(pac, l_pac, reads.codes, reads.offs, chains, chain_off, seeds, opt)
    assert want.size > 1000
    for r, o in ((raw, off), (raw2, off2), (res.regs, res.reg_off)):
        got = np.frombuffer(r.tobytes(), dtype=golden_data.ALNREG_DT)
        _assert_same(got, o, want, want_off)


@pytest.mark.gpu
@pytest.mark.parametrize("o_del,o_ins", [(6, 0), (0, 0)], ids=["o_ins0", "o_del0_o_ins0"])
def test_aln_gpu_vs_oracle_gap_open_0(gpu_device, o_del, o_ins):
    """Gap open 0 (bwa mem -O 6,0 and -O 0,0): with o_ins = 0 the reference's
    ksw_align2 carries F across a block of its striped query into one column
    only (tests/test_ksw_align.py), and the regions go into SAM as they are.
    200 kbp, 1000 reads with 3 % indels and one longer insertion each, half
    150 bp and half 257..500 bp, and 500 reads whose only match is a stretch of
    45..95 bp between unrelated flanks: a chain that short inside a read is what
    mem_chain2aln_short takes (software/bwamem.c:825-836).  GPU regions ==
    restatement on all three routes of test_aln_gpu_vs_oracle_repeat_dense."""
    import smemgpu
    from smemgpu import synth
    g = synth.make_genome(200_000, seed=96, repeat_frac=0.6, n_families=5, exact_frac=0.01, tandem_frac=0.01)
    idx, sa = smemgpu.Index.build_sa(g.codes, sa_intv=32)
    src = synth.concat_reads([synth.make_reads(g.codes, 500, 150, seed=97, sub_rate=0.02),
                              synth.make_reads(g.codes, 500, (257, 500), seed=98, sub_rate=0.02)])
    rng = np.random.default_rng(99)
    parts = []
    for i in range(src.n):
        r = synth._mutated_copy(src.read(i), rng, 0.0, 0.03)
        at = int(rng.integers(1, r.size))
        parts.append(np.concatenate([r[:at], rng.integers(0, 4, size=int(rng.integers(2, 7))).astype(np.uint8),
                                     r[at:]]))
    for i in range(500):
        n = int(rng.integers(45, 96))
        pos = int(rng.integers(0, g.codes.size - n))
        r = synth._mutated_copy(g.codes[pos:pos + n], rng, 0.01, 0.03)
        at = int(rng.integers(r.size // 4, 3 * r.size // 4))
        r = np.concatenate([r[:at], rng.integers(0, 4, size=int(rng.integers(2, 7))).astype(np.uint8), r[at:]])
        if i % 2:
            r = (3 - r)[::-1]
        parts.append(np.concatenate([rng.integers(0, 4, size=int(rng.integers(70, 200))), r,
                                     rng.integers(0, 4, size=int(rng.integers(70, 200)))]).astype(np.uint8))
    lens = np.array([p.size for p in parts], dtype=np.int32)
    reads = synth.Reads(lens, np.concatenate(parts).astype(np.uint8),
                        np.concatenate([[0], np.cumsum(lens, dtype=np.int64)]))
    opt = oracle.aln_opt(o_del=o_del, o_ins=o_ins)
    pac = _pack(g.codes)
    l_pac = int(g.codes.size)
    gpu = smemgpu.Gpu(idx, device=gpu_device)
    try:
        gpu.load_sa(sa)
        gpu.load_pac(pac, l_pac)
        b = gpu.batch(reads.n, reads.codes.size, int(reads.lens.max()))
        try:
            b.set_reads(reads.codes, reads.offs)
            b.run(smemgpu.Options())
            b.sa(19, 10000)
            b.chain(l_pac)
            b.chain2aln(opt)
            res = b.fetch()
            chains, chain_off, seeds = res.chains, res.chain_off, res.seeds
        finally:
            b.close()
        raw, off, ms = gpu.chain2aln(pac, l_pac, reads.codes, reads.offs, chains, chain_off, seeds, opt)
        raw2, off2, _ = gpu.chain2aln(None, l_pac, reads.codes, reads.offs, chains, chain_off, seeds, opt)
    finally:
        gpu.close()
    want, want_off = oracle.aln(pac, l_pac, reads.codes, reads.offs, chains, chain_off, seeds, opt)
    assert want.size > 500
    for r, o in ((raw, off), (raw2, off2), (res.regs, res.reg_off)):
        got = np.frombuffer(r.tobytes(), dtype=golden_data.ALNREG_DT)
        _assert_same(got, o, want, want_off)


@pytest.mark.gpu
def test_aln_gpu_argument_checks(gpu_device):
    """The host API refuses query codes > 4 (they would index past the scoring
    matrix), chains sharing seeds (they would share sort scratch), a short
    .pac and a missing resident .pac; the batch stage needs filtered chains."""
    import smemgpu
    from smemgpu import synth
    g = synth.make_genome(50_000, seed=3)
    idx, sa = smemgpu.Index.build_sa(g.codes, sa_intv=32)
    gpu = smemgpu.Gpu(idx, device=gpu_device)
    try:
        gpu.load_sa(sa)
        reads = synth.make_reads(g.codes, 50, 150, seed=4)
        b = gpu.batch(reads.n, reads.codes.size, 150)
        b.set_reads(reads.codes, reads.offs)
        b.run()
        b.sa(19, 10000)
        b.chain(g.codes.size, filter=False)
        with pytest.raises(smemgpu.SmemError):   # unfiltered chains
            b.chain2aln(oracle.aln_opt())
        b.chain(g.codes.size)
        with pytest.raises(smemgpu.SmemError):   # no resident .pac
            b.chain2aln(oracle.aln_opt())
        res = b.fetch()
        b.close()
        opt = oracle.aln_opt()
        pac = _pack(g.codes)
        l_pac = int(g.codes.size)
        with pytest.raises(smemgpu.SmemError):   # no pac given, none resident
            gpu.chain2aln(None, l_pac, reads.codes, reads.offs, res.chains, res.chain_off, res.seeds, opt)
        with pytest.raises(smemgpu.SmemError):   # short pac
            gpu.chain2aln(pac[:10], l_pac, reads.codes, reads.offs, res.chains, res.chain_off, res.seeds, opt)
        bad = reads.codes.copy()
        bad[5] = 7
        with pytest.raises(smemgpu.SmemError):   # code > 4
            gpu.chain2aln(pac, l_pac, bad, reads.offs, res.chains, res.chain_off, res.seeds, opt)
        ch = res.chains.copy()
        k = int(np.nonzero(ch["n"] > 0)[0][1])
        ch["seed_off"][k] = ch["seed_off"][int(np.nonzero(ch["n"] > 0)[0][0])]
        with pytest.raises(smemgpu.SmemError):   # chains sharing seeds
            gpu.chain2aln(pac, l_pac, reads.codes, reads.offs, ch, res.chain_off, res.seeds, opt)
    finally:
        gpu.close()


# ---- non-default extension options: fresh problems against the restatement ----
OPTION_NAMES = list(aln_reads.OPTION_SETS)


def _reads_of(parts):
    from smemgpu import synth
    lens = np.array([p.size for p in parts], dtype=np.int32)
    return synth.Reads(lens, np.concatenate(parts).astype(np.uint8),
                       np.concatenate([[0], np.cumsum(lens, dtype=np.int64)]))


def _rc(r):
    return (3 - np.asarray(r, dtype=np.uint8))[::-1].astype(np.uint8)


@pytest.fixture(scope="module")
def opt_world(gpu_device):
    """One 200 kbp genome, half of it repeat copies, one record; its index, SA
    and .pac resident on one device handle for the module; the restatement's
    regions are kept per problem (want), computed once."""
    import smemgpu
    from smemgpu import synth
    g = synth.make_genome(200_000, seed=131, repeat_frac=0.5, n_chrom=1)
    idx, sa = smemgpu.Index.build_sa(g.codes, sa_intv=32)
    gpu = smemgpu.Gpu(idx, device=gpu_device)
    gpu.load_sa(sa)
    pac = _pack(g.codes)
    gpu.load_pac(pac, int(g.codes.size))
    G = g.codes
    reads = synth.concat_reads([aln_reads.option_reads(G, 500, 132, len_range=(150, 150), n_long=0),
                                aln_reads.option_reads(G, 640, 133, len_range=(70, 250), n_long=50,
                                                       long_range=(257, 700)),
                                # 690..700 bp, nearly clean: at a = 100 their right extensions start past 16 bits
                                _reads_of([aln_reads.one_read(G, np.random.default_rng(134 + i), "ends", 690 + i)
                                           for i in range(10)])])
    w = dict(G=G, gpu=gpu, pac=pac, l_pac=int(G.size), reads=reads, want={})
    yield w
    gpu.close()


def _routes(world, reads, oname, key):
    """Seeding -> filtered chains on the GPU under the option set's
    min_seed_len and w, then the regions on the three routes (device-resident
    batch stage, host API with an explicit .pac, host API with the resident
    one), each asserted equal to the restatement over the same chains.
    Returns (restatement regions, reg_off, chains, chain_off, seeds)."""
    import smemgpu
    o = aln_reads.full_options(oname)
    opt = oracle.aln_opt(**o)
    gpu, pac, l_pac = world["gpu"], world["pac"], world["l_pac"]
    b = gpu.batch(reads.n, reads.codes.size, int(reads.lens.max()))
    try:
        b.set_reads(reads.codes, reads.offs)
        b.run(smemgpu.Options(min_seed_len=o["min_seed_len"]))
        b.sa(o["min_seed_len"], 500)
        b.chain(l_pac, w=o["w"])
        b.chain2aln(opt)
        res = b.fetch()
        assert b.stats()["n_regs"] == int(res.reg_off[-1])
    finally:
        b.close()
    chains, chain_off, seeds = res.chains, res.chain_off, res.seeds
    raw, off, _ = gpu.chain2aln(pac, l_pac, reads.codes, reads.offs, chains, chain_off, seeds, opt)
    raw2, off2, _ = gpu.chain2aln(None, l_pac, reads.codes, reads.offs, chains, chain_off, seeds, opt)
    if key not in world["want"]:
        oracle.ext_wide16()
        want, want_off = oracle.aln(pac, l_pac, reads.codes, reads.offs, chains, chain_off, seeds, opt)
        world["want"][key] = (want, want_off, chains.tobytes(), seeds.tobytes(), oracle.ext_wide16())
    want, want_off, ch, sd, wide = world["want"][key]
    assert ch == chains.tobytes() and sd == seeds.tobytes()   # the chain stage gave the chains `want` was made over
    for r, ro in ((res.regs, res.reg_off), (raw, off), (raw2, off2)):
        got = np.frombuffer(r.tobytes(), dtype=golden_data.ALNREG_DT)
        _assert_same(got, ro, want, want_off)
    return want, want_off, chains, chain_off, seeds, wide


@pytest.mark.gpu
@pytest.mark.parametrize("heavy", [None, "1"], ids=["lanes", "all_heavy"])
@pytest.mark.parametrize("oname", OPTION_NAMES)
def test_aln_gpu_vs_oracle_options(opt_world, oname, heavy, monkeypatch):
    """Every option set of tests/aln_reads.py (bwa mem -d / -L / -B / -O / -E /
    -A / -w / -k, values literal) on 1200 reads of its mix: 500 of 150 bp, 640
    of 70..250 bp, 60 of 257..700 bp, either strand.  All FIELDS bit-exact
    against the restatement on the three routes, with the light reads on the
    lane engine (heavy None) and every read on the heavy path ("1").  A100
    (a = b = 100): some extension of at most 256 columns has h0 + qlen * top >
    65535, which the lane engine must refuse (RegionPol::start,
    extend_lane_ok) and leave to the walk."""
    _heavy_env(monkeypatch, heavy)
    want, want_off, _, _, _, wide = _routes(opt_world, opt_world["reads"], oname, ("options", oname))
    print(f"options {oname} heavy={heavy}: {want.size} regions on each of 3 routes, "
          f"{wide} extensions of <= 256 columns past 16 bits")
    assert want.size > 1000
    if oname == "A100":
        assert wide >= 1


@pytest.mark.gpu
@pytest.mark.parametrize("oname", ["default", "L0_9"])
def test_aln_gpu_genome_edges(opt_world, oname):
    """Reads at the ends of the forward-reverse text: unrelated 40 bp before
    G[:110] and after G[-110:] and their reverse complements (chain_span's
    clamps at 0, l_pac and 2 l_pac; a left extension with no reference left,
    tlen 0), G[-80:] + revcomp(G)[:70] (chains on both sides of l_pac),
    islands of 45..95 bp from either end of G between unrelated flanks of
    70..200 bp (chain_short's clamp), and reads of exactly 256, 257, 1023 and
    1024 bp.  The reads of at most 256 bp run once alone (the narrow kernel
    instantiation) and once with the rest; a 1025 bp read, in a call of its
    own, is refused."""
    w = opt_world
    G, l_pac = w["G"], w["l_pac"]
    rng = np.random.default_rng(141)
    junk = lambda n: rng.integers(0, 4, size=int(n)).astype(np.uint8)
    parts = [np.concatenate([junk(40), G[:110]]), np.concatenate([G[-110:], junk(40)])]
    parts += [_rc(p) for p in parts]
    parts += [G[:110].copy(), G[-110:].copy(), _rc(G[:110]), _rc(G[-110:])]
    parts.append(np.concatenate([G[-80:], _rc(G)[:70]]))
    for n in (45, 52, 60, 75, 95):
        for isl in (G[:n], G[-n:], _rc(G[:n]), _rc(G[-n:])):
            parts.append(np.concatenate([junk(rng.integers(70, 201)), isl, junk(rng.integers(70, 201))]))
    short = [p for p in parts if p.size <= 256]
    for n in (256, 257, 1023, 1024):
        for k in range(2):
            pos = int(rng.integers(0, l_pac - n))
            r = G[pos:pos + n].copy()
            hit = rng.random(n) < 0.02
            r[hit] = (r[hit] + 1) & 3
            parts.append(_rc(r) if k else r)
            if n <= 256:
                short.append(parts[-1])
    parts += [G[:256].copy(), _rc(G[-257:])]
    short.append(G[:256].copy())
    _routes(w, _reads_of(short), oname, ("edges_short", oname))
    want, want_off, *_ = _routes(w, _reads_of(parts), oname, ("edges", oname))
    print(f"edges {oname}: {want.size} regions on each of 3 routes")
    assert (want["rb"] == 0).any() and (want["re"] == l_pac).any()
    assert (want["rb"] == l_pac).any() and (want["re"] == 2 * l_pac).any()
    _refuses_1025(w)


def _refuses_1025(w):
    """a read of 1025 bp: chains -> regions refuses the call on both routes"""
    import smemgpu
    reads = _reads_of([w["G"][5000:5150].copy(), w["G"][9000:10025].copy()])
    b = w["gpu"].batch(reads.n, reads.codes.size, 1025)
    try:
        b.set_reads(reads.codes, reads.offs)
        b.run(smemgpu.Options())
        b.sa(19, 500)
        b.chain(w["l_pac"])
        res = b.fetch()
        with pytest.raises(smemgpu.SmemError):
            b.chain2aln(oracle.aln_opt())
    finally:
        b.close()
    with pytest.raises(smemgpu.SmemError):
        w["gpu"].chain2aln(w["pac"], w["l_pac"], reads.codes, reads.offs, res.chains, res.chain_off, res.seeds,
                           oracle.aln_opt())


@pytest.mark.gpu
def test_aln_gpu_lane_gap_queue(opt_world):
    """400 reads of exactly 161 bp seeded with min_seed_len 10: in a batch
    whose longest read is 161 bp (<= LQ_GAP_HI + 1) the 256-column lane tier is
    not launched and the extensions of LQ_GAP_LO..LQ_GAP_HI = 145..160 columns
    leave the lanes for aln_region_rest_kernel (task_key); with one 162 bp
    read appended the same extensions go to the 256-column tier.  Both equal
    the restatement; at least 10 seeds have such an extension."""
    from smemgpu import synth
    w = opt_world
    reads = synth.make_reads(w["G"], 400, 161, seed=151, sub_rate=0.02, n_rate=0.0)
    assert int(reads.lens.max()) == 161
    want, _, chains, chain_off, seeds, _ = _routes(w, reads, "k10", ("gap", 161))
    n_gap = 0
    for r in range(reads.n):
        for c in chains[int(chain_off[r]):int(chain_off[r + 1])]:
            sd = seeds[int(c["seed_off"]):int(c["seed_off"]) + int(c["n"])]
            left, right = sd["qbeg"], 161 - sd["qbeg"] - sd["len"]
            n_gap += int((((left >= 145) & (left <= 160)) | ((right >= 145) & (right <= 160))).sum())
    print(f"gap queue: {want.size} regions, {n_gap} seeds with an extension of 145..160 columns")
    assert n_gap >= 10
    pos = 70_000
    more = synth.concat_reads([reads, _reads_of([w["G"][pos:pos + 162].copy()])])
    want2, *_ = _routes(w, more, "k10", ("gap", 162))
    assert want2.size >= want.size
