"""The default seeding kernel's virtual short entries (seed_wp_kernel SKIP, variant 68; DESIGN.md §5
"Virtual short entries") against the restatement, bit for bit.

A bwt_smem1 call skips the extends of strings of fewer than dp bases, dp chosen (for a read's first calls
and for its re-seeding calls) from the k-mer table's facts (D: the largest level such that every string of D + 1 bases occurs, minsz[L]: the smallest
interval size of level L).  The cases put a call's edges at every distance from 1 to K + 1 of its start:
ambiguous bases, the read's ends, calls that begin within K bases of the read's start, matches that end
at once; on the golden genome (D = 6), a 20 kbp one (D = 5, with a repeat family that makes re-seeding
calls ask for more than minsz[D]), a low-complexity one (2 kbp of one base, 2 kbp of a dinucleotide, 4 kbp
random: the random part alone holds every 5-mer, so D = 4 and most of its reads' strings sit far above
minsz) and one of two letters where the property fails at once (D = 0: the path is off).  Table depths K = 1, 2, D - 1 .. D + 2 and 12; the five option sets of
test_gpu_parity.py and a start width of 3; the overflow pass; repeated launches; batch sizes around a
wave's 24 owners; the plain kernel (variant 49) and the A/B shapes on the same batch.

One case at the size the benchmark runs: 2,000 reads on a 6.2 G-symbol index built for it (about ten
seconds on the GPU), on a handle of its own, which must hold a 12-mer table with D >= 10 and launch the
skipping kernel.
"""
import numpy as np
import pytest

from oracle import oracle

pytestmark = pytest.mark.gpu

OPTS = {
    "default": dict(min_seed_len=19, split_factor=1.5, split_width=10, start_width=1),
    "noexact": dict(min_seed_len=19, split_factor=1.5, split_width=10, start_width=2),
    "k14s20": dict(min_seed_len=14, split_factor=1.5, split_width=20, start_width=1),
    "reseed": dict(min_seed_len=19, split_factor=1.0, split_width=500, start_width=1),
    "k30": dict(min_seed_len=30, split_factor=2.0, split_width=3, start_width=1),
    "width3": dict(min_seed_len=10, split_factor=1.0, split_width=500, start_width=3),
}
OWN = 24       # reads a wave of the default kernel owns
N_COPIES = 30  # of the repeat unit in the small genome


def _level_min(codes, k_max):
    """minsz[L], L = 1..k_max, counted on the text the index holds (both strands), and D."""
    from smemgpu import synth
    t = synth.forward_reverse_text(codes).astype(np.int64)
    mn = [0]
    for L in range(1, k_max + 1):
        if t.size < L:
            mn.append(0)
            continue
        v = np.zeros(t.size - L + 1, np.int64)
        for o in range(L):
            v = v * 4 + t[o:t.size - L + 1 + o]
        mn.append(int(np.bincount(v, minlength=4 ** L).min()))
    d = 0
    while d + 1 <= k_max and mn[d + 1] > 0:
        d += 1
    return mn, max(d - 1, 0)


def _one(arr):
    from smemgpu import synth
    arr = np.asarray(arr, np.uint8)
    return synth.Reads(np.array([arr.size], np.int32), arr, np.array([0, arr.size], np.int64))


def _edge_reads(g, rng, ks, unit=None):
    """Reads whose calls start, stop and meet ambiguous bases at every distance 0..13 of each other."""
    from smemgpu import synth
    parts = []
    for L in sorted({0, 1, 18, 19, 150} | {k + d for k in ks for d in (-1, 0, 1) if k + d >= 0}):
        parts.append(_one(g[700:700 + L]))                        # lengths around every K
    base = g[1200:1260].copy()
    for p in range(0, 15):                                        # an ambiguous base at x + p of the first call
        q = base.copy()
        q[p] = 4
        parts.append(_one(q))
    for p in range(0, 15):                                        # ... and of a later call (x = 31), one left of x
        q = base.copy()
        q[30] = 4
        if p:
            q[30 + p] = 4
        parts.append(_one(q))
    for p in range(1, 15):                                        # a later call starts at x = p < K
        q = g[2000:2080].copy()
        q[p - 1] = 4
        parts.append(_one(q))
    for p in range(1, 15):                                        # a forward match that ends at the read's end,
        q = g[2400:2440].copy()                                   # p bases from x (no backward partner but the N)
        q[40 - p - 1] = 4
        parts.append(_one(q))
    for p in range(1, 15):                                        # a mismatch p bases into the read: calls whose
        q = g[3000:3100].copy()                                   # backward phase reaches i = -1 from x <= p
        q[p] = (q[p] + 1) & 3
        q[p + 20] = (q[p + 20] + 2) & 3
        parts.append(_one(q))
    parts.append(_one(np.full(60, 4)))                            # all N, N at both ends, alternating N
    parts.append(_one(np.concatenate([[4], g[5000:5100], [4]])))
    parts.append(_one(np.where(np.arange(120) % 7 == 0, 4, g[3300:3420])))
    parts.append(_one(np.where(np.arange(120) % 3 == 0, 4, g[3300:3420])))
    for n in (40, 150, 260):                                      # not of the genome: calls end at once
        parts.append(_one(rng.integers(0, 4, n)))
    for n in (30, 150, 400):                                      # tandem repeats: lists beyond 18 and 64 entries
        parts.append(_one(np.zeros(n)))
        parts.append(_one(np.tile([1, 2], n)[:n]))
        parts.append(_one(np.tile([0, 0, 3], n)[:n]))
    if unit is not None:                                          # the repeat family: re-seeds with min_intv = copies + 1
        parts.append(_one(unit))
        parts.append(_one(unit[3:90]))
        u = unit.copy()
        u[50] = (u[50] + 1) & 3
        parts.append(_one(u))
    parts.append(synth.make_reads(g, 120, (1, 200), seed=5, n_rate=0.03, random_frac=0.1))
    parts.append(synth.make_reads(g, 120, 150, seed=6, sub_rate=0.04))
    return synth.concat_reads(parts)


def _genomes():
    out = {}
    rng = np.random.default_rng(77)
    # 20 kbp random with a 100-base unit copied N_COPIES times and a short dinucleotide run
    g = rng.integers(0, 4, 20_000).astype(np.uint8)
    unit = g[100:200].copy()
    for c in range(1, N_COPIES):
        g[100 + 600 * c:200 + 600 * c] = unit
    g[19_000:19_300] = np.tile([1, 2], 150)
    out["rnd20k"] = (g, unit)
    # low complexity: the property fails at once
    lc = np.concatenate([np.zeros(2000, np.uint8), np.tile([1, 2], 1000).astype(np.uint8),
                         rng.integers(0, 4, 4000).astype(np.uint8)])
    out["lowcx"] = (lc, None)
    # two letters: most 2-mers are absent, D = 0
    out["ac8k"] = (rng.integers(0, 2, 8000).astype(np.uint8), None)
    return out


@pytest.fixture(scope="module")
def worlds(gpu_device):
    """Per index: the handle on its default, the restatement's index, the reads and (lazily, once) the
    restatement's streams per option set."""
    import smemgpu
    from tests import golden_data
    ws = {}
    fx = golden_data.load()
    items = {"g1": (None, None)}
    items.update(_genomes())
    for name, (g, unit) in items.items():
        if name == "g1":
            idx, g = fx.index, fx.genome
        else:
            idx = smemgpu.Index.build(g)
        ws[name] = dict(name=name, idx=idx, g=g, unit=unit, truth={}, reads=None,
                        ref=oracle.OracleIndex(words=idx.words, primary=idx.primary, L2=idx.L2))
    yield ws
    for w in ws.values():
        w["ref"].close()


def _reads_of(w, ks=(1, 2, 5, 8, 9, 10, 12)):
    if w["reads"] is None:
        from smemgpu import synth
        rng = np.random.default_rng(3)
        g = w["g"]
        if w["name"] == "g1":  # (an ambiguous base of the FASTA is a random base in the index: never cut there)
            g = np.where(g < 4, g, 0).astype(np.uint8)
        w["reads"] = _edge_reads(g, rng, ks, w["unit"])
    return w["reads"]


def _want(w, optname, reads=None, key=None):
    k = (optname, key)
    if k not in w["truth"]:
        r = _reads_of(w) if reads is None else reads
        w["truth"][k] = oracle.seed(w["ref"], r.codes, r.offs, threads=4, **OPTS[optname])
    return w["truth"][k]


def _diff(got, want):
    from smemgpu import synth
    a, b = synth.read_smgo(got), synth.read_smgo(want)
    bad = [i for i in range(len(b)) if len(a[i]) != len(b[i]) or any(
        x.shape != y.shape or (x != y).any() for x, y in zip(a[i], b[i]))]
    return f"{len(bad)} reads differ, first {bad[:8]}"


def _seed(gpu, reads, optname):
    import smemgpu
    return smemgpu.seed(gpu, reads.codes, reads.offs, smemgpu.Options(**OPTS[optname]))


def _check(gpu, w, optname, what=""):
    reads = _reads_of(w)
    want = _want(w, optname)[0]
    got = _seed(gpu, reads, optname).to_smgo()
    assert got == want, (w["name"], optname, what, _diff(got, want))


def test_table_facts(worlds, gpu_device):
    """D and minsz as the handle reports them against a count of the text's k-mers; the indexes are
    the ones the cases below were made for (D = 6, 5, 4 and 0: the path off)."""
    import smemgpu
    seen = {}
    for name, w in worlds.items():
        gpu = smemgpu.Gpu(w["idx"], device=gpu_device)
        try:
            f = gpu.kmer_facts()
            seen[name] = f
            print(f"[kmer_skip] {name}: {f}, kernel {gpu.seed_kernel}")
            assert 1 <= f["k"] <= 12 and 4 ** f["k"] <= w["idx"].seq_len or f["k"] == 1
            mn = f["minsz"]
            assert all(mn[l] >= mn[l + 1] for l in range(1, f["k"]))           # non-increasing
            assert all(mn[l] > 0 for l in range(1, f["D"] + 2))                # complete through D + 1
            assert f["D"] == f["k"] - 1 or mn[f["D"] + 2] == 0                 # ... and no further
            assert gpu.variant == 49 and gpu.seed_kernel == (68 if f["D"] >= 2 else 49)
            if (w["g"] < 4).all():
                want_mn, want_d = _level_min(w["g"], f["k"])
                assert mn[1:] == want_mn[1:] and f["D"] == want_d, (name, mn, want_mn)
            gpu.set_kmer_table(0)                                              # the opt-out
            assert gpu.kmer_facts() == {"k": 0, "D": 0, "minsz": [0]} and gpu.seed_kernel == 49
        finally:
            gpu.close()
    assert seen["g1"]["D"] == 6 and seen["rnd20k"]["D"] == 5 and seen["lowcx"]["D"] == 4, seen
    assert seen["ac8k"]["D"] == 0, seen["ac8k"]
    # the repeat family's re-seeding calls (min_intv = copies + 1, both strands counted once each) ask for
    # more than the deepest level holds: dp < D occurs
    f = seen["rnd20k"]
    assert f["minsz"][f["D"]] < N_COPIES + 1 <= 500, f


@pytest.mark.parametrize("name", ["g1", "rnd20k", "lowcx", "ac8k"])
@pytest.mark.parametrize("optname", list(OPTS))
def test_default_handle_parity(worlds, gpu_device, name, optname):
    """The handle as every caller gets it (its own table), every option set."""
    import smemgpu
    w = worlds[name]
    gpu = smemgpu.Gpu(w["idx"], device=gpu_device)
    try:
        _check(gpu, w, optname)
        if name == "rnd20k" and optname in ("reseed", "width3"):
            # the unit's read is one match of all copies, re-seeded with min_intv = copies + 1 > minsz[D];
            # the kernel takes the depth of split_width + 1 for every re-seeding call: below D as well
            res = _seed(gpu, _one(w["unit"]), optname)
            assert int(res.intv[:, 2].max()) == N_COPIES
            f = gpu.kmer_facts()
            lib = smemgpu.load()
            mn = np.array(f["minsz"] + [0] * 16, np.uint64)[:16]
            assert lib.smem_kmer_call_depth(mn.ctypes.data, f["D"], N_COPIES + 1) < f["D"]
            assert 2 <= lib.smem_kmer_call_depth(mn.ctypes.data, f["D"], OPTS[optname]["split_width"] + 1) < f["D"]
    finally:
        gpu.close()


@pytest.mark.parametrize("name", ["g1", "rnd20k", "lowcx", "ac8k"])
def test_table_depths(worlds, gpu_device, name):
    """K = 1, 2, D - 1 .. D + 2 and 12 on one handle (the table replaced each time); variant 68 by number
    runs the skipping kernel whatever the depth."""
    import smemgpu
    w = worlds[name]
    gpu = smemgpu.Gpu(w["idx"], device=gpu_device)
    try:
        d0 = gpu.kmer_facts()["D"]
        gpu.set_variant(68)
        for k in sorted({1, 2, 12} | {d for d in (d0 - 1, d0, d0 + 1, d0 + 2) if d >= 1}):
            gpu.set_kmer_table(k)
            f = gpu.kmer_facts()
            assert f["k"] == k and f["D"] == min(d0, k - 1), (k, f)
            for optname in ("default", "reseed", "width3"):
                _check(gpu, w, optname, f"K={k}")
    finally:
        gpu.close()


@pytest.mark.parametrize("name", ["g1", "rnd20k"])
def test_variants_agree(worlds, gpu_device, name):
    """The default against the plain kernel (49 by number) and the A/B shapes on the same batch: identical
    fetch() arrays, not only identical streams."""
    import smemgpu
    w = worlds[name]
    reads = _reads_of(w)
    outs = {}
    for variant in (0, 49, 69, 70):
        if variant and not smemgpu.load().smem_seed_variant_built(variant):
            continue
        gpu = smemgpu.Gpu(w["idx"], device=gpu_device, variant=variant)
        try:
            if variant == 0:
                assert gpu.seed_kernel == 68
            if variant == 49:
                assert gpu.seed_kernel == 49
            r = _seed(gpu, reads, "reseed")
            outs[variant] = (r.intv.copy(), r.intv_off.copy())
        finally:
            gpu.close()
    assert 0 in outs and 49 in outs
    for v, (a, b) in outs.items():
        assert np.array_equal(a, outs[49][0]) and np.array_equal(b, outs[49][1]), v


@pytest.mark.parametrize("cap", [2, 64])
def test_overflow_pass(worlds, gpu_device, cap):
    import smemgpu
    w = worlds["rnd20k"]
    reads = _reads_of(w)
    gpu = smemgpu.Gpu(w["idx"], device=gpu_device, intv_cap=cap)
    try:
        assert gpu.seed_kernel == 68
        b = gpu.batch(reads.n, reads.codes.size, int(reads.lens.max()))
        b.set_reads(reads.codes, reads.offs)
        b.run(smemgpu.Options(**OPTS["k14s20"]))
        if cap == 2:
            assert b.stats()["n_overflow"] > 0
        got = b.fetch().to_smgo()
        b.close()
        want = _want(w, "k14s20")[0]
        assert got == want, _diff(got, want)
    finally:
        gpu.close()


def test_repeated_launches_and_batch_sizes(worlds, gpu_device):
    """One batch launched three times gives the same bytes; batches of OWN - 1, OWN, OWN + 1 and
    4 OWN + 1 reads (a wave's owners all busy, one idle, one read in a second wave)."""
    import smemgpu
    w = worlds["g1"]
    reads = _reads_of(w)
    gpu = smemgpu.Gpu(w["idx"], device=gpu_device)
    try:
        assert gpu.seed_kernel == 68
        b = gpu.batch(reads.n, reads.codes.size, int(reads.lens.max()))
        b.set_reads(reads.codes, reads.offs)
        want = _want(w, "default")[0]
        for _ in range(3):
            b.run(smemgpu.Options(**OPTS["default"]))
            assert b.fetch().to_smgo() == want
        b.close()
        # the densest reads first: the last ones of the set are plain genome reads
        for n in (OWN - 1, OWN, OWN + 1, 4 * OWN + 1):
            sub = reads.subset(np.arange(reads.n - n, reads.n))
            want_n = oracle.seed(w["ref"], sub.codes, sub.offs, threads=4, **OPTS["default"])[0]
            got = _seed(gpu, sub, "default").to_smgo()
            assert got == want_n, (n, _diff(got, want_n))
    finally:
        gpu.close()


def test_golden_streams(gpu_device):
    """The committed streams of the compiled reference on the default handle, and with K = 2 and 12."""
    import smemgpu
    from tests import golden_data
    fx = golden_data.load()
    gpu = smemgpu.Gpu(fx.index, device=gpu_device)
    try:
        for k in (None, 2, 12):
            if k is not None:
                gpu.set_kmer_table(k)
            assert gpu.seed_kernel == (68 if gpu.kmer_facts()["D"] >= 2 else 49)
            for case in fx.cases:
                reads = fx.reads.subset(np.arange(case["n_reads"]))
                res = smemgpu.seed(gpu, reads.codes, reads.offs, smemgpu.Options(**case["opt"]))
                assert res.to_smgo() == fx.stream(case), (k, case["name"])
    finally:
        gpu.close()


HUMAN_BP = 3_101_804_739   # human_g1k_v37 l_pac


def test_human_size(gpu_device):
    """The size bench.py runs at: the handle builds its 12-mer table beside a 6.2 G-symbol index, finds
    D >= 10 and launches the skipping kernel (not the plain one, which a failed allocation or a small D
    would fall back to in silence); 2,000 reads bit for bit against the restatement, under the default
    options and a re-seeding set, and the plain kernel on the same handle gives the same arrays."""
    import smemgpu
    from smemgpu import synth
    g = synth.make_genome(HUMAN_BP, seed=1, n_chrom=24)
    idx = smemgpu.Index.build_gpu(g.codes, device=gpu_device, large=True)
    assert idx.seq_len == 2 * HUMAN_BP
    ref = oracle.OracleIndex(words=idx.words, primary=idx.primary, L2=idx.L2)
    gpu = smemgpu.Gpu(idx, device=gpu_device)
    try:
        f = gpu.kmer_facts()
        print(f"[kmer_skip] human size: {f}, kernel {gpu.seed_kernel}")
        assert f["k"] == 12 and f["D"] >= 10, f
        assert f["minsz"][f["D"]] >= 11, f          # the default options' re-seeding calls keep the full depth
        assert gpu.variant == 49 and gpu.seed_kernel == 68
        reads = synth.make_reads(g.codes, 2_000, 150, seed=31, sub_rate=0.02, n_rate=0.001)
        outs = {}
        for optname in ("default", "reseed"):
            want = oracle.seed(ref, reads.codes, reads.offs, threads=16, **OPTS[optname])[0]
            res = _seed(gpu, reads, optname)
            got = res.to_smgo()
            assert got == want, (optname, _diff(got, want))
            outs[optname] = (res.intv.copy(), res.intv_off.copy())
        assert int(outs["default"][0][:, :2].max()) > 2 ** 32   # coordinates past 32 bits came through the table
        gpu.set_variant(49)
        assert gpu.seed_kernel == 49
        res = _seed(gpu, reads, "default")
        assert np.array_equal(res.intv, outs["default"][0]) and np.array_equal(res.intv_off, outs["default"][1])
    finally:
        gpu.close()
        ref.close()
