"""The k-mer table probed at its deepest stored level (DESIGN.md §5 "Probing at the table's depth").

A table of K levels vouches for depth K - 1 by what it stores (smem_gpu_kmer_facts' D); the build also
reduces level K + 1, computed from level K and never stored, to its smallest size, and a launch runs at
depth K where that level is complete (smem_gpu_kmer_probe_depth).  Checked here, on the four small
indexes of test_gpu_kmer_skip.py (the golden genome, D = 6; 20 kbp random with a repeat family, D = 5; a
low-complexity one, D = 4; one of two letters, D = 0):

 * the unstored level's minimum against a numpy count of the text's (K + 1)-mers, and the depth a launch
   takes, for K = 1, 2 and d0 - 1 .. d0 + 2 (d0: the index's own D, so level d0 + 1 is its last complete
   one).  The depth is the largest L <= K with levels 1 .. L + 1 complete, which on these indexes is
   min(d0, K): K itself up to K == d0 -- the deepest table that can run at its own depth -- and
   min(d0, K - 1) = d0 beyond it, where the reported D is min(d0, K - 1) throughout;
 * the kernel at dp == K (set_kmer_table(d0), instantiation 68) bit for bit against the restatement, on
   reads that put the seam everywhere: reads of K - 1 .. 2 K bases, an ambiguous base around K bases from
   a call's start, call starts at every residue of the 16-byte query window, reads that end K bases
   after a call start, a repeat unit whose re-seeding min_intv exceeds minsz[K], all-N and empty reads;
 * that the launch really ran at depth K (else the cases pass on the old path in silence);
 * the overflow pass and the plain kernel on the same handle: identical arrays.
"""
import numpy as np
import pytest

from oracle import oracle

pytestmark = pytest.mark.gpu

OPTS = {
    "default": dict(min_seed_len=19, split_factor=1.5, split_width=10, start_width=1),
    "reseed": dict(min_seed_len=19, split_factor=1.0, split_width=500, start_width=1),
    "width3": dict(min_seed_len=10, split_factor=1.0, split_width=500, start_width=3),
}
N_COPIES = 30  # of the repeat unit in the small genome
WANT_D = {"g1": 6, "rnd20k": 5, "lowcx": 4, "ac8k": 0}


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
    # low complexity
    lc = np.concatenate([np.zeros(2000, np.uint8), np.tile([1, 2], 1000).astype(np.uint8),
                         rng.integers(0, 4, 4000).astype(np.uint8)])
    out["lowcx"] = (lc, None)
    # two letters: most 2-mers are absent, D = 0
    out["ac8k"] = (rng.integers(0, 2, 8000).astype(np.uint8), None)
    return out


def _golden_text():
    """The golden genome as the index holds it (the FASTA's ambiguous bases are random bases there):
    the reference's 2-bit .pac, four bases a byte, the first one highest."""
    from tests import golden_data
    n = golden_data.l_pac("g1")
    pac = golden_data.pac("g1")
    pos = np.arange(n)
    return ((pac[pos >> 2] >> ((~pos & 3) << 1)) & 3).astype(np.uint8)


@pytest.fixture(scope="module")
def worlds(gpu_device):
    """Per index: the restatement's index, the text, the index's own D (from a handle on its default),
    and (lazily, once) the seam reads and the restatement's streams per depth and option set."""
    import smemgpu
    from tests import golden_data
    ws = {}
    fx = golden_data.load()
    items = {"g1": (None, None)}
    items.update(_genomes())
    for name, (g, unit) in items.items():
        if name == "g1":
            idx, g = fx.index, _golden_text()
        else:
            idx = smemgpu.Index.build(g)
        gpu = smemgpu.Gpu(idx, device=gpu_device)
        try:
            d0 = gpu.kmer_facts()["D"]
        finally:
            gpu.close()
        ws[name] = dict(name=name, idx=idx, g=g, unit=unit, d0=d0, reads={}, truth={}, mins=None,
                        ref=oracle.OracleIndex(words=idx.words, primary=idx.primary, L2=idx.L2))
    yield ws
    for w in ws.values():
        w["ref"].close()


def _level_min(w, k_max):
    """minsz[L], L = 1..k_max, counted on the text the index holds (both strands)."""
    from smemgpu import synth
    if w["mins"] is None or len(w["mins"]) <= k_max:
        t = synth.forward_reverse_text(w["g"]).astype(np.int64)
        mn = [0]
        for L in range(1, k_max + 1):
            v = np.zeros(t.size - L + 1, np.int64)
            for o in range(L):
                v = v * 4 + t[o:t.size - L + 1 + o]
            mn.append(int(np.bincount(v, minlength=4 ** L).min()))
        w["mins"] = mn
    return w["mins"]


def _one(arr):
    from smemgpu import synth
    arr = np.asarray(arr, np.uint8)
    return synth.Reads(np.array([arr.size], np.int32), arr, np.array([0, arr.size], np.int64))


def _seam_reads(w, K):
    """Ordinary reads of the index and reads whose calls meet the depth-K seam at every position."""
    from smemgpu import synth
    if K in w["reads"]:
        return w["reads"][K]
    g, n = w["g"], w["g"].size
    at = lambda o, L: g[o % (n - 400):o % (n - 400) + L].copy()
    parts = []
    for L in sorted({0, 1, max(K - 1, 0), K, K + 1, 2 * K, 2 * K + 1, 19, 40}):   # lengths around K and 2 K
        parts.append(_one(at(700, L)))
    for x in (0, 31):                          # an ambiguous base K - 2 .. K + 1 (and nearby) from a call's start:
        for off in range(max(K - 3, 1), K + 3):  # the first call (x = 0) and one that starts after an N (x = 31)
            q = at(1200, 80)
            if x:
                q[x - 1] = 4
            q[x + off] = 4
            parts.append(_one(q))
    for p in range(1, 34):                     # call starts at 33 consecutive positions: every residue of the
        q = at(2000, 90)                       # 16-byte window, whatever the read's offset in the batch, so the K
        q[p - 1] = 4                           # collected bases cross the window's end at each position
        parts.append(_one(q))
    for p in range(max(K - 2, 1), K + 3):      # a read that ends K - 2 .. K + 2 bases after a call start
        q = at(2400, 60)
        q[60 - p - 1] = 4
        parts.append(_one(q))
    for p in range(1, K + 3):                  # a mismatch p bases into the read: the backward phase of calls
        q = at(3000, 100)                      # that start within K bases of the read's start reaches i = -1
        q[p] = (q[p] + 1) & 3
        q[p + 25] = (q[p + 25] + 2) & 3
        parts.append(_one(q))
    parts.append(_one(np.full(60, 4)))         # all N; N at both ends; every K-th base N
    parts.append(_one(np.concatenate([[4], at(5000, 100), [4]])))
    parts.append(_one(np.where(np.arange(120) % (K + 1) == K, 4, at(3300, 120))))
    parts.append(_one(np.where(np.arange(120) % (K + 2) == 0, 4, at(3300, 120))))
    rng = np.random.default_rng(11)
    parts.append(_one(rng.integers(0, 4, 150)))  # not of the genome: calls end at once
    for nn in (30, 150):                       # tandem repeats: long lists
        parts.append(_one(np.zeros(nn)))
        parts.append(_one(np.tile([1, 2], nn)[:nn]))
    if w["unit"] is not None:                  # the repeat family: re-seeds with min_intv = copies + 1
        parts.append(_one(w["unit"]))
        parts.append(_one(w["unit"][3:90]))
    parts.append(synth.make_reads(g, 96, (1, 200), seed=5, n_rate=0.03, random_frac=0.1))
    parts.append(synth.make_reads(g, 96, 150, seed=6, sub_rate=0.04))
    w["reads"][K] = synth.concat_reads(parts)
    return w["reads"][K]


def _want(w, K, optname):
    if (K, optname) not in w["truth"]:
        r = _seam_reads(w, K)
        w["truth"][(K, optname)] = oracle.seed(w["ref"], r.codes, r.offs, threads=4, **OPTS[optname])[0]
    return w["truth"][(K, optname)]


def _diff(got, want):
    from smemgpu import synth
    a, b = synth.read_smgo(got), synth.read_smgo(want)
    bad = [i for i in range(len(b)) if len(a[i]) != len(b[i]) or any(
        x.shape != y.shape or (x != y).any() for x, y in zip(a[i], b[i]))]
    return f"{len(bad)} reads differ, first {bad[:8]}"


def _seed(gpu, reads, optname):
    import smemgpu
    return smemgpu.seed(gpu, reads.codes, reads.offs, smemgpu.Options(**OPTS[optname]))


@pytest.mark.parametrize("name", ["g1", "rnd20k", "lowcx", "ac8k"])
def test_unstored_minimum_and_depth(worlds, gpu_device, name):
    import smemgpu
    w = worlds[name]
    d0 = w["d0"]
    assert d0 == WANT_D[name]
    lib = smemgpu.load()
    gpu = smemgpu.Gpu(w["idx"], device=gpu_device)
    try:
        ks = sorted({1, 2} | {d for d in (d0 - 1, d0, d0 + 1, d0 + 2) if d >= 1})
        want = _level_min(w, max(ks) + 1)
        assert all(want[l] > 0 for l in range(1, d0 + 2)) and want[d0 + 2] == 0   # d0 is the text's own D
        for k in ks:
            gpu.set_kmer_table(k)
            f = gpu.kmer_facts()
            p = gpu.kmer_probe_depth(1)
            print(f"[kmer_edge] {name} K={k}: {f}, {p}")
            assert f["k"] == k and f["D"] == min(d0, k - 1), (k, f)          # the reported D: stored levels only
            assert f["minsz"][1:] == want[1:k + 1], (k, f, want)
            assert p["min_next"] == want[k + 1], (k, p, want)                # 0 when a (k + 1)-mer is absent
            assert p["depth"] == min(d0, k), (k, p)
            assert (p["depth"] == k) == (k <= d0) and (k <= d0 or p["depth"] == min(d0, k - 1)), (k, p)
            mn = np.array(f["minsz"] + [0] * 16, np.uint64)[:16]
            for mi in (1, 3, 11, N_COPIES + 1, 501):
                q = gpu.kmer_probe_depth(mi)
                assert q["depth"] == lib.smem_kmer_probe_depth(mn.ctypes.data, k, p["min_next"], mi) <= p["depth"]
                assert q["depth"] == 0 or f["minsz"][q["depth"]] >= mi
        if name == "ac8k":
            assert all(gpu.kmer_probe_depth(mi)["depth"] == 0 for mi in (1, 3))   # the path is off
        gpu.set_kmer_table(0)
        assert gpu.kmer_probe_depth(1) == {"depth": 0, "min_next": 0}
    finally:
        gpu.close()


@pytest.mark.parametrize("name", ["g1", "rnd20k", "lowcx", "ac8k"])
def test_parity_at_the_tables_depth(worlds, gpu_device, name):
    """set_kmer_table(d0): every stored level and the unstored one complete, so the launch probes level
    K = d0 itself.  (The two-letter index has d0 = 0: a table of 2 levels there, the depth 0 and the
    same reads on the plain path of the skipping kernel.)"""
    import smemgpu
    w = worlds[name]
    K = w["d0"] if w["d0"] >= 1 else 2
    gpu = smemgpu.Gpu(w["idx"], device=gpu_device)
    try:
        gpu.set_variant(68)
        gpu.set_kmer_table(K)
        assert gpu.seed_kernel == 68
        f = gpu.kmer_facts()
        reads = _seam_reads(w, K)
        for optname, o in OPTS.items():
            dp0 = gpu.kmer_probe_depth(o["start_width"])
            dp1 = gpu.kmer_probe_depth(o["split_width"] + 1)
            print(f"[kmer_edge] {name} K={K} {optname}: D {f['D']}, depths {dp0['depth']} / {dp1['depth']}, "
                  f"unstored minimum {dp0['min_next']}")
            if w["d0"] >= 1:   # the path actually taken: the read's first calls run at the table's depth
                assert dp0["min_next"] > 0 and f["D"] == K - 1
                for dp, mi in ((dp0, o["start_width"]), (dp1, o["split_width"] + 1)):
                    assert dp["depth"] == max([l for l in range(1, K + 1) if f["minsz"][l] >= mi], default=0), (optname, dp, f)
                if optname == "default":
                    assert dp0["depth"] == K, (dp0, f)
            else:
                assert dp0["depth"] == 0 and dp1["depth"] == 0
            want = _want(w, K, optname)
            got = _seed(gpu, reads, optname).to_smgo()
            assert got == want, (name, K, optname, _diff(got, want))
        if name == "rnd20k":
            # the unit's read is one match of all copies, re-seeded with min_intv = copies + 1 > minsz[K]: the
            # depth of such a call is below K although the unstored level is complete
            assert f["minsz"][K] < N_COPIES + 1
            q = gpu.kmer_probe_depth(N_COPIES + 1)
            assert q["min_next"] > 0 and 0 < q["depth"] < K, q
            assert 2 <= gpu.kmer_probe_depth(OPTS["reseed"]["split_width"] + 1)["depth"] < K
            res = _seed(gpu, _one(w["unit"]), "reseed")
            assert int(res.intv[:, 2].max()) == N_COPIES
    finally:
        gpu.close()


def test_first_calls_at_depth_k_where_min_intv_allows(worlds, gpu_device):
    """The golden genome at K = d0 = 6 under every option set: minsz[6] >= 3, so the first calls of
    `width3` run at depth 6 too, and the launch's depth is the getter's."""
    import smemgpu
    w = worlds["g1"]
    K = w["d0"]
    gpu = smemgpu.Gpu(w["idx"], device=gpu_device)
    try:
        gpu.set_variant(68)
        gpu.set_kmer_table(K)
        f = gpu.kmer_facts()
        assert f["minsz"][K] >= 3, f
        for optname, o in OPTS.items():
            assert gpu.kmer_probe_depth(o["start_width"])["depth"] == K
    finally:
        gpu.close()


@pytest.mark.parametrize("name", ["g1", "rnd20k"])
def test_overflow_pass_and_plain_kernel(worlds, gpu_device, name):
    """List capacity 2 (most reads go through the overflow pass) at dp == K, then the plain kernel (49 by
    number) on the same handle: the restatement's stream and identical fetch() arrays; a handle of the
    default capacity gives the same arrays."""
    import smemgpu
    w = worlds[name]
    K = w["d0"]
    reads = _seam_reads(w, K)
    want = _want(w, K, "reseed")
    outs = {}
    for cap in (2, 0):
        gpu = smemgpu.Gpu(w["idx"], device=gpu_device, intv_cap=cap) if cap else smemgpu.Gpu(w["idx"], device=gpu_device)
        try:
            gpu.set_variant(68)
            gpu.set_kmer_table(K)
            assert gpu.seed_kernel == 68 and gpu.kmer_probe_depth(1)["depth"] == K
            b = gpu.batch(reads.n, reads.codes.size, int(reads.lens.max()))
            b.set_reads(reads.codes, reads.offs)
            b.run(smemgpu.Options(**OPTS["reseed"]))
            if cap:
                assert b.stats()["n_overflow"] > 0
            r = b.fetch()
            got = r.to_smgo()
            assert got == want, (cap, _diff(got, want))
            outs[(cap, 68)] = (r.intv.copy(), r.intv_off.copy())
            b.close()
            if cap:
                gpu.set_variant(49)
                assert gpu.seed_kernel == 49
                r = _seed(gpu, reads, "reseed")
                outs[(cap, 49)] = (r.intv.copy(), r.intv_off.copy())
        finally:
            gpu.close()
    ref = outs[(2, 49)]
    for key, (a, o) in outs.items():
        assert np.array_equal(a, ref[0]) and np.array_equal(o, ref[1]), key
