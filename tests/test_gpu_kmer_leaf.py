"""The k-mer table's leaf level (DESIGN.md §5 "A leaf level").

Behind the k levels it reports, a table may store level k + 1, the leaf.  A launch probes the leaf when it is
complete, its smallest size holds min_intv, and it is strict (no present string of it has a one-base
extension of its own size), which the build reduces beside level k + 2's minimum; completeness of level
k + 2 is no longer needed.  Checked here on 40 kbp genomes whose own D is 5 (every 6-mer occurs, some 7-mers
do not), with a table of 5 levels and the leaf 6; every property a test was made for is counted on the text
with numpy and asserted, never assumed:

 * strict, next level incomplete: the facts, the launch at depth 6, and the results bit for bit against the
   restatement under three option sets, on reads that put the seam everywhere;
 * complete but not strict (a genome edited until one 6-mer is always followed by the same base): the leaf
   reports it, the launch stays at the old rule's depth, the results are bit exact;
 * a leaf too small for re-seeding calls: their depth is below the first calls';
 * a default handle on a small index has no leaf; SMEM_GPU_KMER_LEAF=0 removes it from the entry point that
   builds one; the overflow pass and the plain kernel on a handle with a leaf give the same arrays.
"""
import numpy as np
import pytest

from oracle import oracle

pytestmark = pytest.mark.gpu

OPTS = {
    "default": dict(min_seed_len=19, split_factor=1.5, split_width=10, start_width=1),
    "reseed": dict(min_seed_len=19, split_factor=1.0, split_width=500, start_width=1),
    "long_seed": dict(min_seed_len=40, split_factor=1.5, split_width=10, start_width=1),
}
N_COPIES = 30   # of the repeat unit
N_FEW = 8       # of the second unit: at most split_width, so the default options re-seed its match
D0 = 5          # the genomes' own D
LEAF = D0 + 1


def _strict_genome():
    """40 kbp random with a 100-base unit copied N_COPIES times (re-seeding calls with min_intv = 31)."""
    rng = np.random.default_rng(77)
    g = rng.integers(0, 4, 40_000).astype(np.uint8)
    unit = g[100:200].copy()
    for c in range(1, N_COPIES):
        g[100 + 600 * c:200 + 600 * c] = unit
    for c in range(1, N_FEW):                       # a second family of N_FEW copies: re-seeded under the default
        g[20_000 + 700 * c:20_100 + 700 * c] = g[20_000:20_100]   # options, with min_intv = N_FEW + 1
    return g, unit


def _code(w):
    c = 0
    for b in w:
        c = c * 4 + int(b)
    return c


def _not_strict_genome():
    """The same genome edited until every occurrence of one LEAF-mer W, on either strand, is followed by
    the same base b: each W in the forward strand gets b behind it, each rc(W) gets rc(b) before it, again
    and again until nothing changes (an edit can make a new occurrence).  Returns (genome, unit, W, b)."""
    g, _ = _strict_genome()
    g = g.copy()
    W = g[5000:5000 + LEAF].copy()
    rc = (3 - W)[::-1]
    assert (W != rc).any()
    b = int(g[5000 + LEAF])
    n = g.size
    for _ in range(100):
        win = np.lib.stride_tricks.sliding_window_view(g, LEAF)
        fw = np.flatnonzero((win == W).all(1))
        rv = np.flatnonzero((win == rc).all(1))
        fw, rv = fw[fw + LEAF < n], rv[rv >= 1]
        if (g[fw + LEAF] == b).all() and (g[rv - 1] == 3 - b).all():
            break
        g[fw + LEAF] = b
        g[rv - 1] = 3 - b
    else:
        raise AssertionError("the edit did not reach a fixed point")
    return g, g[100:200].copy(), W, b


def _counts(g, k_max):
    """[L] -> occurrences of every L-mer in the text the index holds (both strands), L = 1..k_max."""
    from smemgpu import synth
    t = synth.forward_reverse_text(g).astype(np.int64)
    out = [None]
    for L in range(1, k_max + 1):
        v = np.zeros(t.size - L + 1, np.int64)
        for o in range(L):
            v = v * 4 + t[o:t.size - L + 1 + o]
        out.append(np.bincount(v, minlength=4 ** L))
    return out


def _as_large_as_itself(cnt, L):
    """The present L-mers with a one-base right extension of their own size.  (The text holds both strands,
    so the left extensions of a string are the right ones of its reverse complement.)"""
    return np.flatnonzero((cnt[L] > 0) & (cnt[L + 1].reshape(-1, 4).max(1) == cnt[L]))


def _one(arr):
    from smemgpu import synth
    arr = np.asarray(arr, np.uint8)
    return synth.Reads(np.array([arr.size], np.int32), arr, np.array([0, arr.size], np.int64))


def _seam_reads(g, unit):
    """Reads whose calls meet the leaf's seam everywhere, and ordinary ones."""
    from smemgpu import synth
    n = g.size
    at = lambda o, L: g[o % (n - 400):o % (n - 400) + L].copy()
    parts = [_one(at(700, L)) for L in range(32)]            # lengths 0-31
    parts.append(_one(np.full(60, 4)))                        # all N
    for x in (0, 31):                                         # an N at each of the LEAF + 1 positions after a call's
        for off in range(1, LEAF + 2):                        # start: the first call, and one that starts after an N
            q = at(1200, 80)
            if x:
                q[x - 1] = 4
            q[x + off] = 4
            parts.append(_one(q))
    for p in range(1, LEAF + 1):                              # a read that ends fewer than LEAF bases (and LEAF)
        q = at(2400, 60)                                      # after a call's start
        q[60 - p - 1] = 4
        parts.append(_one(q))
    for p in range(1, 18):                                    # call starts at every residue of the 16-byte window
        q = at(2000, 90)
        q[p - 1] = 4
        parts.append(_one(q))
    for p in range(1, LEAF + 3):                              # the backward phase reaches i = -1 within LEAF bases
        q = at(3000, 100)
        q[p] = (q[p] + 1) & 3
        q[p + 25] = (q[p + 25] + 2) & 3
        parts.append(_one(q))
    parts.append(_one(np.where(np.arange(120) % (LEAF + 1) == LEAF, 4, at(3300, 120))))
    parts.append(_one(at(4990, 120)))                         # across the edited 6-mer of the not-strict genome
    parts.append(_one((3 - at(4990, 120))[::-1]))
    parts.append(_one(unit))                                  # the repeat family: re-seeds with min_intv = copies + 1
    parts.append(_one(unit[3:90]))
    parts.append(_one(g[20_000:20_100]))                      # the family of N_FEW copies: re-seeds under the defaults
    parts.append(_one(np.zeros(30)))
    parts.append(synth.make_reads(g, 500, 150, seed=6, sub_rate=0.04))   # 500 ordinary 150-bp reads
    return synth.concat_reads(parts)


@pytest.fixture(scope="module")
def worlds(gpu_device):
    """Per genome: the index, the restatement's index, the counted k-mers, the reads and (lazily, once) the
    restatement's stream per option set."""
    import smemgpu
    ws = {}
    for name, made in (("strict", _strict_genome()), ("notstrict", _not_strict_genome())):
        g, unit = made[0], made[1]
        idx = smemgpu.Index.build(g)
        ws[name] = dict(name=name, g=g, unit=unit, idx=idx, made=made, cnt=_counts(g, LEAF + 2), truth={},
                        reads=_seam_reads(g, unit),
                        ref=oracle.OracleIndex(words=idx.words, primary=idx.primary, L2=idx.L2))
    yield ws
    for w in ws.values():
        w["ref"].close()


def _want(w, optname):
    if optname not in w["truth"]:
        r = w["reads"]
        w["truth"][optname] = oracle.seed(w["ref"], r.codes, r.offs, threads=4, **OPTS[optname])[0]
    return w["truth"][optname]


def _diff(got, want):
    from smemgpu import synth
    a, b = synth.read_smgo(got), synth.read_smgo(want)
    bad = [i for i in range(len(b)) if len(a[i]) != len(b[i]) or any(
        x.shape != y.shape or (x != y).any() for x, y in zip(a[i], b[i]))]
    return f"{len(bad)} reads differ, first {bad[:8]}"


def _seed(gpu, reads, optname):
    import smemgpu
    return smemgpu.seed(gpu, reads.codes, reads.offs, smemgpu.Options(**OPTS[optname]))


def _old_depth(gpu, min_intv):
    """The depth by the rule without a leaf, from the handle's reported facts."""
    import smemgpu
    f = gpu.kmer_facts()
    mn = np.array(f["minsz"] + [0] * 16, np.uint64)[:16]
    return smemgpu.load().smem_kmer_probe_depth(mn.ctypes.data, f["k"], gpu.kmer_probe_depth(1)["min_next"], min_intv)


def test_strict_leaf_next_level_incomplete(worlds, gpu_device):
    import smemgpu
    w = worlds["strict"]
    cnt = w["cnt"]
    mins = [0] + [int(cnt[L].min()) for L in range(1, LEAF + 2)]
    # the properties this genome was made for, counted: its own D is D0, so the leaf D0 + 1 is complete and
    # level D0 + 2 has absent strings; no present string of the leaf has an extension as large as itself
    assert all(mins[L] > 0 for L in range(1, LEAF + 1)) and mins[LEAF + 1] == 0
    assert _as_large_as_itself(cnt, LEAF).size == 0
    gpu = smemgpu.Gpu(w["idx"], device=gpu_device)
    try:
        assert gpu.kmer_facts()["D"] == D0
        gpu.set_kmer_table_leaf(D0)
        f, lf = gpu.kmer_facts(), gpu.kmer_leaf_facts()
        print(f"[kmer_leaf] strict: {f}, {lf}, {gpu.kmer_probe_depth(1)}")
        assert f["k"] == D0 and f["D"] == D0 - 1 and f["minsz"][1:] == mins[1:D0 + 1], (f, mins)
        assert lf == {"level": LEAF, "min": mins[LEAF], "strict": True, "next_min": 0}, (lf, mins)
        assert gpu.seed_kernel == 68
        for optname, o in OPTS.items():
            dp0 = gpu.kmer_probe_depth(o["start_width"])
            dp1 = gpu.kmer_probe_depth(o["split_width"] + 1)
            print(f"[kmer_leaf] strict {optname}: depths {dp0['depth']} / {dp1['depth']}")
            assert dp0["min_next"] == mins[LEAF]
            assert dp0["depth"] == LEAF and _old_depth(gpu, o["start_width"]) == D0     # one deeper than before
            assert dp1["depth"] == max(L for L in range(0, LEAF + 1) if L == 0 or mins[L] >= o["split_width"] + 1)
            want = _want(w, optname)
            got = _seed(gpu, w["reads"], optname).to_smgo()
            assert got == want, (optname, _diff(got, want))
    finally:
        gpu.close()


def test_complete_leaf_that_is_not_strict(worlds, gpu_device):
    """Fails if the strictness word is ignored: the launch would then run at the leaf."""
    import smemgpu
    w = worlds["notstrict"]
    cnt, (_, _, W, b) = w["cnt"], w["made"]
    mins = [0] + [int(cnt[L].min()) for L in range(1, LEAF + 2)]
    assert all(mins[L] > 0 for L in range(1, LEAF + 1)) and mins[LEAF + 1] == 0   # complete, the next level not
    cw = _code(W)
    assert cnt[LEAF][cw] >= 2 and cnt[LEAF + 1][cw * 4 + b] == cnt[LEAF][cw]     # W is always followed by b
    assert cw in _as_large_as_itself(cnt, LEAF)
    gpu = smemgpu.Gpu(w["idx"], device=gpu_device)
    try:
        gpu.set_kmer_table_leaf(D0)
        f, lf = gpu.kmer_facts(), gpu.kmer_leaf_facts()
        print(f"[kmer_leaf] not strict: {f}, {lf}, {gpu.kmer_probe_depth(1)}")
        assert f["k"] == D0 and f["D"] == D0 - 1
        assert lf == {"level": LEAF, "min": mins[LEAF], "strict": False, "next_min": 0}, (lf, mins)
        assert gpu.seed_kernel == 68
        for optname, o in OPTS.items():
            for mi in (o["start_width"], o["split_width"] + 1):
                assert gpu.kmer_probe_depth(mi)["depth"] == _old_depth(gpu, mi) <= D0
            assert gpu.kmer_probe_depth(o["start_width"])["depth"] == D0       # level D0 + 1 complete: the old rule's
            want = _want(w, optname)
            got = _seed(gpu, w["reads"], optname).to_smgo()
            assert got == want, (optname, _diff(got, want))
    finally:
        gpu.close()


def test_leaf_too_small_for_reseeding(worlds, gpu_device):
    """minsz[leaf] < N_FEW + 1 <= split_width + 1: a read's first calls probe the leaf, its re-seeding calls
    (the second repeat family's ask for min_intv = N_FEW + 1) a level below it."""
    import smemgpu
    w = worlds["strict"]
    o = OPTS["default"]
    mins = [0] + [int(w["cnt"][L].min()) for L in range(1, LEAF + 1)]
    assert 1 <= mins[LEAF] < N_FEW + 1 <= o["split_width"] + 1 and mins[2] >= o["split_width"] + 1
    gpu = smemgpu.Gpu(w["idx"], device=gpu_device)
    try:
        gpu.set_kmer_table_leaf(D0)
        dp0 = gpu.kmer_probe_depth(o["start_width"])["depth"]
        dp1 = gpu.kmer_probe_depth(o["split_width"] + 1)["depth"]
        assert 2 <= dp1 < dp0 == LEAF, (dp0, dp1)
        assert dp1 == max(L for L in range(1, LEAF + 1) if mins[L] >= o["split_width"] + 1)
        reads = _one(w["g"][20_000:20_100])          # one match of N_FEW copies, re-seeded with min_intv = N_FEW + 1
        res = _seed(gpu, reads, "default")
        # (the re-seeding call finds nothing of min_seed_len bases with more copies: its work shows in the parity)
        assert [int(s) for s in res.intv[:, 2]] == [N_FEW]
        want = oracle.seed(w["ref"], reads.codes, reads.offs, threads=1, **o)[0]
        assert res.to_smgo() == want
        want = _want(w, "default")
        got = _seed(gpu, w["reads"], "default").to_smgo()
        assert got == want, _diff(got, want)
    finally:
        gpu.close()


def test_defaults_switch_and_overflow_pass(worlds, gpu_device, monkeypatch):
    import smemgpu
    w = worlds["strict"]
    no_leaf = {"level": 0, "min": 0, "strict": False, "next_min": 0}
    reads, want = w["reads"], _want(w, "reseed")
    outs = {}
    for cap in (2, 0):
        gpu = smemgpu.Gpu(w["idx"], device=gpu_device, intv_cap=cap) if cap else smemgpu.Gpu(w["idx"], device=gpu_device)
        try:
            if not cap:
                # a default handle on a small index: no leaf, and the facts and the depth of a table of as many
                # levels built by number
                f = gpu.kmer_facts()
                dps = [gpu.kmer_probe_depth(mi) for mi in (1, 3, 11, N_COPIES + 1, 501)]
                assert gpu.kmer_leaf_facts() == no_leaf and f["k"] < 12
                assert dps[0]["depth"] == D0 and [d["depth"] for d in dps] == [_old_depth(gpu, mi) for mi in (1, 3, 11, N_COPIES + 1, 501)]
                gpu.set_kmer_table(f["k"])
                assert gpu.kmer_leaf_facts() == no_leaf and gpu.kmer_facts() == f
                assert [gpu.kmer_probe_depth(mi) for mi in (1, 3, 11, N_COPIES + 1, 501)] == dps
                # the switch: the entry point that builds a leaf builds none, and the depth is the one without it
                monkeypatch.setenv("SMEM_GPU_KMER_LEAF", "0")
                gpu.set_kmer_table_leaf(D0)
                assert gpu.kmer_leaf_facts() == no_leaf and gpu.kmer_facts()["k"] == D0
                assert gpu.kmer_probe_depth(1)["depth"] == D0
                monkeypatch.delenv("SMEM_GPU_KMER_LEAF")
            gpu.set_kmer_table(D0)
            before = gpu.memory()["index_bytes"]
            gpu.set_kmer_table_leaf(D0)
            assert gpu.seed_kernel == 68 and gpu.kmer_probe_depth(1)["depth"] == LEAF
            assert gpu.memory()["index_bytes"] - before == 16 * 4 ** LEAF   # smem_gpu_memory counts the leaf
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
            gpu.set_variant(49)
            assert gpu.seed_kernel == 49
            r = _seed(gpu, reads, "reseed")
            outs[(cap, 49)] = (r.intv.copy(), r.intv_off.copy())
        finally:
            gpu.close()
    ref = outs[(2, 49)]
    for key, (a, o) in outs.items():
        assert np.array_equal(a, ref[0]) and np.array_equal(o, ref[1]), key
