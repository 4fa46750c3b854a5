"""The seeding kernel's owner state machine, phase by phase (DESIGN.md §5,
"The iteration's instruction diet").

Bar: `Batch.fetch().to_smgo()` equals `oracle.seed` for the same reads, bit for
bit (the comparison bench.py's cpu_leg makes), on the default kernel.

One 300-kbp index from the host builder with three planted structures: a
300-bp homopolymer and a 400-bp dinucleotide run (the tandem repeats: a
re-seeding call that starts inside one pushes a forward entry per base or per
two bases, so its backward steps carry more entries than the 18 of an owner's
LDS list, and more than the 64 lanes of a wave), and an exact repeat family of
five 600-bp copies (equal interval sizes: the dedup and its carry between the
chunks of a step).

The cases are the smallest inputs at which the owners' blocks can go wrong:
 * batches of 1, 23, 24, 25, 95, 96, 97 and 257 reads -- fewer owners than a
   wave has (24), exactly a wave's and a block's (96), one more: the claim and
   exit paths, and lanes that never own a read;
 * lengths 0, 1, 18, 19, 20, 31, 32, 33, 150 and 151 mixed in one batch, so
   reads start anywhere in the 16-base query windows, and reads whose forward
   extension ends on a window's last base, on its first and beside them;
 * N at the first base, at the last, at window positions 15 and 16, two in a
   row, and an all-N read;
 * reads inside the tandem repeats (asserted from the oracle's counters to
   reach steps of more than 18 and of more than 64 entries);
 * re-seeding reads at the default options and where split_len equals the
   read's length; reads that log 0, 1, 2 and 3 records in all (the even / odd
   pending record of the one log site) and calls that keep 1, 2 and 3 -- a call
   keeps at least its longest match (software/bwamem.c:263), so no call keeps 0:
   the read without a record is the one without a call;
 * a small intv_cap, so some reads go through the overflow pass;
 * run after run on one batch object, the second read set smaller;
 * the four arms of the diet taken out one by one and together (A/B build only).
"""
import numpy as np
import pytest

from oracle import oracle

pytestmark = pytest.mark.gpu

OPTS = {
    "default": dict(min_seed_len=19, split_factor=1.5, split_width=10, start_width=1),
    # split_len = (int)(19 * 2.0 + .499) = 38: the length of the `u38` reads
    "split38": dict(min_seed_len=19, split_factor=2.0, split_width=10, start_width=1),
}
SIZES = [1, 23, 24, 25, 95, 96, 97, 257]
LENGTHS = [0, 1, 18, 19, 20, 31, 32, 33, 150, 151]
HP0, HPN = 100_000, 300      # homopolymer run
DI0, DIN = 140_000, 400      # dinucleotide run
FAM, FAML = [20_000, 61_000, 150_000, 222_000, 280_000], 600
OWN_LIST = 18                # LDS list entries per owner of the default kernel (seed_wp_kernel<24, 18, ..>)
ORC_NL = 11                  # the list length the oracle's n_bwd_task_hi counts from (smem_oracle.c list_lds)


def _genome():
    from smemgpu import synth
    g = synth.make_genome(300_000, seed=31).codes.copy()
    rng = np.random.default_rng(5)
    g[HP0:HP0 + HPN] = 0
    g[HP0 - 1], g[HP0 + HPN] = 1, 2
    g[DI0:DI0 + DIN] = np.tile(np.array([0, 1], np.uint8), DIN // 2)
    g[DI0 - 1], g[DI0 + DIN] = 3, 3
    fam = rng.integers(0, 4, size=FAML, dtype=np.uint8)
    for p in FAM:
        g[p:p + FAML] = fam
    return g


def _reads_of(arrs):
    from smemgpu import synth
    lens = np.array([a.size for a in arrs], np.int32)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    codes = np.concatenate([np.asarray(a, np.uint8) for a in arrs]) if arrs else np.zeros(0, np.uint8)
    return synth.Reads(lens, codes.astype(np.uint8), offs)


def _tandem(g):
    """Reads that end 20 bases past a run (unique: the call re-seeds from its middle, inside the run)
    or start 20 bases before it."""
    e = HP0 + HPN
    d = DI0 + DIN
    return [g[e - 220:e + 20], g[e - 130:e + 20], g[HP0 - 20:HP0 + 80], g[d - 130:d + 20], g[DI0 - 20:DI0 + 130]]


def _special(g):
    """The hand-made reads, before the window-aligned substitutions (which need the batch's offsets)."""
    out = list(_tandem(g))
    # the exact repeat family: inside a copy, across its edge, with a substitution in the middle
    out += [g[20_100:20_250], g[19_950:20_100], g[61_300:61_451]]
    r = g[20_100:20_250].copy()
    r[75] = (r[75] + 1) & 3
    out.append(r)
    # N: first base, last base, two in a row, all N, N only at the ends of a short read
    for lo, n_at in [(5_000, [0]), (7_000, [149]), (9_000, [10, 11]), (11_000, [0, 1, 148, 149]), (13_000, [70, 71, 72])]:
        r = g[lo:lo + 150].copy()
        r[n_at] = 4
        out.append(r)
    out.append(np.full(50, 4, np.uint8))
    out.append(np.full(1, 4, np.uint8))
    r = g[15_000:15_020].copy()
    r[0] = 4
    out.append(r)  # 19 bases after the N: one call of exactly min_seed_len
    # lengths around min_seed_len and the window size, exact copies
    for k, n in enumerate(LENGTHS):
        out.append(g[30_000 + 200 * k:30_000 + 200 * k + n])
    # split_len = len under `split38`: exact unique 38-mers
    out += [g[40_000 + 100 * k:40_038 + 100 * k] for k in range(4)]
    return out


def _windowed(g, arrs):
    """Append 150-mers and give each a substitution (or an N) where the batch's 16-base window has
    its base 15, 0, 1 or 14 (or 15 / 16 counted from the read's first window): the forward extension of
    the first call ends exactly there."""
    off = int(sum(a.size for a in arrs))
    out = []
    for k, (want, code) in enumerate([(15, None), (0, None), (1, None), (14, None), (15, 4), (0, 4)]):
        r = g[50_000 + 300 * k:50_150 + 300 * k].copy()
        p = next(p for p in range(40, 60) if (off + p) % 16 == want)
        r[p] = (r[p] + 1) & 3 if code is None else code
        out.append(r)
        off += r.size
    return out


@pytest.fixture(scope="module")
def world(gpu_device):
    import smemgpu
    from smemgpu import synth
    g = _genome()
    idx = smemgpu.Index.build(g)
    ref = oracle.OracleIndex(words=idx.words, primary=idx.primary, L2=idx.L2)
    arrs = _special(g)
    arrs += _windowed(g, arrs)
    n_special = len(arrs)
    fill = synth.concat_reads([
        synth.make_reads(g, 120, (1, 200), seed=41, n_rate=0.02),
        synth.make_reads(g, 257 - n_special - 120, 150, seed=42, sub_rate=0.03, random_frac=0.1),
    ])
    arrs += [fill.read(i) for i in range(fill.n)]
    reads = _reads_of(arrs)
    assert reads.n == 257
    truth = {}  # (n reads, option set) -> SMGO stream, per-read counts, counters: computed once, never changed

    def want(n, optname):
        if (n, optname) not in truth:
            sub = reads if n == reads.n else reads.subset(range(n))
            truth[(n, optname)] = (sub,) + tuple(oracle.seed(ref, sub.codes, sub.offs, threads=4, **OPTS[optname]))
        return truth[(n, optname)]

    yield dict(g=g, idx=idx, ref=ref, reads=reads, want=want, device=gpu_device, n_special=n_special)
    ref.close()


def _assert_stream(res, want):
    got = res.to_smgo()
    if got != want:
        from smemgpu import synth
        a, b = synth.read_smgo(got), synth.read_smgo(want)
        bad = [i for i in range(len(b)) if len(a[i]) != len(b[i]) or any(
            x.shape != y.shape or (x != y).any() for x, y in zip(a[i], b[i]))]
        pytest.fail(f"{len(bad)} reads differ, first {bad[:8]}")


def _run(world, reads, optname, intv_cap=0, variant=0):
    import smemgpu
    gpu = smemgpu.Gpu(world["idx"], device=world["device"], intv_cap=intv_cap, variant=variant)
    try:
        assert gpu.variant == (variant or 49)  # 49: the default kernel
        b = gpu.batch(max(1, reads.n), max(16, reads.codes.size), max(1, int(reads.lens.max())))
        b.set_reads(reads.codes, reads.offs)
        b.run(smemgpu.Options(**OPTS[optname]))
        st = b.stats()
        res = b.fetch()
        b.close()
        return res, st
    finally:
        gpu.close()


def test_inputs_reach_the_paths(world):
    """The oracle's view of the inputs (no GPU work): the tandem reads' backward steps exceed the
    owners' LDS list and a wave's lanes, every length and record count is there."""
    from smemgpu import synth
    t = _reads_of(_tandem(world["g"]))
    for k in range(t.n):
        one = t.subset([k])
        _, st = oracle.seed_stats(world["ref"], one.codes, one.offs, **OPTS["default"])
        steps, hi = st["n_bwd_step"], st["n_bwd_task_hi"]
        assert steps > 0 and st["n_step_hist"][16] == steps          # every step has 16 entries or more
        # n_bwd_task_hi counts the extends of entries at index >= ORC_NL: above steps * (m - ORC_NL)
        # some step has more than m entries
        assert hi > steps * (OWN_LIST - ORC_NL), (k, st)
        if k == 0:  # the 240-base homopolymer read: a step that no single iteration of a wave can serve
            assert hi > steps * (64 - ORC_NL), (k, st)
    reads, stream, per, st = world["want"](257, "default")
    assert set(LENGTHS) <= set(int(x) for x in reads.lens)
    assert st["n_fwd_spill"] > 0                                     # forward lists past the LDS ring
    lists = synth.read_smgo(stream)
    assert {0, 1, 2, 3} <= {sum(a.shape[0] for a in calls) for calls in lists}
    assert {1, 2, 3} <= {a.shape[0] for calls in lists for a in calls}
    _, s38, _, _ = world["want"](257, "split38")
    assert s38 != stream                                             # split_len = len re-seeds what the default does not


@pytest.mark.parametrize("n", SIZES)
def test_batch_sizes(world, n):
    reads, want, _, _ = world["want"](n, "default")
    res, st = _run(world, reads, "default")
    assert st["n_overflow"] == 0
    _assert_stream(res, want)


def test_split_len_equals_read_length(world):
    reads, want, _, _ = world["want"](257, "split38")
    res, _ = _run(world, reads, "split38")
    _assert_stream(res, want)


@pytest.mark.parametrize("intv_cap", [2, 3])
def test_overflow_pass(world, intv_cap):
    reads, want, _, _ = world["want"](257, "default")
    res, st = _run(world, reads, "default", intv_cap=intv_cap)
    assert st["n_overflow"] > 0
    _assert_stream(res, want)


def test_run_after_run_on_one_batch(world):
    """Three launches on one batch object: all reads, the first 25, all again.  Nothing of a launch
    (claims, pending records, lists, windows) may survive into the next."""
    import smemgpu
    big, want_big, _, _ = world["want"](257, "default")
    small, want_small, _, _ = world["want"](25, "default")
    gpu = smemgpu.Gpu(world["idx"], device=world["device"])
    try:
        b = gpu.batch(big.n, big.codes.size, int(big.lens.max()))
        for reads, want in [(big, want_big), (small, want_small), (big, want_big)]:
            b.set_reads(reads.codes, reads.offs)
            b.run(smemgpu.Options(**OPTS["default"]))
            _assert_stream(b.fetch(), want)
        b.close()
    finally:
        gpu.close()


@pytest.mark.parametrize("variant", [63, 64, 65, 66, 67])
def test_diet_arms_taken_out(world, variant):
    """The code each arm of the instruction diet replaced stays behind its OPT bit (variants 63-66 take
    one arm out, 67 all four: the kernel before the diet) and stays bit-exact.  The product library
    instantiates the default only; these need `make -C bwa-mem-harp2_amd AB=1` (lib_ab/, run with
    SMEMGPU_LIB), as tests/test_gpu_parity.py's A/B variants do."""
    import smemgpu
    if not smemgpu.load().smem_seed_variant_built(variant):
        pytest.skip(f"A/B variant {variant} is not in this build (make AB=1)")
    for optname in OPTS:
        reads, want, _, _ = world["want"](257, optname)
        res, _ = _run(world, reads, optname, variant=variant)
        _assert_stream(res, want)
    reads, want, _, _ = world["want"](257, "default")
    res, st = _run(world, reads, "default", intv_cap=2, variant=variant)
    assert st["n_overflow"] > 0
    _assert_stream(res, want)
