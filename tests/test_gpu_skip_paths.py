"""The skipping kernel's paths around a call's first dp bases and its step probes (seed_wp_kernel SKIP,
variant 68; DESIGN.md §5 "The skipping arm's fixed cost"), bit for bit against the restatement through
the public batch API.

The cases aim at what the kernel's bookkeeping can get wrong when its phases and flags are rearranged,
beyond the seams tests/test_gpu_kmer_skip.py and test_gpu_kmer_edge.py already walk: the collection of a
call's first bases across two query windows at every offset of the 16-byte window, an ambiguous base at
every distance from 1 to dp + 1 of a call's start, reads shorter than dp and shorter than min_seed_len,
calls that reach their end (i == -1 or an ambiguous base) while virtual entries are left, steps of more
than a wave's 64 tasks (the probe, ranked last, then falls in a later chunk than the first entries) and an
option set whose re-seeding depth differs from the first calls'.  Every case runs at each table depth from
2 to the index's own D, and at depth 1 (the plain path inside the skipping kernel), on a 400 kbp index.

Two states the kernel has a path for are NOT reachable on a handle whose depths the host chose, and so
cannot be asserted present: a step, or a call's end, with *only* virtual entries left (prev_n == 0: the
probe-only step and the P_KEND probe).  Up to dp bases no string's interval falls below min_intv, so a
stored entry dies only with more than dp bases; the stored entries continue the virtual ones without a
gap in length (the start probe's string of d bases is stored, the forward lengths 1 .. d - 1 are virtual,
and once the longest virtual entry has reached dp bases every later step probes the next one, whose string
of exactly dp bases survives that step).  Hence while a virtual entry is left, the shortest stored one has
at most dp bases and survives.  What is reachable, and asserted here, is the end of a call with virtual
entries left beside a stored one.
"""
import numpy as np
import pytest

from oracle import oracle

pytestmark = pytest.mark.gpu

OPTS = {
    "default": dict(min_seed_len=19, split_factor=1.5, split_width=10, start_width=1),
    "short": dict(min_seed_len=3, split_factor=1.0, split_width=500, start_width=1),
    "wide": dict(min_seed_len=19, split_factor=1.0, split_width=500, start_width=1),
}
RUN_AT, RUN_LEN = 123_456, 200   # a homopolymer run written into the genome, a C on either side


@pytest.fixture(scope="module")
def world(gpu_device):
    import smemgpu
    from smemgpu import synth
    g = synth.make_genome(400_000, seed=21).codes.copy()
    g[RUN_AT - 1] = g[RUN_AT + RUN_LEN] = 1
    g[RUN_AT:RUN_AT + RUN_LEN] = 0
    idx = smemgpu.Index.build(g)
    ref = oracle.OracleIndex(words=idx.words, primary=idx.primary, L2=idx.L2)
    gpu = smemgpu.Gpu(idx, device=gpu_device)
    d0 = gpu.kmer_facts()["D"]
    assert d0 >= 6, d0   # a 400 kbp text holds every string of 7 bases
    yield dict(g=g, idx=idx, ref=ref, gpu=gpu, d0=d0)
    gpu.close()
    ref.close()


def _one(arr):
    from smemgpu import synth
    arr = np.asarray(arr, np.uint8)
    return synth.Reads(np.array([arr.size], np.int32), arr, np.array([0, arr.size], np.int64))


def _diff(got, want):
    from smemgpu import synth
    a, b = synth.read_smgo(got), synth.read_smgo(want)
    bad = [i for i in range(len(b)) if len(a[i]) != len(b[i]) or any(
        x.shape != y.shape or (x != y).any() for x, y in zip(a[i], b[i]))]
    return f"{len(bad)} reads differ, first {bad[:8]}"


def _check_all_depths(world, reads, optname, want=None):
    """The batch on the skipping kernel at every table depth 1 .. D against the restatement's stream
    (computed once); returns the restatement's (stream, per-read counts, stats) and the depths run."""
    import smemgpu
    gpu, o = world["gpu"], OPTS[optname]
    if want is None:
        want = oracle.seed(world["ref"], reads.codes, reads.offs, threads=4, **o)
    depths = []
    for k in range(1, world["d0"] + 1):
        gpu.set_variant(68)
        gpu.set_kmer_table(k)
        assert gpu.seed_kernel == 68
        dp0 = gpu.kmer_probe_depth(o["start_width"])["depth"]
        dp1 = gpu.kmer_probe_depth(o["split_width"] + 1)["depth"]
        assert dp0 == k, (k, dp0)    # the first calls run at the table's depth (k == 1: the plain path)
        depths.append((dp0, dp1))
        got = smemgpu.seed(gpu, reads.codes, reads.offs, smemgpu.Options(**o)).to_smgo()
        assert got == want[0], (optname, k, dp0, dp1, _diff(got, want[0]))
    return want, depths


def _first_call_start(q):
    """Where a read's first bwt_smem1 call starts: its first unambiguous base."""
    ok = np.flatnonzero(np.asarray(q) < 4)
    return int(ok[0]) if ok.size else -1


def test_first_bases_across_two_query_windows(world):
    """A call's first dp bases lie in one 16-byte query window or cross into the next, with the call's start
    at every offset of the window: reads of varied lengths follow each other, so (o0 + x) & 15 takes all 16
    values, for calls that start a read and for calls that start after an ambiguous base."""
    from smemgpu import synth
    g, d0 = world["g"], world["d0"]
    parts = []
    for j in range(96):
        q = g[5000 + 97 * j:5000 + 97 * j + 41 + (j * 7) % 13].copy()
        if j % 3 == 1:
            q[:4] = 4            # the first call starts at x = 4
        elif j % 3 == 2:
            q[9] = 4             # a second call starts at x = 10, after the ambiguous base
        parts.append(_one(q))
    reads = synth.concat_reads(parts)
    res_first, res_after = set(), set()
    for r in range(reads.n):
        q, o0 = reads.read(r), int(reads.offs[r])
        res_first.add((o0 + _first_call_start(q)) & 15)
        if r % 3 == 2:
            res_after.add((o0 + 10) & 15)
    assert res_first == set(range(16)) and res_after == set(range(16)), (res_first, res_after)
    for dp in range(2, d0 + 1):   # at every depth some calls' first dp bases cross the window's end, others do not
        assert any(r + dp > 16 for r in res_first) and any(r + dp <= 16 for r in res_first)
    want, _ = _check_all_depths(world, reads, "default")
    assert all(int(n) >= 1 for n in want[1]["n_calls"])


def test_ambiguous_base_after_a_call_start(world):
    """An ambiguous base at x + 1 (the call probes nothing: the plain path) and at each of x + 2 .. x + D + 1
    (the start probe of 2 .. D bases, and the first one clear of it), for a call that starts a read (x = 0)
    and one that starts after an ambiguous base (x = 7)."""
    from smemgpu import synth
    g, d0 = world["g"], world["d0"]
    parts, seen = [], set()
    for x in (0, 7):
        for off in range(1, d0 + 2):
            q = g[20_000 + 61 * off:20_000 + 61 * off + 70].copy()
            if x:
                q[x - 1] = 4
            q[x + off] = 4
            parts.append(_one(q))
            assert _first_call_start(q) == 0 and (x == 0 or q[x - 1] == 4) and q[x + off] == 4 and (q[x:x + off] < 4).all()
            seen.add((x, off))
    assert seen == {(x, off) for x in (0, 7) for off in range(1, d0 + 2)}
    reads = synth.concat_reads(parts)
    want, _ = _check_all_depths(world, reads, "default")
    # the stretch after the ambiguous base is long enough for a match: every read has calls on both sides
    assert all(int(n) >= 2 for n in want[1]["n_calls"])
    _check_all_depths(world, reads, "short")   # min_seed_len 3: the stretches of 1 .. D bases are reported too


def test_reads_shorter_than_the_depth_and_than_min_seed_len(world):
    """Reads of 1 .. D bases (shorter than dp: the start probe takes the whole read, or the plain path does)
    and of D + 1 .. 18 bases, under min_seed_len 19 (the kernel drops them whole) and under min_seed_len 3
    (they run: a read of L < dp bases is one probe of L bases and L - 1 virtual entries to its end)."""
    from smemgpu import synth
    g, d0 = world["g"], world["d0"]
    parts = [_one(g[30_000 + 37 * L:30_000 + 37 * L + L]) for L in range(1, 19) for _ in range(2)]
    parts.append(synth.make_reads(g, 64, (1, 18), seed=31, n_rate=0.05))
    parts.append(synth.make_reads(g, 32, 150, seed=32))            # ordinary reads among them
    reads = synth.concat_reads(parts)
    assert (reads.lens < 2).any() and all((reads.lens == L).any() for L in range(1, 19))
    assert (reads.lens < d0).any() and ((reads.lens >= d0) & (reads.lens < 19)).any()
    want, _ = _check_all_depths(world, reads, "default")
    assert all(int(n) == 0 for n, L in zip(want[1]["n_intv"], reads.lens) if L < 19)
    want, _ = _check_all_depths(world, reads, "short")
    n_intv = np.asarray(want[1]["n_intv"])
    assert all(n_intv[r] >= 1 for r in range(36) if 3 <= reads.lens[r] < d0)   # reads shorter than dp are reported


def test_calls_that_end_with_virtual_entries_left(world):
    """A call's end while virtual entries are left (see the module docstring for what cannot occur):
    the end at i == -1 at once (x = 0), at an ambiguous base at once (x after an N), and -- re-seeding
    calls of reads of 6 .. 2 D bases under min_seed_len 3, which start in the read's middle -- after backward
    steps that probed some virtual entries and left the shortest ones."""
    from smemgpu import synth
    g, d0 = world["g"], world["d0"]
    parts = []
    for L in range(6, 2 * d0 + 1):
        for rep in range(3):
            parts.append(_one(g[40_000 + 53 * L + 17 * rep:40_000 + 53 * L + 17 * rep + L]))
    for L in range(6, 2 * d0 + 1):   # the same behind an ambiguous base: the backward phase ends there, not at -1
        parts.append(_one(np.concatenate([g[41_000:41_005], [4], g[42_000 + 53 * L:42_000 + 53 * L + L]])))
    reads = synth.concat_reads(parts)
    want, depths = _check_all_depths(world, reads, "short")
    lists = synth.read_smgo(want[0])
    n_plain = 3 * (2 * d0 - 5)
    # a re-seeding call ran and kept a sub-match (a list of several intervals: a whole read that matches gives
    # one) in reads short enough for its start, the match's middle, to lie fewer than dp1 - 1 bases from the
    # read's start: its shortest virtual entries never reach dp1 bases
    dp1 = max(d1 for _, d1 in depths)
    assert dp1 >= 4
    reseeded = [r for r in range(n_plain) if max(a.shape[0] for a in lists[r]) >= 2 and reads.lens[r] // 2 + 1 < dp1]
    assert reseeded, (dp1, [[a.shape[0] for a in c] for c in lists[:n_plain]])
    behind = range(n_plain, reads.n)   # behind the N: calls on both sides of it, and a re-seeding call that kept a sub-match
    assert all(len(lists[r]) >= 2 for r in behind) and any(max(a.shape[0] for a in lists[r]) >= 2 for r in behind)


def test_steps_of_more_than_a_waves_tasks(world):
    """A homopolymer read inside the genome's run of 200: every forward extend changes the interval's size,
    so a call's list holds one entry per base and a backward step has more than 64 tasks, in several chunks,
    the step's probe in the last."""
    from smemgpu import synth
    g, d0 = world["g"], world["d0"]
    assert (g[RUN_AT:RUN_AT + RUN_LEN] == 0).all() and g[RUN_AT - 1] == 1 and g[RUN_AT + RUN_LEN] == 1
    # occurrences of A^L on both strands, from the text's runs of A and of T: strictly falling up to the run's length
    t = np.concatenate([[1], synth.forward_reverse_text(g), [1]])
    edge = np.flatnonzero(np.diff((t == 0).astype(np.int8)))
    runs = edge[1::2] - edge[0::2]             # the lengths of the text's runs of A
    occ = [int(np.maximum(runs - L + 1, 0).sum()) for L in range(1, 121)]
    assert all(x > y for x, y in zip(occ, occ[1:])) and occ[-1] >= RUN_LEN - 120 + 1
    q = np.zeros(150, np.uint8)
    q[30] = 2                                   # A^30 G A^119: G A.. ends within a few bases, the next call starts in the run
    tail = _one(np.concatenate([np.zeros(100, np.uint8), g[RUN_AT + RUN_LEN:RUN_AT + RUN_LEN + 50]]))
    parts = [_one(q), _one(np.zeros(150, np.uint8)), tail, synth.make_reads(g, 40, 150, seed=33)]
    reads = synth.concat_reads(parts)
    want1 = oracle.seed(world["ref"], parts[0].codes, parts[0].offs, **OPTS["default"])
    st = want1[2]
    # the read's last call starts past the G with about 110 bases of the run ahead: that many pushes, and
    # backward steps (the bases between the G's match and the call's start) over the whole list
    assert st["n_fwd_push"] >= 30 + 100, st["n_fwd_push"]
    assert st["n_step_hist"][16] >= 1 and st["n_bwd_task_hi"] >= 64, (st["n_step_hist"], st["n_bwd_task_hi"])
    _check_all_depths(world, reads, "default")
    _check_all_depths(world, reads, "wide")


def test_reseeding_depth_differs_from_the_first_calls(world):
    """split_width 500: a re-seeding call's min_intv may be 501, which only a shallower level's smallest
    interval reaches, so the kernel runs a read's first calls and its re-seeding calls at different depths."""
    from smemgpu import synth
    g, d0, gpu = world["g"], world["d0"], world["gpu"]
    reads = synth.concat_reads([synth.make_reads(g, 1500, 150, seed=34, sub_rate=0.05),
                                synth.make_reads(g, 300, (19, 60), seed=35, n_rate=0.01)])
    want, depths = _check_all_depths(world, reads, "wide")
    dp0, dp1 = depths[-1]   # at the index's own depth
    assert dp0 == d0 and 2 <= dp1 < dp0, depths
    assert any(a != b for a, b in depths) and any(b >= 2 for _, b in depths)
    # re-seeding calls ran and kept sub-matches (the restatement's lists show calls of several intervals)
    assert max(a.shape[0] for calls in synth.read_smgo(want[0]) for a in calls) > 1
    assert int(np.asarray(want[1]["n_calls"]).sum()) > reads.n
    _check_all_depths(world, reads, "default")
