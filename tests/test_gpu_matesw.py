"""smem_matesw on the GPU against tests/matesw_ref.py (the restatement of
software/bwamem_pair.c:109-175, 252-263 that tests/test_matesw.py pins): both
ends' lists, their offsets, n_sw and status equal, on the hand-built pairs of
tests/matesw_data.py -- one group per branch, each group's size and what it
reaches asserted -- and on the paired-end set of tests/golden/msw.  On every batch
of tests/golden/msw/hand the device's lists and n_sw are also compared with the
reference's own mem_matesw (run_fixture)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import matesw_data as D
from tests import matesw_ref as R
from tests import regfin_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def world(gpu_device):
    import smemgpu
    G = D.genome()
    gpu = smemgpu.Gpu(smemgpu.Index.build(G), device=gpu_device)
    yield {"G": G, "pac": D.pack(G), "gpu": gpu, "all": D.build(G), "fr": D.build_fr(G)}
    gpu.close()


def c_opt(o: R.Opt):
    from smemgpu import synth
    from smemgpu.lib import matesw_opt
    return matesw_opt(mat=synth.bwa_scmat(o.a, o.b), o_del=o.o_del, e_del=o.e_del, o_ins=o.o_ins, e_ins=o.e_ins, a=o.a,
                      min_seed_len=o.min_seed_len, pen_unpaired=o.pen_unpaired, max_matesw=o.max_matesw,
                      mask_level_redun=o.mask_level_redun)


def c_pes(pes):
    return [(p.low, p.high, p.failed) for p in pes]


def run_both(world, P, pes, opt, l_pac=D.L_PAC):
    codes, offs, regs, reg_off = P.arrays()
    want = R.matesw(opt, l_pac, world["G"], pes, codes, offs, regs, reg_off)
    got = world["gpu"].matesw(world["pac"], l_pac, codes, offs, regs, reg_off, c_pes(pes), c_opt(opt))
    return got, want, (codes, offs, regs, reg_off)


def run_fixture(world, name):
    """a batch of tests/golden/msw/hand on the GPU: equal to the restatement (whose result
    tests/test_matesw.py computes, once), and to the reference's own lists and n where the pair stays
    on the device; a pair left to the host comes back as it went in.  Returns (got, want, arrays, Case)."""
    from tests import test_matesw as T
    G, l_pac, case, arrays, ref, want = T.hand(name)
    codes, offs, regs, reg_off = arrays
    got = world["gpu"].matesw(D.pack(G), l_pac, codes, offs, regs, reg_off, c_pes(case.pes), c_opt(case.opt))
    same(got, want)
    out, off, n_sw, status, ms = got
    r_regs, r_off, r_n = ref
    for p in range(status.size):
        mine = out[int(off[2 * p]):int(off[2 * p + 2])]
        if status[p] == 0:
            assert n_sw[p] == r_n[p] and np.array_equal(off[2 * p:2 * p + 3] - off[2 * p], r_off[2 * p:2 * p + 3] - r_off[2 * p])
            assert mine.tobytes() == r_regs[int(r_off[2 * p]):int(r_off[2 * p + 2])].tobytes(), (name, p, case.pairs.group[p])
        else:
            assert status[p] == R.MSW_HOST and n_sw[p] == 0
            assert mine.tobytes() == regs[int(reg_off[2 * p]):int(reg_off[2 * p + 2])].tobytes(), (name, p, case.pairs.group[p])
    return got, want, arrays, case


def same(got, want):
    out, off, n_sw, status, ms = got
    lists, w_sw, w_st, _ = want
    w_off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint64)
    bad = [p for p in range(len(w_sw)) if n_sw[p] != w_sw[p] or status[p] != w_st[p]]
    assert not bad, f"n_sw / status differ for pairs {bad[:10]}: got {[(int(n_sw[p]), int(status[p])) for p in bad[:10]]}, " \
                    f"want {[(w_sw[p], w_st[p]) for p in bad[:10]]}"
    assert np.array_equal(off, w_off), f"reg_off_out differs first at read {int(np.nonzero(off != w_off)[0][0])}"
    assert out.size == int(w_off[-1])
    k = 0
    for r, lst in enumerate(lists):
        for x in lst:
            for f in regfin_ref.FIELDS:
                assert int(out[k][f]) == x[f], f"read {r}, region {k - int(w_off[r])}: {f} {int(out[k][f])} != {x[f]}"
            k += 1


def test_matesw_every_orientation_open(world):
    P = world["all"]
    run_fixture(world, "all_base")
    got, want, (codes, offs, regs, reg_off) = run_both(world, P, D.PES_ALL, R.Opt())
    same(got, want)
    out, off, n_sw, status, ms = got
    lists, w_sw, w_st, tr = want
    assert ms > 0
    sizes = {g: len(P.of(g)) for g in dict.fromkeys(P.group)}
    assert sizes == {"rescue_FF": 10, "rescue_FR": 10, "rescue_RF": 10, "rescue_RR": 10, "rescue_end0": 10,
                     "rescue_rev_anchor": 10, "clip_0": 10, "clip_2l": 10, "bridge": 10, "below": 10, "empty": 5,
                     "long250": 10, "dedup_drops_old": 10, "dedup_drops_new": 10, "host_300": 3}
    for r, name in enumerate(("FF", "FR", "RF", "RR")):
        for p in P.of("rescue_" + name):       # four SWs from the one anchor, the hit in orientation r
            assert (tr[p].sw, tr[p].inserted, n_sw[p]) == (4, 1, 4) and sorted(tr[p].dirs) == [0, 1, 2, 3]
            a, hit = P.lists[2 * p][0], lists[2 * p + 1]
            assert len(hit) == 1 and hit[0]["secondary"] == -1 and hit[0]["score"] >= 100
            assert R.infer_dir(D.L_PAC, a["rb"], hit[0]["rb"])[0] == r
    for p in P.of("rescue_end0"):
        assert len(lists[2 * p]) == 1 and n_sw[p] == 4
    for p in P.of("rescue_rev_anchor"):
        assert len(lists[2 * p + 1]) == 1 and lists[2 * p + 1][0]["rb"] < D.L_PAC
    assert all(tr[p].clipped >= 2 and tr[p].inserted == 1 for p in P.of("clip_0") + P.of("clip_2l"))
    assert all(tr[p].bridged == 2 and n_sw[p] == 2 for p in P.of("bridge"))
    for p in P.of("below"):                    # nothing inserted, every SW counted
        assert (tr[p].below, tr[p].inserted, n_sw[p]) == (4, 0, 4) and off[2 * p + 2] == off[2 * p + 1]
    assert all(n_sw[p] == 0 and off[2 * p + 2] == off[2 * p] for p in P.of("empty"))
    assert all(tr[p].word == 4 and tr[p].byte == 0 and tr[p].inserted == 1 for p in P.of("long250"))
    for p in P.of("dedup_drops_old"):          # the partial hit goes, the rescued one stays
        assert tr[p].dedup_drop == 2 and [x["score"] for x in lists[2 * p + 1]] == [150]
    for p in P.of("dedup_drops_new"):          # the rescued hit goes
        assert tr[p].dedup_drop == 2 and [x["score"] for x in lists[2 * p + 1]] == [200]
    host = [p for p in range(len(w_st)) if status[p] == R.MSW_HOST]
    assert host == P.of("host_300")
    for p in host:                             # lists copied through
        lo, hi = int(reg_off[2 * p]), int(reg_off[2 * p + 2])
        assert n_sw[p] == 0 and np.array_equal(out[int(off[2 * p]):int(off[2 * p + 2])], regs[lo:hi])


def test_matesw_only_fr_open(world):
    P = world["fr"]
    run_fixture(world, "fr_base")
    got, want, (codes, offs, regs, reg_off) = run_both(world, P, D.PES_FR, R.Opt())
    same(got, want)
    out, off, n_sw, status, ms = got
    lists, w_sw, w_st, tr = want
    sizes = {g: len(P.of(g)) for g in dict.fromkeys(P.group)}
    assert sizes == {"consistent": 20, "second_anchor_skips": 10, "two_anchors": 10, "rescue_FR": 10}
    assert not status.any()
    for p in P.of("consistent"):               # no SW: the lists byte for byte
        lo, hi = int(reg_off[2 * p]), int(reg_off[2 * p + 2])
        assert tr[p].calls == 0 and n_sw[p] == 0
        assert out[int(off[2 * p]):int(off[2 * p + 2])].tobytes() == regs[lo:hi].tobytes()
    for p in P.of("second_anchor_skips"):      # the first anchor's hit fills FR for the second
        assert (tr[p].calls, tr[p].all_skipped, tr[p].inserted, n_sw[p]) == (1, 1, 1, 1)
    for p in P.of("two_anchors"):              # the third region is below the floor
        assert (tr[p].calls, tr[p].sw, tr[p].inserted, n_sw[p]) == (2, 2, 1, 2)
    assert all(n_sw[p] == 1 for p in P.of("rescue_FR"))


def test_matesw_a2_scoring(world):
    """-A 2 scaling: queries of 150 bp take the 16-bit branch, min_seed_len * a is the threshold"""
    P = world["all"]
    opt = R.Opt(a=2, b=8, o_del=12, e_del=2, o_ins=12, e_ins=2)
    got, want, _ = run_both(world, P, D.PES_ALL, opt)
    same(got, want)
    tr = want[3]
    assert sum(t.word for t in tr) >= 300 and sum(t.inserted for t in tr) >= 100
    assert all(want[0][2 * p + 1][0]["score"] >= 200 for p in P.of("rescue_FR"))
    for name in ["all_a2", "fr_a2"] + [f"{c}_a2" for c in D.EDGE_SIZES]:
        run_fixture(world, name)


def test_matesw_one_anchor_no_margin(world):
    """max_matesw = 1 and pen_unpaired = 0: one anchor per end, and only regions that tie the best"""
    P = world["fr"]
    for opt, calls in ((R.Opt(max_matesw=1), 1), (R.Opt(pen_unpaired=0), 1), (R.Opt(max_matesw=0), 0)):
        got, want, _ = run_both(world, P, D.PES_FR, opt)
        same(got, want)
        assert all(want[3][p].calls == calls for p in P.of("two_anchors"))
    got, want, _ = run_both(world, world["all"], D.PES_ALL, R.Opt(max_matesw=1, pen_unpaired=0))
    same(got, want)
    for name in [f"{b}_{o}" for b in ("all", "fr") for o in ("one_anchor", "no_margin", "no_anchor")] + \
            [f"{c}_one_anchor" for c in D.EDGE_SIZES]:
        run_fixture(world, name)


def test_matesw_window_past_the_limit(world):
    """bounds whose windows pass SMEM_KSWA_MAX_TLEN: every pair that would run an SW is the host's"""
    P = world["all"]
    got, want, (codes, offs, regs, reg_off) = run_both(world, P, D.PES_WIDE, R.Opt())
    same(got, want)
    out, off, n_sw, status, ms = got
    host = [p for p in range(status.size) if status[p] == R.MSW_HOST]
    assert set(host) == set(range(status.size)) - set(P.of("empty"))
    assert not n_sw.any() and np.array_equal(off, reg_off) and out.tobytes() == regs.tobytes()


@pytest.mark.parametrize("name", sorted(D.EDGE_SIZES))
def test_matesw_edges(world, name):
    """the groups of matesw_data.build_edges (tests/test_matesw.py asserts what each reaches)"""
    got, want, (codes, offs, regs, reg_off), case = run_fixture(world, name + "_base")
    out, off, n_sw, status, ms = got
    P = case.pairs
    host = {"long": P.of("long_1024_host") + P.of("two_1023_host"), "roll": list(range(status.size)),
            "window": P.of("win_2049")}.get(name, [])
    assert [p for p in range(status.size) if status[p]] == sorted(host)
    if name == "roll":       # every pair rolled back after an insertion: the batch as it came
        assert not n_sw.any() and np.array_equal(off, reg_off) and out.tobytes() == regs.tobytes()
    if name == "both":
        assert all(n_sw[p] == 2 and off[2 * p + 1] - off[2 * p] == 2 and off[2 * p + 2] - off[2 * p + 1] == 2
                   for p in range(status.size))
    if name == "long":
        (p,) = P.of("long_1023")
        assert off[2 * p + 2] - off[2 * p + 1] == R.MAX_REGS


@pytest.mark.parametrize("l_pac", D.L_PAC_ODD)
def test_matesw_l_pac_not_a_multiple_of_4(world, l_pac):
    """the last .pac byte partly filled, and windows that end at, start at and pass l_pac"""
    got, want, _, case = run_fixture(world, f"lpac{l_pac}_base")
    assert l_pac % 4 and not got[3].any() and sum(t.inserted for t in want[3]) == 4


def waves_per_cu():
    import re
    with open(os.path.join(ROOT, "bwa-mem-harp2_amd", "csrc", "matesw_kernels.h")) as fh:
        m = re.search(r"MSW_WAVES_PER_CU\s*=\s*(\d+)", fh.read())
    assert m, "csrc/matesw_kernels.h no longer spells MSW_WAVES_PER_CU = <n>: tell this test where the grid's size is"
    return int(m.group(1))


def test_matesw_more_pairs_than_the_grid(world):
    """three rounds of the wave kernel's grid and a few pairs more: every block takes a second and a
    third pair with what the one before left in LDS and scratch.  The kernel strides over the wave
    list, which holds the pairs the pre-pass did not settle, so the kinds are laid out along that
    list: 13 listed kinds of build_fr and build_edges in turn (a 129-region list, then an empty one;
    a 256 bp word-mode mate, then one of 20 bp; an inserting pair, then one that stays below), a
    period coprime to the grid's size, two of the 1000-region lists in place of two of them, and a
    settled pair after every twelfth, so that the wave list is a strict subset of the batch.  With
    the wave list in batch order no block meets the same kind twice (asserted); the atomic counter
    that fills the list may reorder neighbours, and then about one successor in 13 is of the same
    kind.  Equal to the restatement (computed once per distinct pair), and a second run byte for
    byte: the wave list's order does not matter."""
    import math
    from smemgpu.lib import ALNREG_DT
    from tests import test_matesw as T
    slots = waves_per_cu() * world["gpu"].cu_count()
    n_pairs = 3 * slots + 17
    G, fr = world["G"], world["fr"]
    opt = R.Opt(max_matesw=2)
    edges = {n: T.hand(n + "_base")[2].pairs for n in D.EDGE_SIZES}

    def pick(P, group, k=0):
        p = P.of(group)[k]
        return P.reads[2 * p], P.lists[2 * p], P.reads[2 * p + 1], P.lists[2 * p + 1]

    kinds = [pick(edges["long"], "long_129"), pick(fr, "rescue_FR"), pick(edges["short"], "short_256"),
             pick(edges["short"], "short_20"), pick(fr, "rescue_FR", 1), pick(edges["short"], "short_18"),
             pick(edges["long"], "long_128"), pick(edges["both"], "both"), pick(edges["long"], "long_65"),
             pick(fr, "two_anchors"), pick(edges["equal"], "equal", 1), pick(edges["n"], "n_5_FR"),
             pick(fr, "second_anchor_skips")]
    n_listed = len(kinds)
    kinds += [pick(edges["long"], "long_1000"), pick(edges["long"], "long_1023"), pick(fr, "consistent")]
    big, settled = (n_listed, n_listed + 1), n_listed + 2
    assert math.gcd(n_listed, slots) == 1, "choose a number of listed kinds coprime to the grid's size"
    order, i = [], 0
    while len(order) < n_pairs:
        order.append(big[0] if i == slots // 3 else big[1] if i == 2 * slots + 5 else i % n_listed)
        i += 1
        if i % 12 == 0 and len(order) < n_pairs:
            order.append(settled)
    order = np.array(order)

    def regs_of(lst):
        a = np.zeros(len(lst), dtype=ALNREG_DT)
        for k, x in enumerate(lst):
            for f in regfin_ref.FIELDS:
                a[k][f] = x[f]
        return a

    one, res = [], []
    for r0, l0, r1, l1 in kinds:             # each kind: its arrays, and the restatement of it alone
        P = D.Pairs()
        P.add("x", r0, l0, r1, l1)
        lists, n, st, tr = R.matesw(opt, D.L_PAC, G, D.PES_FR, *P.arrays())
        assert st[0] == 0
        one.append((r0, r1, regs_of(l0), regs_of(l1)))
        res.append((regs_of(lists[0]), regs_of(lists[1]), n[0], n[0] > 0 or lists[0] != l0 or lists[1] != l1, tr[0].calls))
    reads = [x for k in order for x in one[k][:2]]
    rl = [x for k in order for x in one[k][2:]]
    codes = np.concatenate(reads)
    offs = np.concatenate([[0], np.cumsum([x.size for x in reads])]).astype(np.uint64)
    regs = np.concatenate(rl)
    reg_off = np.concatenate([[0], np.cumsum([x.size for x in rl])]).astype(np.uint64)
    wl = [x for k in order for x in res[k][:2]]
    w_regs = np.concatenate(wl)
    w_off = np.concatenate([[0], np.cumsum([x.size for x in wl])]).astype(np.uint64)
    w_sw = np.array([res[k][2] for k in order], dtype=np.int32)
    # the test's own preconditions: the kinds meant for the wave list are listed (an anchor gets past the skip
    # test) and do something, the settled one is not; more than two rounds of the grid do something; and along
    # the wave list in batch order a block's next pair, `slots` entries on, is never of the kind it just ran
    assert all(res[k][4] > 0 and res[k][3] for k in range(settled)) and res[settled][4] == 0 and not res[settled][3]
    wave = order[order != settled]
    assert wave.size > 2 * slots and 0 < n_pairs - wave.size
    assert (wave[:-slots] != wave[slots:]).all() and (wave[:-2 * slots] != wave[2 * slots:]).all()
    args = (world["pac"], D.L_PAC, codes, offs, regs, reg_off, c_pes(D.PES_FR), c_opt(opt))
    out, off, n_sw, status, ms = world["gpu"].matesw(*args)
    assert not status.any() and np.array_equal(n_sw, w_sw)
    assert np.array_equal(off, w_off)
    bad = np.nonzero(out != w_regs)[0]
    assert bad.size == 0, (int(bad[0]), out[bad[0]], w_regs[bad[0]])
    again = world["gpu"].matesw(*args)
    assert again[0].tobytes() == out.tobytes() and np.array_equal(again[1], off) and np.array_equal(again[2], n_sw)


def test_matesw_golden_pairs(world):
    """the paired-end set the reference's SAM pins (tests/test_matesw.py): no pair left to the host"""
    from tests import test_matesw as T
    S = T.load_set()
    codes, offs, regs, reg_off = S["arrays"]
    want = R.matesw(R.Opt(), S["l_pac"], S["G"], S["pes"], codes, offs, regs, reg_off)
    got = world["gpu"].matesw(S["pac"], S["l_pac"], codes, offs, regs, reg_off, c_pes(S["pes"]), c_opt(R.Opt()))
    same(got, want)
    assert not got[3].any()
    assert sum(want[1]) >= 40


def test_matesw_contract(world):
    import smemgpu
    from smemgpu.lib import SMEM_E_CAPACITY, load
    P = world["fr"]
    gpu, pac = world["gpu"], world["pac"]
    codes, offs, regs, reg_off = P.arrays()
    pes, opt = c_pes(D.PES_FR), c_opt(R.Opt())
    full = gpu.matesw(pac, D.L_PAC, codes, offs, regs, reg_off, pes, opt)
    need = int(full[1][-1])
    assert need > int(reg_off[-1])
    with pytest.raises(smemgpu.SmemError) as e:         # too small: the size comes back, and works
        gpu.matesw(pac, D.L_PAC, codes, offs, regs, reg_off, pes, opt, regs_cap=need - 1, grow=False)
    assert e.value.n_regs == need
    again = gpu.matesw(pac, D.L_PAC, codes, offs, regs, reg_off, pes, opt, regs_cap=e.value.n_regs, grow=False)
    assert again[0].tobytes() == full[0].tobytes() and np.array_equal(again[1], full[1])
    grown = gpu.matesw(pac, D.L_PAC, codes, offs, regs, reg_off, pes, opt, regs_cap=1)
    assert grown[0].tobytes() == full[0].tobytes()
    # a batch of which some pairs are the host's (copied through) and others grow
    from tests import test_matesw as T
    case = T.hand("window_base")[2]
    w_args = (pac, D.L_PAC) + case.pairs.arrays() + (c_pes(case.pes), c_opt(case.opt))
    w_full = gpu.matesw(*w_args)
    lens_in, lens_out = np.diff(w_args[5].astype(np.int64)), np.diff(w_full[1].astype(np.int64))
    assert 0 < int(w_full[3].sum()) < w_full[3].size and (lens_out > lens_in).any()
    assert all((lens_out[2 * p:2 * p + 2] == lens_in[2 * p:2 * p + 2]).all() for p in np.nonzero(w_full[3])[0])
    w_need = int(w_full[1][-1])
    with pytest.raises(smemgpu.SmemError) as e:
        gpu.matesw(*w_args, regs_cap=w_need - 1, grow=False)
    assert e.value.n_regs == w_need
    for cap in (dict(regs_cap=w_need, grow=False), dict(regs_cap=1)):
        w_again = gpu.matesw(*w_args, **cap)
        assert w_again[0].tobytes() == w_full[0].tobytes() and np.array_equal(w_again[1], w_full[1])
        assert np.array_equal(w_again[3], w_full[3])
    # no pairs
    e0 = gpu.matesw(pac, D.L_PAC, np.zeros(0, np.uint8), np.zeros(1, np.uint64), regs[:0], np.zeros(1, np.uint64), pes, opt)
    assert e0[0].size == 0 and e0[1].tolist() == [0] and e0[2].size == 0

    def bad(**kw):
        a = dict(pac=pac, l_pac=D.L_PAC, codes=codes, offs=offs, regs=regs, reg_off=reg_off, pes=pes, opt=opt)
        a.update(kw)
        with pytest.raises(smemgpu.SmemError):
            gpu.matesw(a["pac"], a["l_pac"], a["codes"], a["offs"], a["regs"], a["reg_off"], a["pes"], a["opt"])

    o2 = offs.copy()
    o2[3] = o2[2] - 1
    bad(offs=o2)                                        # offsets that do not ascend
    r2 = reg_off.copy()
    r2[1], r2[2] = r2[2], r2[1] - 1 if r2[1] else 0
    if (np.diff(r2.astype(np.int64)) < 0).any():
        bad(reg_off=r2)
    c2 = codes.copy()
    c2[7] = 5
    bad(codes=c2)                                       # a code above 4
    g2 = regs.copy()
    g2[0]["qe"] = 151
    bad(regs=g2)                                        # a region outside its read
    g3 = regs.copy()
    g3[0]["qb"] = -1
    bad(regs=g3)
    bad(pac=None)                                       # no .pac: none is resident
    bad(opt=c_opt(R.Opt(e_ins=0)))                      # bad scoring
    bad(opt=c_opt(R.Opt(o_del=-1)))
    bad(opt=c_opt(R.Opt(a=0)))
    # and the handle still works
    ok = gpu.matesw(pac, D.L_PAC, codes, offs, regs, reg_off, pes, opt)
    assert ok[0].tobytes() == full[0].tobytes()
    # the resident .pac serves when none is given
    gpu.load_pac(pac, D.L_PAC)
    res = gpu.matesw(None, D.L_PAC, codes, offs, regs, reg_off, pes, opt)
    assert res[0].tobytes() == full[0].tobytes()


CHILD = r"""
import os
import sys
import numpy as np
sys.path[:0] = [%(root)r, %(pkg)r]
import smemgpu
from tests import matesw_data as D, matesw_ref as R
from tests.test_gpu_matesw import c_opt, c_pes
G = D.genome()
gpu = smemgpu.Gpu(smemgpu.Index.build(G), device=%(dev)d)
codes, offs, regs, reg_off = D.build_fr(G).arrays()
args = (D.pack(G), D.L_PAC, codes, offs, regs, reg_off, c_pes(D.PES_FR), c_opt(R.Opt()))
want = gpu.matesw(*args)
os.environ["SMEM_GPU_FAIL"] = sys.argv[1]
try:
    gpu.matesw(*args)
    raise SystemExit("the injected failure did not surface")
except smemgpu.SmemError as e:
    assert "SMEM_E_DEVICE" in str(e) and "injected" in str(e), e
if sys.argv[1].endswith(":sticky"):      # as a runtime failure: the device is marked, whatever the setting now
    os.environ.pop("SMEM_GPU_FAIL")
    assert gpu.fault()[0] != 0
try:
    gpu.matesw(*args)
    raise SystemExit("a call after the failure went through")
except smemgpu.SmemError as e:
    assert "SMEM_E_DEVICE" in str(e), e
print("child ok", int(want[1][-1]))
"""


@pytest.mark.parametrize("setting", ["matesw:1", "matesw:1:sticky"])
def test_injected_failure_in_a_child(gpu_device, setting):
    """SMEM_GPU_FAIL=matesw:1 (the library's own return-code hook, after the work is enqueued) in a
    fresh process: SMEM_E_DEVICE, and the calls after it are refused with SMEM_E_DEVICE too -- with
    :sticky because the device is marked faulted, as after a runtime failure"""
    env = dict(os.environ)
    env.pop("SMEM_GPU_FAIL", None)
    src = CHILD % {"root": ROOT, "pkg": os.path.join(ROOT, "bwa-mem-harp2_amd"), "dev": gpu_device}
    p = subprocess.run([sys.executable, "-c", src, setting], env=env, capture_output=True, timeout=120)
    out = p.stdout.decode(errors="replace") + p.stderr.decode(errors="replace")
    assert p.returncode == 0 and "child ok" in out, out[-3000:]
