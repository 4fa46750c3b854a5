"""smem_pestat and smem_pair on the GPU against tests/pair_ref.py (the restatement of
software/bwamem_pair.c:32-107, 177-236, 264-304, 321-326 that tests/test_pair.py pins to the
reference's SAM and to values worked out by hand): pes -- avg and std as bit patterns -- and
n_cand equal, every field of every pair's smem_pair_sel_t equal, on the hand-built cases of
tests/pair_data.py, on the paired-end set of tests/golden/msw, at the limits of either stage, on
batches longer than one pass of the grid, and byte-identical on a second run."""
import functools
import struct
import time

import numpy as np
import pytest

from tests import pair_data as D
from tests import pair_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(gpu_device):
    import smemgpu
    rng = np.random.default_rng(7)
    g = smemgpu.Gpu(smemgpu.Index.build(rng.integers(0, 4, size=4096).astype(np.uint8)), device=gpu_device)
    yield g
    g.close()


def bits(x):
    return struct.pack("<d", float(x))


def c_pestat_opt(o):
    from smemgpu.lib import pestat_opt
    return pestat_opt(a=o.a, min_seed_len=o.min_seed_len, max_ins=o.max_ins, mask_level=o.mask_level)


def c_pair_opt(o):
    from smemgpu.lib import pair_opt
    return pair_opt(a=o.a, b=o.b, o_del=o.o_del, e_del=o.e_del, o_ins=o.o_ins, e_ins=o.e_ins, pen_unpaired=o.pen_unpaired,
                    T=o.T, min_seed_len=o.min_seed_len, mapQ_coef_len=o.mapQ_coef_len, mapQ_coef_fac=o.mapQ_coef_fac,
                    nopairing=o.nopairing)


def same_pes(got, n_got, want, n_want, what):
    want = R.zeroed(want)   # smem_pestat: a failed orientation is all zeros apart from failed
    assert [int(x) for x in n_got] == list(n_want), (what, n_got, n_want)
    for d in range(4):
        g = got[d]
        assert (int(g["low"]), int(g["high"]), int(g["failed"])) == (want[d].low, want[d].high, want[d].failed), (what, d, g, want[d])
        assert bits(g["avg"]) == bits(want[d].avg) and bits(g["std"]) == bits(want[d].std), (what, d, g, want[d])


def same_sel(got, want, what):
    for f in ("status", "branch", "proper", "o", "subo", "n_sub"):
        assert int(got[f]) == want[f], (what, f, got, want)
    for f in ("z", "mapq", "sub", "promoted"):
        assert [int(x) for x in got[f]] == list(want[f]), (what, f, got, want)


# ------------------------------------------------------------------ smem_pestat
@pytest.mark.parametrize("name", sorted(D.pestat_cases()))
def test_pestat_hand_cases(gpu, name):
    lists, opt = D.pestat_cases()[name]
    want, n_want, _ = R.pestat(opt, D.L_PAC, lists)
    regs, reg_off = D.arrays(lists)
    pes, n_cand, ms = gpu.pestat(regs, reg_off, D.L_PAC, c_pestat_opt(opt))
    same_pes(pes, n_cand, want, n_want, name)
    again = gpu.pestat(regs, reg_off, D.L_PAC, c_pestat_opt(opt))
    assert again[0].tobytes() == pes.tobytes() and again[1].tobytes() == n_cand.tobytes()


def test_pestat_argument_limits(gpu):
    import smemgpu
    from smemgpu.lib import pestat_opt
    regs, reg_off = D.arrays(D.sized(1, D.TEN))
    gpu.pestat(regs, reg_off, D.L_PAC, pestat_opt(max_ins=65535))
    for bad in (65536, 0):
        with pytest.raises(smemgpu.SmemError, match="SMEM_E_ARG"):
            gpu.pestat(regs, reg_off, D.L_PAC, pestat_opt(max_ins=bad))
    down = reg_off.copy()
    down[3] = down[2] - 1
    with pytest.raises(smemgpu.SmemError, match="SMEM_E_ARG"):
        gpu.pestat(regs, down, D.L_PAC)


def test_pestat_golden_set(gpu):
    """the reference's regions of tests/golden/msw: the bounds its mem_pestat printed"""
    from tests import test_matesw as TM
    from tests import test_pair as TP
    S = TM.load_set()
    _, _, regs, reg_off = S["arrays"]
    pes, n_cand, _ = gpu.pestat(regs, reg_off, S["l_pac"])
    want, n_want = TP.g1_chain()[:2]
    same_pes(pes, n_cand, want, n_want, "g1_pe")
    assert (int(pes[1]["low"]), int(pes[1]["high"])) == (S["pes"][1].low, S["pes"][1].high)


def test_pestat_more_pairs_than_the_grid(gpu):
    """3 passes of the grid + 17 pairs of one region an end; one bin takes most of the counts"""
    from smemgpu.lib import ALNREG_DT, PESTAT_WAVES_PER_CU
    n = 3 * gpu.cu_count() * PESTAT_WAVES_PER_CU * 64 + 17
    k = np.arange(n, dtype=np.int64)
    is_ = np.where(k % 10 < 8, 300, 200 + (k * 7919) % 250)
    d = np.where(k % 50 == 0, 2, 1)
    p = 50_000 + (k * 13) % 60_000
    rb1 = 2 * D.L_PAC - 1 - np.where(d == 1, p + is_, p - is_)
    regs = np.zeros(2 * n, dtype=ALNREG_DT)
    regs["rb"][0::2], regs["rb"][1::2] = p, rb1
    regs["re"] = regs["rb"] + 100
    regs["qe"], regs["score"], regs["secondary"] = 100, 100, -1
    reg_off = np.arange(2 * n + 1, dtype=np.uint64)
    isize = [[], [], [], []]
    isize[1] = is_[d == 1].tolist()
    isize[2] = is_[d == 2].tolist()
    # (a list of one region: cal_sub is min_seed_len * a = 19 <= 80, and mem_infer_dir gives (d, is) by place())
    for j in (0, 1, n - 1):
        lists = [[{"rb": int(regs["rb"][2 * j])}], [{"rb": int(regs["rb"][2 * j + 1])}]]
        assert R.infer_dir(D.L_PAC, lists[0][0]["rb"], lists[1][0]["rb"]) == (int(d[j]), int(is_[j]))
    want, n_want = R.pestat_finish(isize)
    pes, n_cand, ms = gpu.pestat(regs, reg_off, D.L_PAC)
    same_pes(pes, n_cand, want, n_want, "grid")
    assert gpu.pestat(regs, reg_off, D.L_PAC)[0].tobytes() == pes.tobytes()


# ------------------------------------------------------------------ smem_pair
def run_pair(gpu, c):
    regs, reg_off = D.arrays(c.lists)
    return gpu.pair(regs, reg_off, D.L_PAC, c.pes, c_pair_opt(c.opt), ids=np.array(c.ids, dtype=np.int64))


@pytest.mark.parametrize("name", sorted(D.pair_cases()))
def test_pair_hand_cases(gpu, name):
    from tests import test_pair as TP
    c, want = TP.pair_results()[name]
    sel, ms = run_pair(gpu, c)
    for p, (w, _) in enumerate(want):
        same_sel(sel[p], w, (name, c.names[p]))
    assert run_pair(gpu, c)[0].tobytes() == sel.tobytes()


def test_pair_ids_default_to_id0_plus_p(gpu):
    c = D.pair_cases()["basic"]
    regs, reg_off = D.arrays(c.lists)
    sel, _ = gpu.pair(regs, reg_off, D.L_PAC, c.pes, id0=1000)
    for p in range(len(c.names)):
        same_sel(sel[p], R.pair(c.opt, D.L_PAC, c.pes, (c.lists[2 * p], c.lists[2 * p + 1]), 1000 + p)[0], c.names[p])


def test_pair_table_limit(gpu):
    import smemgpu
    c = D.pair_cases()["basic"]
    regs, reg_off = D.arrays(c.lists)
    gpu.pair(regs, reg_off, D.L_PAC, [(1, R.PAIR_TAB_LEN, 0, 300.0, 50.0)] * 4)
    with pytest.raises(smemgpu.SmemError, match="SMEM_E_ARG"):
        gpu.pair(regs, reg_off, D.L_PAC, [(1, R.PAIR_TAB_LEN + 1, 0, 300.0, 50.0)] * 4)
    gpu.pair(regs, reg_off, D.L_PAC, [(1, R.PAIR_TAB_LEN + 1, 1, 300.0, 50.0)] * 4)   # failed: no table


@functools.lru_cache(maxsize=None)
def window_want():
    c = D.long_cases()["window_1024"]
    return c, R.pair(c.opt, D.L_PAC, c.pes, (c.lists[0], c.lists[1]), c.ids[0])


def test_pair_quadratic_window(gpu):
    """1024 + 1024 regions inside one window: 2^20 candidates, none of them stored"""
    c, (want, tr) = window_want()
    assert tr.n_cand == 1024 * 1024
    sel, ms = run_pair(gpu, c)
    same_sel(sel[0], want, "window")
    t = time.perf_counter()
    again, ms = run_pair(gpu, c)
    assert again.tobytes() == sel.tobytes()
    assert ms < 500.0 and time.perf_counter() - t < 1.0, ms


def test_pair_host_cases(gpu):
    c = D.long_cases()["host"]
    sel, _ = run_pair(gpu, c)
    for p in range(len(c.names)):
        want, tr = R.pair(c.opt, D.L_PAC, c.pes, (c.lists[2 * p], c.lists[2 * p + 1]), c.ids[p])
        same_sel(sel[p], want, c.names[p])
    assert [int(x) for x in sel["status"]] == [0, R.PAIR_HOST, R.PAIR_HOST]


def test_pair_golden_set(gpu):
    """the paired-end set of tests/golden/msw after the restated rescue and mem_mark_primary_se"""
    from tests import test_matesw as TM
    from tests import test_pair as TP
    pes, _, fin, sels, _, _, _ = TP.g1_chain()
    regs, reg_off = D.arrays(fin)
    sel, _ = gpu.pair(regs, reg_off, TM.load_set()["l_pac"], pes)
    for p, w in enumerate(sels):
        same_sel(sel[p], w, ("g1_pe", p))


def test_pair_mixed_batch_crosses_both_kernels(gpu):
    """short and long pairs with a period of 7, more long pairs than the wave kernel's grid and more
    short ones than a block: compared pair by pair, and run twice"""
    from smemgpu.lib import PAIR_WAVES_PER_CU
    n = 7 * (gpu.cu_count() * PAIR_WAVES_PER_CU + 3) + 5
    c = D.mixed_batch(n)
    assert c.names.count("long") > gpu.cu_count() * PAIR_WAVES_PER_CU and c.names.count("one_one") > 64
    sel, _ = run_pair(gpu, c)
    memo = {}
    for p in range(n):
        key = c.names[p] if c.names[p] == "empty" else None
        want = memo.get(key) if key else None
        if want is None:
            want = R.pair(c.opt, D.L_PAC, c.pes, (c.lists[2 * p], c.lists[2 * p + 1]), c.ids[p])[0]
            if key:
                memo[key] = want
        same_sel(sel[p], want, (p, c.names[p]))
    assert run_pair(gpu, c)[0].tobytes() == sel.tobytes()


# ------------------------------------------------------------------ tests/golden/pair
@pytest.mark.parametrize("name", ["fr_only", "fr_rf", "ratio", "nine_ten", "heavy", "short", "repeats", "rep", "rep_a2"])
def test_pestat_reference_sets(gpu, name):
    """the reference's regions of each set: what its mem_pestat printed (tests/test_pair.py pins the
    restatement to the messages; here the bounds are compared with them directly as well)"""
    from tests import pair_chain as PC
    from tests import test_pair as TP
    man, _, lists, _ = TP.load_pair_set(name)
    l_pac = PC.genome(man["genome"])[1]
    opt = PC.OPTS[man.get("options", "default")]["pair"]
    want, n_want, _ = R.pestat(opt, l_pac, lists)
    regs, reg_off = D.arrays(lists)
    pes, n_cand, _ = gpu.pestat(regs, reg_off, l_pac, c_pestat_opt(opt))
    same_pes(pes, n_cand, want, n_want, name)
    msg = man["pestat"]
    assert [int(x) for x in n_cand] == msg["n_cand"]
    for d in range(4):
        alive = str(d) in msg["dirs"] and d not in msg["ratio"]
        assert int(pes[d]["failed"]) == (0 if alive else 1)
        if alive:
            assert [int(pes[d]["low"]), int(pes[d]["high"])] == msg["dirs"][str(d)]["bounds"]
            assert ["%.2f" % pes[d]["avg"], "%.2f" % pes[d]["std"]] == msg["dirs"][str(d)]["mean_std"]


@pytest.mark.parametrize("name", ["rep", "rep_a2"])
def test_pair_reference_sets(gpu, name):
    """the pairing sets (default options and -A 2) after the restated rescue and mem_mark_primary_se:
    the decision that tests/test_pair.py shows to give the reference's SAM lines"""
    from tests import pair_chain as PC
    from tests import test_pair as TP
    man = TP.load_pair_set(name)[0]
    fin, pes, out, _ = TP.pair_set_chain(name)
    regs, reg_off = D.arrays(fin)
    sel, _ = gpu.pair(regs, reg_off, PC.genome(man["genome"])[1], pes, c_pair_opt(PC.OPTS[man["options"]]["pair"]))
    for p, (w, _) in enumerate(out):
        same_sel(sel[p], w, (name, p))
