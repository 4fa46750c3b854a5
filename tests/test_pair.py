"""mem_pestat, mem_pair and the decision block of mem_sam_pe restated (tests/pair_ref.py).

Pinned to the reference on the paired-end set of tests/golden/msw (g1_pe: the reference's
regions, the bounds mem_pestat printed and its SAM): the restatement must infer the recorded
bounds from the regions, and regions -> sort_and_dedup -> pestat -> mate rescue ->
mem_mark_primary_se -> pair must give both primary lines' FLAG & 2 and MAPQ of every pair.
The hand-built cases of tests/pair_data.py pin what SAM cannot observe against values worked
out by hand and against what each case was built to reach (Trace).  The GPU stages are
compared with the restatement in tests/test_gpu_pair.py.
"""
import functools
import gzip
import math
import os

import pytest

from tests import matesw_ref, pair_chain as PC, pair_data as D, pair_ref as R, regfin_data, regfin_ref
from tests import test_matesw as TM


# ------------------------------------------------------------------ against the reference
@functools.lru_cache(maxsize=None)
def g1_chain():
    """the paired-end set through the restated pipeline: (pes, n_cand, lists after rescue and
    mem_mark_primary_se, sel per pair, Trace per pair, the reference's primary (flag, mapq) per read)"""
    S = TM.load_set()
    codes, offs, regs, reg_off = S["arrays"]
    n = S["man"]["pairs"]
    lists = [[matesw_ref._as_dict(regs[k]) for k in range(int(reg_off[r]), int(reg_off[r + 1]))] for r in range(2 * n)]
    pes, n_cand, ptr = R.pestat(R.Opt(), S["l_pac"], lists)
    after, n_sw, status, _ = matesw_ref.matesw(matesw_ref.Opt(), S["l_pac"], S["G"], pes, codes, offs, regs, reg_off)
    assert not any(status)
    fin = [regfin_ref.mark_primary_se(regfin_ref.Opt(), after[r], (r >> 1) << 1 | (r & 1)) for r in range(2 * n)]
    out = [R.pair(R.Opt(), S["l_pac"], pes, (fin[2 * p], fin[2 * p + 1]), p) for p in range(n)]
    sam = {}
    with gzip.open(os.path.join(TM.MSW, "g1_pe.sam.gz"), "rt") as fh:
        for line in fh:
            f = line.split("\t")
            if line.startswith("@") or int(f[1]) & 0x900:
                continue
            sam[2 * int(f[0][1:]) + (1 if int(f[1]) & 0x80 else 0)] = (int(f[1]), int(f[4]), f[2])
    return pes, n_cand, fin, [x[0] for x in out], [x[1] for x in out], sam, ptr


def test_pestat_infers_the_reference_bounds():
    pes, n_cand, _, _, _, _, ptr = g1_chain()
    want = TM.load_set()["pes"]
    assert [p.failed for p in pes] == [p.failed for p in want] == [1, 0, 1, 1]
    assert (pes[1].low, pes[1].high) == (want[1].low, want[1].high)
    assert n_cand[1] >= 200 and ptr.empty == 60


def test_pairing_gives_the_reference_flags_and_mapq():
    """every pair: FLAG & 2 and MAPQ of both primary lines.  In branch 0 the MAPQ is the single-end
    selection's (regfin_ref.select) and the proper bit is ANDed with both ends lying on one contig."""
    S = TM.load_set()
    pes, _, fin, sels, trs, sam, _ = g1_chain()
    contigs = regfin_data.contigs("g1")
    n1 = n2 = 0
    for p, (sel, tr) in enumerate(zip(sels, trs)):
        assert sel["status"] == 0, (p, tr.host)
        for e in range(2):
            flag, mapq, rname = sam[2 * p + e]
            if sel["branch"] == 0:
                sse, idx = regfin_ref.select(regfin_ref.Opt(), fin[2 * p + e])
                got_q = sse[idx[0]][0] if idx else 0
                same = sam[2 * p][2] == sam[2 * p + 1][2] != "*"
                got_proper = 2 if sel["proper"] and same else 0
            else:
                got_q, got_proper = sel["mapq"][e], sel["proper"]
            assert (flag & 2, mapq) == (got_proper, got_q), (p, e, sel, flag, mapq)
        n1 += sel["branch"] == 1
        n2 += sel["branch"] == 2
    assert n1 >= 250 and len(contigs) >= 1


# ------------------------------------------------------------------ mem_pestat by hand
@functools.lru_cache(maxsize=None)
def pestat_results():
    return {name: R.pestat(opt, D.L_PAC, lists) for name, (lists, opt) in D.pestat_cases().items()}


def test_pestat_ten_by_hand():
    pes, n_cand, tr = pestat_results()["ten_fr"]
    assert n_cand == [0, 10, 0, 0] and tr.few == [0, 2, 3]
    assert tr.idx[1] == (2, 5, 7) and tr.pct[1] == (120, 150, 170) and tr.bounds1[1] == (20, 270)
    # mapping bounds: 120 - 150 = -30 (+ .499, truncated: -29), then the clamp; 170 + 150 = 320
    assert (pes[1].low, pes[1].high, pes[1].failed) == (1, 320, 0) and tr.low2_clamp == [1]
    assert pes[1].avg == 145.0 and pes[1].std == math.sqrt(8250.0 / 10)


def test_pestat_cases_reach_what_they_were_built_for():
    X = pestat_results()
    assert [p.failed for p in X["none"][0]] == [1, 1, 1, 1] and X["none"][1] == [0, 0, 0, 0]
    pes, n_cand, tr = X["nine_and_ten"]
    assert n_cand == [9, 10, 0, 0] and [p.failed for p in pes] == [1, 0, 1, 1]
    assert X["ratio_kept"][1] == [0, 200, 10, 0] and X["ratio_kept"][2].ratio == []         # 10 < 200 * .05 is false
    assert X["ratio_removed"][1] == [0, 220, 10, 0] and X["ratio_removed"][2].ratio == [2]   # 10 < 11
    assert [p.failed for p in X["fr_and_rf"][0]] == [1, 0, 0, 1]
    assert [p.failed for p in X["all_four"][0]] == [0, 0, 0, 0]
    assert X["heavy_tail"][2].low_cap == [1] and X["heavy_tail"][2].low2_clamp == [1]
    assert X["short_inserts"][2].low1_clamp == [1] and X["short_inserts"][0][1].low == 1
    assert X["equal"][0][1].std == 0.0 and (X["equal"][0][1].low, X["equal"][0][1].high) == (333, 333)
    assert X["is_edges"][1] == [0, 11, 0, 0] and X["is_edges"][2].out_of_range == 2           # 0 and 501 out, 500 in
    assert X["max_ins_limit"][1] == [0, 11, 0, 0]
    assert X["empty_end"][2].empty == 3 and X["empty_end"][1] == [0, 10, 0, 0]
    assert X["sub_overlap_50"][1][1] == 10 and X["sub_overlap_50"][2].not_unique == 1
    assert X["sub_overlap_49"][1][1] == 11 and X["sub_overlap_49"][2].sub_found == 0
    assert X["sub_ratio_80"][1][1] == 11 and X["sub_ratio_80"][2].sub_found == 2               # 80 > 80.0 is false
    assert X["sub_ratio_81"][1][1] == 10 and X["sub_ratio_81"][2].not_unique == 1
    assert X["sub_at_1_of_1024"][2].sub_at == [1] and X["sub_at_1023_of_1024"][2].sub_at == [1023]
    assert X["mask_level_03"][1][1] == 11   # 30 >= float(100) * float(0.3) = 30.000001 is false


# ------------------------------------------------------------------ mem_pair by hand
@functools.lru_cache(maxsize=None)
def pair_results(which="pair"):
    cases = D.pair_cases() if which == "pair" else D.long_cases()
    return {cn: (c, [R.pair(c.opt, D.L_PAC, c.pes, (c.lists[2 * p], c.lists[2 * p + 1]), c.ids[p])
                     for p in range(len(c.names))]) for cn, c in cases.items()}


def one(X, case, name):
    c, res = X[case]
    return [res[p] for p in c.of(name)]


def test_pair_basic_by_hand():
    X = pair_results()
    sel, tr = one(X, "basic", "one_one")[0]
    # at the mean the entry is .721 * log(2) = .4998: 200 + .4998 + .499 truncates to 200; score_un = 183
    assert (sel["branch"], sel["z"], sel["o"], sel["subo"], sel["n_sub"], sel["proper"]) == (1, [0, 0], 200, 0, 0, 2)
    assert sel["mapq"] == [60, 60] and tr.pe_clamp60
    for name in ("one_none", "none_one", "none_none"):
        sel, tr = one(X, "basic", name)[0]
        assert (sel["branch"], sel["mapq"], sel["proper"], tr.why0) == (0, [-1, -1], 0, "empty")
    assert one(X, "basic", "same_strand")[0][1].why0 == "none"
    assert [one(X, "basic", "dist_" + n)[0][0]["branch"] for n in ("low_m1", "low", "high", "high_p1")] == [0, 1, 1, 0]
    assert one(X, "basic", "rev_first")[0][0]["o"] == 200
    ties = one(X, "basic", "tie")
    assert all(t.tie and s["o"] == s["subo"] == 190 for s, t in ties)
    assert {tuple(s["z"]) for s, _ in ties} == {(0, 0), (0, 1)}      # the ids reverse the order
    assert [one(X, "basic", n)[0][0]["n_sub"] for n in ("nsub_at_tmp", "nsub_past_tmp")] == [2, 1]
    assert [one(X, "basic", n)[0][0]["branch"] for n in ("o_at_un", "o_at_un_p1", "unpaired_preferred")] == [2, 1, 2]
    assert [one(X, "basic", n)[0][0]["o"] for n in ("o_at_un", "o_at_un_p1")] == [183, 184]
    assert [one(X, "basic", n)[0][1].why0 for n in ("multi_0", "multi_1")] == ["multi", "multi"]
    assert one(X, "basic", "second_below_T")[0][0]["branch"] == 1
    sel, tr = one(X, "basic", "chosen_secondary")[0]
    assert (sel["z"], sel["promoted"], sel["sub"]) == ([0, 1], [0, 1], [0, 100])
    assert one(X, "basic", "q_pe_0")[0][1].pe_clamp0 and one(X, "basic", "q_pe_60")[0][1].pe_clamp60
    assert one(X, "basic", "plus_40_cap")[0][1].cap40 == [0] and one(X, "basic", "plus_40_cap")[0][0]["mapq"] == [40, 60]
    assert one(X, "basic", "csub_cap")[0][1].cap_csub == [0, 1] and one(X, "basic", "csub_cap")[0][0]["mapq"] == [30, 12]
    assert one(X, "basic", "raised_by_q_pe")[0][1].raised == [0]


def test_pair_other_cases():
    X = pair_results()
    assert [one(X, "all_four", f"dir_{d}")[0][0]["branch"] for d in range(4)] == [1, 1, 1, 1]
    assert one(X, "all_four", "every_dir")[0][1].n_cand == 3
    for name in ("std0_at_mean", "std0_off_mean"):   # NaN and -inf: q = 0, mem_pair returns 0
        sel, tr = one(X, "std0", name)[0]
        assert (tr.q_zero, tr.n_cand, sel["o"], tr.why0, sel["proper"]) == (1, 1, 0, "none", 2)
    assert one(X, "minus_inf", "far_tail")[0][1].q_zero == 1 and one(X, "minus_inf", "near")[0][0]["o"] == 200
    sel, tr = one(X, "nopairing", "flag")[0]
    assert (sel["branch"], sel["proper"], tr.why0) == (0, 0, "flag")
    assert one(X, "A2", "one_one")[0][0]["o"] == 401   # 400 + 2 * .4998 + .499


def test_pair_table_limit():
    with pytest.raises(ValueError):
        R.pen_table(R.Opt(), [R.Pes(1, R.PAIR_TAB_LEN + 1, 0, 300.0, 50.0)] * 4)
    assert len(R.pen_table(R.Opt(), [R.Pes(1, R.PAIR_TAB_LEN, 0, 300.0, 50.0)] * 4)[1]) == R.PAIR_TAB_LEN


def test_pair_host_cases():
    c = D.long_cases()["host"]
    res = [R.pair(c.opt, D.L_PAC, c.pes, (c.lists[2 * p], c.lists[2 * p + 1]), c.ids[p]) for p in range(len(c.names))]
    assert [t.host for _, t in res] == ["", "list", "n_sub"]
    assert [s["status"] for s, _ in res] == [0, R.PAIR_HOST, R.PAIR_HOST]


# ------------------------------------------------------------------ tests/golden/pair (make_golden_pair.py)
PESTAT_SETS = ("fr_only", "fr_rf", "ratio", "nine_ten", "heavy", "short", "repeats")
PAIRING_SETS = ("rep", "rep_a2")


@functools.lru_cache(maxsize=None)
def load_pair_set(name):
    return PC.load_set(name)


@pytest.mark.parametrize("name", PESTAT_SETS + PAIRING_SETS)
def test_pestat_gives_what_the_reference_printed(name):
    """candidate counts, percentiles, both pairs of bounds, mean and std.dev as printed (%.2f) and the
    skip lines of either kind, from the reference's own regions"""
    man, _, lists, _ = load_pair_set(name)
    msg = man["pestat"]
    opt = PC.OPTS[man.get("options", "default")]["pair"]
    pes, n_cand, tr = R.pestat(opt, PC.genome(man["genome"])[1], lists)
    assert n_cand == msg["n_cand"] and tr.few == msg["few"] and tr.ratio == msg["ratio"]
    assert sorted(int(d) for d in msg["dirs"]) == [d for d in range(4) if d not in tr.few]
    for d, want in msg["dirs"].items():
        d = int(d)
        assert list(tr.pct[d]) == want["pct"] and list(tr.bounds1[d]) == want["bounds1"]
        assert ["%.2f" % pes[d].avg, "%.2f" % pes[d].std] == want["mean_std"]
        assert [pes[d].low, pes[d].high] == want["bounds"]
    # what each set was built for
    if name == "ratio":
        assert msg["ratio"] == [2] and n_cand[2] >= 10
    if name == "nine_ten":
        assert (n_cand[0], n_cand[2]) == (9, 10) and 0 in tr.few and pes[2].failed == 0
    if name == "heavy":
        assert tr.low_cap == [1]
    if name == "short":
        assert tr.low1_clamp == [1] and tr.low2_clamp == [1]
    if name == "repeats":
        assert tr.not_unique >= 5 and tr.sub_kept >= 3


@functools.lru_cache(maxsize=None)
def pair_set_chain(name):
    """a pairing set through the restated pipeline (pair_chain.run_chain)"""
    man, reads, lists, _ = load_pair_set(name)
    G, l_pac, _, _ = PC.genome(man["genome"])
    return PC.run_chain(G, l_pac, reads, lists, PC.OPTS[man["options"]])


@pytest.mark.parametrize("name", PAIRING_SETS)
def test_pairing_set_gives_the_reference_sam(name):
    """every pair of the set, under its options: FLAG & 2, strand, RNAME / POS, MAPQ and XS of both primary
    lines; a pair the restatement leaves to the host is named and not counted, 2 % of the set at most; and
    the Trace shows at least ten pairs in each group the set was built for"""
    man, reads, _, sam = load_pair_set(name)
    _, l_pac, pac, contigs = PC.genome(man["genome"])
    fin, pes, out, status = pair_set_chain(name)
    checked, left, bad = PC.compare_sam(sam, reads, fin, out, status, PC.OPTS[man["options"]], l_pac, pac, contigs)
    assert not bad, bad[:5]
    assert len(left) <= PC.MAX_HOST_FRACTION * man["pairs"], left
    assert [list(x) for x in left] == man["left_to_host"] and checked == man["pairs"] - len(left)
    c = PC.counts(out, status)
    assert c == man["pairing"]
    for g in PC.GROUPS:
        assert c[g] >= PC.MIN_GROUP, (g, c)
    assert c["tie_by_hash"] >= 1   # wanted too; the manifest states how many there are
