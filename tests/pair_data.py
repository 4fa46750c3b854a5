"""The hand-built pairs of the insert-size and pairing tests: one case per branch of cal_sub /
mem_pestat (software/bwamem_pair.c:32-107) and of mem_pair and the decision block of mem_sam_pe
(:177-236, :264-304, :321-326).  Regions are written by hand, so a case controls exactly which
end has which regions; SAM cannot observe most of what these cases pin, so they are checked
against the restatement (tests/pair_ref.py) only.

Orientations (mem_infer_dir, :23-30) for a first region on the forward strand at p, see place():
0 FF, 1 FR, 2 RF, 3 RR.
"""
import numpy as np

from tests import pair_ref as R, regfin_ref
from tests.matesw_ref import Pes

L_PAC = 200_000


def region(rb, L=100, score=None, qb=0, qe=None, **kw):
    r = {k: 0 for k in regfin_ref.FIELDS}
    qe = qb + L if qe is None else qe
    score = L if score is None else score
    r.update(rb=int(rb), re=int(rb) + L, qb=int(qb), qe=int(qe), score=int(score), truesc=int(score), w=100,
             seedcov=int(qe - qb), secondary=-1)
    r.update(kw)
    return r


def place(p, d, is_):
    """rb of the second end's region so that mem_infer_dir(p, rb) = (d, is_), for p on the forward strand"""
    if d == 0:
        return p + is_
    if d == 3:
        return p - is_
    return 2 * L_PAC - 1 - (p + is_ if d == 1 else p - is_)


def arrays(lists):
    """(regs as ALNREG_DT, reg_off) of a list of lists of regions"""
    from smemgpu.lib import ALNREG_DT
    reg_off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint64)
    regs = np.zeros(int(reg_off[-1]), dtype=ALNREG_DT)
    k = 0
    for lst in lists:
        for r in lst:
            for f in regfin_ref.FIELDS:
                regs[k][f] = r[f]
            k += 1
    return regs, reg_off


# ------------------------------------------------------------------ mem_pestat
def sized(d, sizes, p0=50_000):
    """one pair of single full-length regions per insert size, in orientation d"""
    out = []
    for k, is_ in enumerate(sizes):
        p = p0 + 7 * k
        out += [[region(p)], [region(place(p, d, is_))]]
    return out


TEN = [100 + 10 * k for k in range(10)]   # by hand: indices 2, 5, 7 -> 120, 150, 170; bounds (20, 270), then (1, 320)
HEAVY = [110] * 24 + [300 + 2 * k for k in range(52)] + [590] * 24   # line 94's cap acts, then the clamp


def overlap_pair(p, qb2, score2, at=1, n=2):
    """both ends: a first region on [0, 100) of the read, n - 2 regions on [100, 200) that do not
    overlap it, and at position `at` one on [qb2, qb2 + 100) of score score2"""
    def one(rb):
        lst = [region(rb)] + [region(rb + 1000 + 3 * k, qb=100, score=60) for k in range(n - 1)]
        lst[at] = region(rb + 500, qb=qb2, score=score2)
        return lst
    return [one(p), one(place(p, 1, 300))]


def pestat_cases():
    """name -> (lists, Opt): what each is for is asserted in tests/test_pair.py"""
    fr300 = lambda n, p0=50_000: sized(1, [250 + (k * 37) % 100 for k in range(n)], p0)   # noqa: E731
    C = {}
    C["none"] = ([], R.Opt())
    C["ten_fr"] = (sized(1, TEN), R.Opt())
    C["nine_and_ten"] = (sized(0, TEN[:9]) + sized(1, TEN), R.Opt())
    C["ratio_kept"] = (fr300(200) + sized(2, TEN, 90_000), R.Opt())
    C["ratio_removed"] = (fr300(220) + sized(2, TEN, 90_000), R.Opt())
    C["fr_and_rf"] = (fr300(40) + sized(2, [400 + 3 * k for k in range(30)], 90_000), R.Opt())
    C["all_four"] = (sum((sized(d, [200 + 50 * d + k for k in range(12)], 40_000 + 20_000 * d) for d in range(4)), []),
                     R.Opt())
    C["heavy_tail"] = (sized(1, HEAVY), R.Opt())
    C["short_inserts"] = (sized(1, [3 + k % 5 for k in range(20)]), R.Opt())
    C["equal"] = (sized(1, [333] * 15), R.Opt())
    # is of 0 (FF onto itself), max_ins and max_ins + 1 beside ten ordinary pairs
    C["is_edges"] = (sized(1, TEN) + sized(0, [0]) + sized(1, [500, 501], 120_000), R.Opt(max_ins=500))
    C["max_ins_limit"] = (sized(1, TEN + [65535]), R.Opt(max_ins=65535))
    C["empty_end"] = (sized(1, TEN) + [[region(1000)], [], [], [region(2000)], [], []], R.Opt())
    # cal_sub: an overlap of exactly min_l * mask_level = 50 bases and of 49; a sub of exactly 0.8 * score and one above
    C["sub_overlap_50"] = (sized(1, TEN) + overlap_pair(120_000, 50, 90), R.Opt())
    C["sub_overlap_49"] = (sized(1, TEN) + overlap_pair(120_000, 51, 90), R.Opt())
    C["sub_ratio_80"] = (sized(1, TEN) + overlap_pair(120_000, 50, 80), R.Opt())
    C["sub_ratio_81"] = (sized(1, TEN) + overlap_pair(120_000, 50, 81), R.Opt())
    C["sub_at_1_of_1024"] = (sized(1, TEN) + overlap_pair(120_000, 50, 90, at=1, n=1024), R.Opt())
    C["sub_at_1023_of_1024"] = (sized(1, TEN) + overlap_pair(120_000, 50, 90, at=1023, n=1024), R.Opt())
    C["mask_level_03"] = (sized(1, TEN) + overlap_pair(120_000, 70, 90), R.Opt(mask_level=0.3))
    return C


# ------------------------------------------------------------------ mem_pair
AVG, STD = 300.0, 50.0
PES_FR = [Pes(0, 0, 1), Pes(100, 500, 0, AVG, STD), Pes(0, 0, 1), Pes(0, 0, 1)]
PES_ALL = [Pes(100, 500, 0, AVG, STD) for _ in range(4)]
PES_STD0 = [Pes(0, 0, 1), Pes(100, 500, 0, AVG, 0.0), Pes(0, 0, 1), Pes(0, 0, 1)]
PES_WIDE = [Pes(0, 0, 1), Pes(1, 60000, 0, AVG, STD), Pes(0, 0, 1), Pes(0, 0, 1)]   # entries of -inf far out


def marked(lst, id_, opt=None):
    """the list as mem_mark_primary_se(opt, ..., id_) leaves it"""
    return regfin_ref.mark_primary_se(opt or regfin_ref.Opt(), [dict(x) for x in lst], id_)


class Case:
    def __init__(self, pes=None, opt=None):
        self.pes, self.opt = pes or PES_FR, opt or R.Opt()
        self.lists, self.ids, self.names = [], [], []

    def add(self, name, l0, l1, id_=None, mark=True):
        id_ = len(self.names) if id_ is None else id_
        self.lists += [marked(l0, id_ << 1 | 0) if mark else l0, marked(l1, id_ << 1 | 1) if mark else l1]
        self.ids.append(id_)
        self.names.append(name)

    def of(self, name):
        return [p for p, n in enumerate(self.names) if n == name]


def fr(p, is_, **kw):
    return region(place(p, 1, is_), **kw)


def window_lists(n, p0=60_000):
    """n regions an end, all inside one window: every region of end 1 pairs with every one of end 0 before it"""
    l0 = [region(p0 + k // 8, score=40 + k % 50, qb=k % 7) for k in range(n)]
    l1 = [fr(p0 + 150, 100 + k // 8, score=40 + (k * 7) % 50, qb=k % 5) for k in range(n)]
    return l0, l1


def pair_cases():
    """name -> Case"""
    C = {}
    c = C["basic"] = Case()
    p = 50_000
    c.add("one_one", [region(p)], [fr(p, 300)])
    c.add("one_none", [region(p)], [])
    c.add("none_one", [], [region(p)])
    c.add("none_none", [], [])
    c.add("same_strand", [region(p)], [region(p + 300)])                   # FF: failed here, no candidate
    for name, is_ in (("low_m1", 99), ("low", 100), ("high", 500), ("high_p1", 501)):
        c.add("dist_" + name, [region(p)], [fr(p, is_)])
    # end 0 on the reverse strand: its forward position is 2 l_pac - 1 - rb
    c.add("rev_first", [region(2 * L_PAC - 1 - (p + 300))], [region(p)])
    # two placements of end 1 an equal distance either side of the mean: equal q, the hash decides
    for id_ in range(6):
        c.add("tie", [region(p)], [fr(p, 280, score=90), fr(p, 320, score=90, qb=20)], id_=1000 + id_)
    c.add("tie_big_id", [region(p)], [fr(p, 280, score=90), fr(p, 320, score=90, qb=20)], id_=(1 << 23) + 5)
    # three candidates of q 200, 195 and 188 / 187: sub = 195, and sub - q at tmp = 7 (counted) and at tmp + 1 (not)
    c.add("nsub_at_tmp", [region(p)], [fr(p, 300), fr(p, 310, score=95, qb=30), fr(p, 320, score=88, qb=31)])
    c.add("nsub_past_tmp", [region(p)], [fr(p, 300), fr(p, 310, score=95, qb=30), fr(p, 320, score=87, qb=31)])
    # o against score_un = 100 + 100 - 17 = 183: the two best ends lie 50 kbp apart, and the pair that exists is
    # end 1's best with a secondary region of end 0 (at the mean the table's entry adds nothing: o = 83 + 100)
    c.add("o_at_un", [region(p), region(p + 50_000, score=83, qb=2)], [fr(p + 50_000, 300)])
    c.add("o_at_un_p1", [region(p), region(p + 50_000, score=84, qb=2)], [fr(p + 50_000, 300)])
    c.add("unpaired_preferred", [region(p), region(p + 50_000, score=70, qb=2)], [fr(p + 50_000, 300)])
    # is_multi from either end; a second region below T that does not count
    c.add("multi_0", [region(p), region(p + 9000, qb=120, score=60)], [fr(p, 300)])
    c.add("multi_1", [region(p)], [fr(p, 300), fr(p + 9000, 300, qb=120, score=60)])
    c.add("second_below_T", [region(p), region(p + 9000, qb=120, score=29)], [fr(p, 300)])
    # the chosen region of end 1 is secondary: the best single-end hit lies far away, the pair takes the other
    c.add("chosen_secondary", [region(p)], [fr(p + 30_000, 300, score=100), fr(p, 300, score=95, qb=2)])
    # q_pe at 0 (a second pair as good), at 60; q_se + 40 capping it; the csub cap
    c.add("q_pe_0", [region(p)], [fr(p, 300, score=100), fr(p, 300, score=100, qb=40)])
    c.add("q_pe_60", [region(p, L=150)], [fr(p, 300, L=150)])
    c.add("plus_40_cap", [region(p, L=150), region(p + 40_000, L=150, score=149, qb=1)], [fr(p, 300, L=150)])
    c.add("csub_cap", [region(p, csub=95)], [fr(p, 300, csub=98)])
    c.add("raised_by_q_pe", [region(p, L=150), region(p + 40_000, L=150, score=140, qb=2)], [fr(p, 300, L=150)])
    c = C["all_four"] = Case(PES_ALL)
    for d in range(4):
        c.add(f"dir_{d}", [region(p)], [region(place(p, d, 250 + 10 * d))])
    c.add("every_dir", [region(p), region(2 * L_PAC - 1 - (p + 900), qb=120, score=50)],
          [region(p + 280, score=80), fr(p, 310, score=85, qb=3), region(p - 330, score=70, qb=5)])
    c = C["std0"] = Case(PES_STD0)
    c.add("std0_at_mean", [region(p)], [fr(p, 300)])
    c.add("std0_off_mean", [region(p)], [fr(p, 301)])
    c = C["minus_inf"] = Case(PES_WIDE)
    c.add("far_tail", [region(p)], [fr(p, 59_000)])
    c.add("near", [region(p)], [fr(p, 320)])
    c = C["nopairing"] = Case(opt=R.Opt(nopairing=True))
    c.add("flag", [region(p)], [fr(p, 300)])
    c = C["A2"] = Case(opt=R.Opt(a=2, b=8, o_del=12, e_del=2, o_ins=12, e_ins=2, pen_unpaired=34, T=60))
    c.add("one_one", [region(p, score=200)], [fr(p, 300, score=200)])
    c.add("two", [region(p, score=200)], [fr(p, 300, score=200), fr(p, 330, score=190, qb=9)])
    return C


def long_cases():
    """the quadratic case, the host cases and n_sub past the table"""
    C = {}
    c = C["window_1024"] = Case()
    l0, l1 = window_lists(1024)
    c.add("window", l0, l1, mark=False)
    c = C["host"] = Case()
    c.add("short", [region(50_000)], [fr(50_000, 300)])
    c.add("list_1025", [region(50_000 + k) for k in range(1025)], [fr(50_000, 300)], mark=False)
    # 80 x 80 candidates of equal score: n_sub = 6399 >= the table's 4096; no second primary region
    l0 = [region(60_000 + k, secondary=0 if k else -1) for k in range(80)]
    l1 = [fr(60_000 + 100, 200 + k, secondary=0 if k else -1) for k in range(80)]
    c.add("n_sub_past_table", l0, l1, mark=False)
    return C


def mixed_batch(n_pairs, period=7):
    """short and long pairs with a period coprime to any power-of-two grid"""
    c = Case()
    l0, l1 = window_lists(12)
    for k in range(n_pairs):
        p = 30_000 + 11 * k
        if k % period == 3:
            c.add("long", [dict(x, rb=x["rb"] + k, re=x["re"] + k) for x in l0],
                  [dict(x, rb=x["rb"] - k, re=x["re"] - k) for x in l1], mark=False)
        elif k % period == 5:
            c.add("nine", [region(p), region(p + 50, score=70, qb=3)], [fr(p, 250 + j * 9, score=60 + j, qb=j) for j in range(7)])
        elif k % 11 == 0:
            c.add("empty", [region(p)], [])
        else:
            c.add("one_one", [region(p)], [fr(p, 150 + (k * 13) % 300)])
    return c
