"""Python restatement of what the reference does to a read's raw regions before
mem_reg2aln: mem_sort_and_dedup (software/bwamem.c:705-746),
mem_test_and_remove_exact (:748-753), mem_mark_primary_se (:755-785) and the
selection, MAPQ and flags of mem_reg2sam_se / mem_reg2aln (:1333-1356,
:1367-1379, :1498-1499, :1550).

ks_introsort (software/ksort.h:146-226) is not a stable sort, so it is restated
comparison for comparison over a less-than; the two overlap tests are float
arithmetic (numpy.float32); mapQ_coef_fac is an int (software/bwamem.h:56).
The GPU stage (smem_reg_finalize) is checked against finalize() field by field;
tests/test_regfin.py pins finalize() to the reference's own SAM records.
"""
import math
from dataclasses import dataclass

import numpy as np

F32 = np.float32
MASK64 = (1 << 64) - 1
TAB_LEN = 4096        # SMEM_FIN_TAB_LEN: the stage's log tables cover [0, TAB_LEN)
MAX_REGS = 1024       # SMEM_FIN_MAX_REGS: a read with more raw regions is rejected
FIELDS = ("rb", "re", "qb", "qe", "score", "truesc", "sub", "csub", "sub_n", "w", "seedcov", "secondary", "hash")


@dataclass
class Opt:
    a: int = 1
    b: int = 4
    o_del: int = 6
    e_del: int = 1
    o_ins: int = 6
    e_ins: int = 1
    min_seed_len: int = 19
    T: int = 30
    mask_level: float = 0.50
    mask_level_redun: float = 0.95
    mapQ_coef_len: float = 50.0
    mapQ_coef_fac: int = 3          # (int)log(50), software/bwamem.c:71
    no_exact: bool = False          # MEM_F_NO_EXACT
    all: bool = False               # MEM_F_ALL
    no_multi: bool = False          # MEM_F_NO_MULTI


class Counters:
    """what the sorts met (the fixtures must reach these paths)"""
    def __init__(self):
        self.combsort = 0
        self.partitions = 0


def hash_64(key: int) -> int:
    """software/utils.h:99-110"""
    key &= MASK64
    key = (key + (~(key << 32) & MASK64)) & MASK64
    key ^= key >> 22
    key = (key + (~(key << 13) & MASK64)) & MASK64
    key ^= key >> 8
    key = (key + (key << 3)) & MASK64
    key ^= key >> 15
    key = (key + (~(key << 27) & MASK64)) & MASK64
    key ^= key >> 31
    return key


# ------------------------------------------------------------------ ksort.h
def _insertsort(a, s, t, lt):
    """__ks_insertsort over a[s:t]"""
    for i in range(s + 1, t):
        j = i
        while j > s and lt(a[j], a[j - 1]):
            a[j], a[j - 1] = a[j - 1], a[j]
            j -= 1


def ks_combsort(a, s, n, lt):
    """ks_combsort over a[s:s+n]"""
    shrink = 1.2473309501039786540366528676643
    gap = n
    while True:
        if gap > 2:
            gap = int(gap / shrink)
            if gap in (9, 10):
                gap = 11
        do_swap = False
        for i in range(s, s + n - gap):
            j = i + gap
            if lt(a[j], a[i]):
                a[i], a[j] = a[j], a[i]
                do_swap = True
        if not (do_swap or gap > 2):
            break
    if gap != 1:
        _insertsort(a, s, s + n, lt)


def ks_introsort(a, lt, ctr=None):
    """ks_introsort of the list a, in place"""
    n = len(a)
    if n < 1:
        return
    if n == 2:
        if lt(a[1], a[0]):
            a[0], a[1] = a[1], a[0]
        return
    d = 2
    while (1 << d) < n:
        d += 1
    stack = []
    s, t, d = 0, n - 1, d << 1
    while True:
        if s < t:
            d -= 1
            if d == 0:
                if ctr is not None:
                    ctr.combsort += 1
                ks_combsort(a, s, t - s + 1, lt)
                t = s
                continue
            if ctr is not None:
                ctr.partitions += 1
            i, j = s, t
            k = i + ((j - i) >> 1) + 1
            if lt(a[k], a[i]):
                if lt(a[k], a[j]):
                    k = j
            else:
                k = i if lt(a[j], a[i]) else j
            rp = a[k]
            if k != t:
                a[k], a[t] = a[t], a[k]
            while True:
                i += 1
                while lt(a[i], rp):
                    i += 1
                j -= 1
                while i <= j and lt(rp, a[j]):
                    j -= 1
                if j <= i:
                    break
                a[i], a[j] = a[j], a[i]
            a[i], a[t] = a[t], a[i]
            if i - s > t - i:
                if i - s > 16:
                    stack.append((s, i - 1, d))
                s = i + 1 if t - i > 16 else t
            else:
                if t - i > 16:
                    stack.append((i + 1, t, d))
                t = i - 1 if i - s > 16 else s
        else:
            if not stack:
                _insertsort(a, 0, n, lt)
                return
            s, t, d = stack.pop()


# ------------------------------------------------------------------ bwamem.c
def _slt2(x, y):
    return x["re"] < y["re"]


def _slt(x, y):
    return x["score"] > y["score"] or (x["score"] == y["score"] and
                                       (x["rb"] < y["rb"] or (x["rb"] == y["rb"] and x["qb"] < y["qb"])))


def _hlt(x, y):
    return x["score"] > y["score"] or (x["score"] == y["score"] and x["hash"] < y["hash"])


def sort_and_dedup(a, mask_level_redun, ctr=None):
    """mem_sort_and_dedup; a: list of dicts, changed in place; returns the kept list"""
    n = len(a)
    if n <= 1:
        return a
    mlr = F32(mask_level_redun)
    ks_introsort(a, _slt2, ctr)
    for i in range(1, n):
        p = a[i]
        if p["rb"] >= a[i - 1]["re"]:
            continue
        j = i - 1
        while j >= 0 and p["rb"] < a[j]["re"]:
            q = a[j]
            j -= 1
            if q["qe"] == q["qb"]:
                continue
            or_ = q["re"] - p["rb"]
            oq = q["qe"] - p["qb"] if q["qb"] < p["qb"] else p["qe"] - q["qb"]
            mr = min(q["re"] - q["rb"], p["re"] - p["rb"])
            mq = min(q["qe"] - q["qb"], p["qe"] - p["qb"])
            if F32(or_) > mlr * F32(mr) and F32(oq) > mlr * F32(mq):
                if p["score"] < q["score"]:
                    p["qe"] = p["qb"]
                    break
                q["qe"] = q["qb"]
    a = [x for x in a if x["qe"] > x["qb"]]
    n = len(a)
    ks_introsort(a, _slt, ctr)
    for i in range(1, n):
        if a[i]["score"] == a[i - 1]["score"] and a[i]["rb"] == a[i - 1]["rb"] and a[i]["qb"] == a[i - 1]["qb"]:
            a[i]["qe"] = a[i]["qb"]
    return a[:1] + [x for x in a[1:] if x["qe"] > x["qb"]]


def mark_primary_se(opt, a, id_, ctr=None):
    """mem_mark_primary_se; returns the list in its final order"""
    n = len(a)
    if n == 0:
        return a
    for i in range(n):
        a[i]["sub"], a[i]["secondary"], a[i]["hash"] = 0, -1, hash_64(id_ + i)
    ks_introsort(a, _hlt, ctr)
    tmp = max(opt.a + opt.b, opt.o_del + opt.e_del, opt.o_ins + opt.e_ins)
    ml = F32(opt.mask_level)
    z = [0]
    for i in range(1, n):
        hit = -1
        for j in z:
            b_max = max(a[j]["qb"], a[i]["qb"])
            e_min = min(a[j]["qe"], a[i]["qe"])
            if e_min > b_max:
                min_l = min(a[i]["qe"] - a[i]["qb"], a[j]["qe"] - a[j]["qb"])
                if F32(e_min - b_max) >= F32(min_l) * ml:
                    if a[j]["sub"] == 0:
                        a[j]["sub"] = a[i]["score"]
                    if a[j]["score"] - a[i]["score"] <= tmp:
                        a[j]["sub_n"] += 1
                    hit = j
                    break
        if hit < 0:
            z.append(i)
        else:
            a[i]["secondary"] = hit
    return a


def approx_mapq_se(opt, r, tab_len=TAB_LEN):
    """mem_approx_mapq_se; -1 where the stage's tables end (the caller computes it)"""
    sub = r["sub"] if r["sub"] else opt.min_seed_len * opt.a
    sub = max(r["csub"], sub)
    if sub >= r["score"]:
        return 0
    l = max(r["qe"] - r["qb"], r["re"] - r["rb"])
    if l < 1:
        return -1
    identity = 1. - float(l * opt.a - r["score"]) / (opt.a + opt.b) / l
    if r["score"] == 0:
        mapq = 0
    elif F32(opt.mapQ_coef_len) > 0:
        if F32(l) < F32(opt.mapQ_coef_len):
            tmp = 1.
        else:
            if l < 2 or l >= tab_len:
                return -1
            tmp = opt.mapQ_coef_fac / math.log(l)
        tmp *= identity * identity
        mapq = int(6.02 * (r["score"] - sub) / opt.a * tmp * tmp + .499)
    else:
        if r["seedcov"] < 1 or r["seedcov"] >= tab_len:
            return -1
        mapq = int(30.0 * (1. - float(sub) / r["score"]) * math.log(r["seedcov"]) + .499)
        if identity < 0.95:
            mapq = int(mapq * identity * identity + .499)
    if r["sub_n"] > 0:
        if r["sub_n"] >= tab_len:
            return -1
        mapq -= int(4.343 * math.log(r["sub_n"] + 1) + .499)
    return min(max(mapq, 0), 60)


def select(opt, a, tab_len=TAB_LEN):
    """the loop of mem_reg2sam_se: per region (mapq, flag, xs), flag -1 for a region
    without a record; and the indices of the selected regions in print order"""
    sel, idx = [], []
    first = None
    for k, p in enumerate(a):
        if p["score"] < opt.T or (p["secondary"] >= 0 and not opt.all) or \
                (p["secondary"] >= 0 and p["score"] < a[p["secondary"]]["score"] * .5):
            sel.append((0, -1, 0))
            continue
        flag = 0
        if p["secondary"] >= 0:
            mapq, flag, xs = 0, 0x100, -1
        else:
            mapq, xs = approx_mapq_se(opt, p, tab_len), max(p["sub"], p["csub"])
            if k:
                flag |= 0x10000 if opt.no_multi else 0x800
        if first is None:
            first = mapq
        elif mapq > first:
            mapq = first
        sel.append((mapq, flag, xs))
        idx.append(k)
    return sel, idx


def finalize(opt, regs, l_query, id_, ctr=None, tab_len=TAB_LEN):
    """one read: regs (a structured array or a list of records with FIELDS) ->
    (final list of dicts, sel, sel_idx)"""
    a = [{f: int(r[f]) for f in FIELDS} for r in regs]
    a = sort_and_dedup(a, opt.mask_level_redun, ctr)
    if opt.no_exact and a and a[0]["truesc"] == l_query * opt.a:
        a = a[1:]
    a = mark_primary_se(opt, a, id_, ctr)
    sel, idx = select(opt, a, tab_len)
    return a, sel, idx
