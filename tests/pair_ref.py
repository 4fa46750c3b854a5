"""Python restatement of the two steps of mem_sam_pe around mate rescue: cal_sub and
mem_pestat (software/bwamem_pair.c:32-107), mem_pair (:177-236) and the decision block
(:264-304, :321-326).

The GPU stages (smem_pestat, smem_pair) are checked against pestat() and pair() field by
field, avg and std as bit patterns.  Arithmetic that decides parity is written as the
reference compiles it: cal_sub's overlap test is a float product (numpy.float32), every other
product and sum is a double in the reference's order, the sum of squares is accumulated value
by value in sorted order, log / erfc / sqrt are the host's libm (math.*), and a cast of a
double that is not finite or below zero gives what x86 gives (INT_MIN) before the clamp.

Regions are dicts of regfin_ref.FIELDS.  What smem_pair leaves to the host (SMEM_PAIR_HOST) is
decided here the same way and named in Trace.host: "list" (an end of more than MAX_REGS
regions), "n_sub" (n_sub past the finalize stage's table where line 282 reads it), "mapq" (an
argument of mem_approx_mapq_se outside the tables).
"""
import math
from dataclasses import dataclass, field

import numpy as np

from tests import regfin_ref
from tests.matesw_ref import Pes, infer_dir
from tests.regfin_ref import F32, MASK64, approx_mapq_se, hash_64

MAX_REGS = regfin_ref.MAX_REGS    # SMEM_FIN_MAX_REGS
TAB_LEN = regfin_ref.TAB_LEN      # SMEM_FIN_TAB_LEN
PESTAT_MAX_INS = 65535            # SMEM_PESTAT_MAX_INS
PAIR_TAB_LEN = 65536              # SMEM_PAIR_TAB_LEN
PAIR_HOST = 1                     # SMEM_PAIR_HOST
MIN_RATIO, MIN_DIR_CNT, MIN_DIR_RATIO = 0.8, 10, 0.05
OUTLIER_BOUND, MAPPING_BOUND, MAX_STDDEV = 2.0, 3.0, 4.0
INT_MIN = -(1 << 31)


@dataclass
class Opt:
    a: int = 1
    b: int = 4
    o_del: int = 6
    e_del: int = 1
    o_ins: int = 6
    e_ins: int = 1
    pen_unpaired: int = 17
    T: int = 30
    min_seed_len: int = 19
    max_ins: int = 10000
    mask_level: float = 0.50
    mapQ_coef_len: float = 50.0
    mapQ_coef_fac: int = 3
    nopairing: bool = False         # MEM_F_NOPAIRING


class ToHost(Exception):
    pass


def c_int(x: float) -> int:
    """(int)x as x86 compiles it: cvttsd2si gives INT_MIN for NaN and for anything out of range"""
    if x != x or x >= 2147483648.0 or x <= -2147483649.0:
        return INT_MIN
    return int(x)


# ------------------------------------------------------------------ mem_pestat
@dataclass
class PestatTrace:
    """what mem_pestat met (the fixtures assert their cases by these)"""
    empty: int = 0          # pairs with an empty end (:58)
    not_unique: int = 0     # pairs cal_sub turned away (:59-60)
    out_of_range: int = 0   # is == 0 or is > max_ins (:62)
    sub_found: int = 0      # cal_sub calls that found a significant overlap
    sub_kept: int = 0       # of them, those whose score stayed within MIN_RATIO of the first region's
    sub_at: list = field(default_factory=list)   # the positions they found it at
    few: list = field(default_factory=list)      # orientations under MIN_DIR_CNT (:69)
    ratio: list = field(default_factory=list)    # orientations the 5 % rule removed (:103)
    low1_clamp: list = field(default_factory=list)   # low < 1 at :79
    low2_clamp: list = field(default_factory=list)   # low < 1 at :96
    low_cap: list = field(default_factory=list)      # :94 acted
    high_cap: list = field(default_factory=list)     # :95 acted
    pct: dict = field(default_factory=dict)      # d -> (p25, p50, p75)
    bounds1: dict = field(default_factory=dict)  # d -> (low, high) for mean and std.dev (:78-80)
    idx: dict = field(default_factory=dict)      # d -> the three percentile indices


def cal_sub(opt, a, tr=None):
    """cal_sub (:32-44)"""
    ml = F32(opt.mask_level)
    for j in range(1, len(a)):
        b_max = max(a[j]["qb"], a[0]["qb"])
        e_min = min(a[j]["qe"], a[0]["qe"])
        if e_min > b_max:
            min_l = min(a[j]["qe"] - a[j]["qb"], a[0]["qe"] - a[0]["qb"])
            if F32(e_min - b_max) >= F32(min_l) * ml:
                if tr is not None:
                    tr.sub_found += 1
                    tr.sub_at.append(j)
                return a[j]["score"]
    return opt.min_seed_len * opt.a


def pestat_collect(opt, l_pac, lists, tr=None):
    """:52-63: the insert sizes per orientation, in pair order; lists[2p], lists[2p + 1] are pair p"""
    tr = tr if tr is not None else PestatTrace()
    isize = [[], [], [], []]
    for p in range(len(lists) // 2):
        r = (lists[2 * p], lists[2 * p + 1])
        if not r[0] or not r[1]:
            tr.empty += 1
            continue
        unique = True
        for e in range(2):
            before = tr.sub_found
            if float(cal_sub(opt, r[e], tr)) > MIN_RATIO * r[e][0]["score"]:
                unique = False
                break
            tr.sub_kept += tr.sub_found - before
        if not unique:
            tr.not_unique += 1
            continue
        d, is_ = infer_dir(l_pac, r[0][0]["rb"], r[1][0]["rb"])
        if is_ and is_ <= opt.max_ins:
            isize[d].append(is_)
        else:
            tr.out_of_range += 1
    return isize


def pestat_finish(isize, tr=None):
    """:64-106 over the four lists of insert sizes: (pes[4], n_cand[4])"""
    tr = tr if tr is not None else PestatTrace()
    pes = [Pes(0, 0, 0, 0.0, 0.0) for _ in range(4)]
    for d in range(4):
        q = sorted(isize[d])
        n = len(q)
        r = pes[d]
        if n < MIN_DIR_CNT:
            r.failed = 1
            tr.few.append(d)
            continue
        idx = (int(.25 * n + .499), int(.50 * n + .499), int(.75 * n + .499))
        p25, p50, p75 = q[idx[0]], q[idx[1]], q[idx[2]]
        tr.idx[d], tr.pct[d] = idx, (p25, p50, p75)
        r.low = c_int(p25 - OUTLIER_BOUND * (p75 - p25) + .499)
        if r.low < 1:
            r.low = 1
            tr.low1_clamp.append(d)
        r.high = c_int(p75 + OUTLIER_BOUND * (p75 - p25) + .499)
        tr.bounds1[d] = (r.low, r.high)
        avg, x = 0.0, 0
        for v in q:
            if r.low <= v <= r.high:
                avg += float(v)
                x += 1
        avg /= x
        std = 0.0
        for v in q:   # one addition per value, in sorted order: the sum is not exact
            if r.low <= v <= r.high:
                std += (float(v) - avg) * (float(v) - avg)
        std = math.sqrt(std / x)
        r.avg, r.std = avg, std
        r.low = c_int(p25 - MAPPING_BOUND * (p75 - p25) + .499)
        r.high = c_int(p75 + MAPPING_BOUND * (p75 - p25) + .499)
        if r.low > avg - MAX_STDDEV * std:
            r.low = c_int(avg - MAX_STDDEV * std + .499)
            tr.low_cap.append(d)
        if r.high < avg - MAX_STDDEV * std:   # as written at :95
            r.high = c_int(avg + MAX_STDDEV * std + .499)
            tr.high_cap.append(d)
        if r.low < 1:
            r.low = 1
            tr.low2_clamp.append(d)
    n_cand = [len(isize[d]) for d in range(4)]
    mx = max(n_cand)
    for d in range(4):
        if pes[d].failed == 0 and n_cand[d] < mx * MIN_DIR_RATIO:
            pes[d] = Pes(pes[d].low, pes[d].high, 1, pes[d].avg, pes[d].std)
            tr.ratio.append(d)
    return pes, n_cand


def pestat(opt, l_pac, lists):
    """mem_pestat: (pes[4] as mem_pestat leaves them, n_cand[4], PestatTrace).  smem_pestat
    zeroes low, high, avg and std of a failed orientation; zeroed() gives that form."""
    tr = PestatTrace()
    pes, n_cand = pestat_finish(pestat_collect(opt, l_pac, lists, tr), tr)
    return pes, n_cand, tr


def zeroed(pes):
    return [Pes(0, 0, 1, 0.0, 0.0) if r.failed else r for r in pes]


# ------------------------------------------------------------------ mem_pair
@dataclass
class Trace:
    """which branch and which clamp a pair reached"""
    why0: str = ""          # branch 0: "flag", "empty", "none" (mem_pair returned 0), "multi"
    n_cand: int = 0         # entries the reference's u would hold
    q_zero: int = 0         # candidates whose score came out not finite or negative
    tie: bool = False       # the best and the second candidate have equal q: the hash decided
    pe_clamp0: bool = False     # q_pe < 0 (:283)
    pe_clamp60: bool = False    # q_pe > 60 (:284)
    raised: list = field(default_factory=list)     # ends whose MAPQ q_pe raised (:294-295)
    cap40: list = field(default_factory=list)      # ends where q_se + 40 capped it
    cap_csub: list = field(default_factory=list)   # ends the tandem-repeat cap lowered (:298-299)
    host: str = ""


def pen_table(opt, pes):
    """the host's table: pen[d][dist - low] for dist in [low, high]; ValueError past PAIR_TAB_LEN"""
    tab = []
    for d in range(4):
        r = pes[d]
        if r.failed or r.high < r.low:
            tab.append([])
            continue
        if r.high - r.low + 1 > PAIR_TAB_LEN:
            raise ValueError("range past SMEM_PAIR_TAB_LEN")
        tab.append([pen(opt, r, dist) for dist in range(r.low, r.high + 1)])
    return tab


def pen(opt, r, dist):
    """.721 * log(2. * erfc(fabs(ns) * M_SQRT1_2)) * a (:210-211), with the libm's values at 0, inf and NaN"""
    std, num = float(r.std), float(dist) - float(r.avg)
    if std == 0.0:
        ns = math.nan if num == 0.0 else math.copysign(math.inf, num) * (1.0 if math.copysign(1.0, std) > 0 else -1.0)
    else:
        ns = num / std
    x = 2. * math.erfc(math.fabs(ns) * 0.70710678118654752440)
    lg = math.nan if x != x else (-math.inf if x == 0.0 else math.log(x))
    return .721 * lg * opt.a


def raw_mapq(diff, a):
    return c_int(6.02 * diff / a + .499)


def mem_pair(opt, l_pac, pes, a, id_, tr=None):
    """mem_pair (:177-236): (ret, sub, n_sub, z); a = (list0, list1)"""
    tr = tr if tr is not None else Trace()
    v = []
    for r in range(2):
        for i, e in enumerate(a[r]):
            x = e["rb"] if e["rb"] < l_pac else (l_pac << 1) - 1 - e["rb"]
            y = ((e["score"] << 32) & MASK64) | i << 2 | (1 if e["rb"] >= l_pac else 0) << 1 | r
            v.append((x, y))
    v.sort()   # pair64_lt is a total order on these (distinct) keys
    id32 = ((id_ & 0xffffffff) << 8) & 0xffffffff   # an int: the shift in 32 bits, sign-extended below
    idx = (id32 - (1 << 32) if id32 >> 31 else id32) & MASK64
    y_last = [-1, -1, -1, -1]
    u = []
    pens = {}   # the penalty per (orientation, distance): what the stage's table holds
    for i in range(len(v)):
        for r in range(2):
            d = r << 1 | (v[i][1] >> 1 & 1)
            if pes[d].failed:
                continue
            which = r << 1 | ((v[i][1] & 1) ^ 1)
            if y_last[which] < 0:
                continue
            for k in range(y_last[which], -1, -1):
                if (v[k][1] & 3) != which:
                    continue
                dist = v[i][0] - v[k][0]
                if dist > pes[d].high:
                    break
                if dist < pes[d].low:
                    continue
                if (d, dist) not in pens:
                    pens[(d, dist)] = pen(opt, pes[d], dist)
                s = float((v[i][1] >> 32) + (v[k][1] >> 32)) + pens[(d, dist)] + .499
                q = c_int(s)
                if q < 0:
                    q = 0
                if not (s >= 0.0) or math.isinf(s):
                    tr.q_zero += 1
                py = k << 32 | i
                u.append((q << 32 | (hash_64(py ^ idx) & 0xffffffff), py))
        y_last[v[i][1] & 3] = i
    tr.n_cand = len(u)
    z = [0, 0]
    if not u:
        return 0, 0, 0, z
    tmp = max(opt.a + opt.b, opt.o_del + opt.e_del, opt.o_ins + opt.e_ins)
    u.sort()
    i, k = u[-1][1] >> 32, u[-1][1] & 0xffffffff
    z[v[i][1] & 1] = (v[i][1] & 0xffffffff) >> 2
    z[v[k][1] & 1] = (v[k][1] & 0xffffffff) >> 2
    ret = u[-1][0] >> 32
    sub = u[-2][0] >> 32 if len(u) > 1 else 0
    tr.tie = len(u) > 1 and sub == ret
    n_sub = sum(1 for e in u[:-1] if sub - (e[0] >> 32) <= tmp)
    return ret, sub, n_sub, z


def pair(opt, l_pac, pes, a, id_, tab_len=TAB_LEN):
    """the decision of mem_sam_pe for one pair whose lists a = (list0, list1) went through
    mem_mark_primary_se (:266-304, :321-326): (smem_pair_sel_t as a dict, Trace).  The lists are
    left as they are; line 291's side effect is reported in sub / promoted."""
    tr = Trace()
    sel = dict(status=0, branch=0, z=[0, 0], mapq=[-1, -1], proper=0, o=0, subo=0, n_sub=0, sub=[0, 0],
               promoted=[0, 0])
    if any(len(x) > MAX_REGS for x in a):
        tr.host = "list"
        return dict(sel, status=PAIR_HOST, mapq=[0, 0]), tr

    def no_pairing(why):
        tr.why0 = why
        if not opt.nopairing and all(x and x[0]["score"] >= opt.T for x in a):   # :321-325, short of the rid test
            d, dist = infer_dir(l_pac, a[0][0]["rb"], a[1][0]["rb"])
            if not pes[d].failed and pes[d].low <= dist <= pes[d].high:
                sel["proper"] = 2
        return sel, tr

    if opt.nopairing:
        return no_pairing("flag")
    if not a[0] or not a[1]:
        return no_pairing("empty")
    o, subo, n_sub, z = mem_pair(opt, l_pac, pes, a, id_, tr)
    sel["o"], sel["subo"], sel["n_sub"] = o, subo, n_sub
    if o <= 0:
        return no_pairing("none")
    for i in range(2):                                                        # :271-276
        if any(x["secondary"] < 0 and x["score"] >= opt.T for x in a[i][1:]):
            return no_pairing("multi")
    try:
        score_un = a[0][0]["score"] + a[1][0]["score"] - opt.pen_unpaired     # :278
        subo = max(subo, score_un)                                            # :280
        q_pe = raw_mapq(o - subo, opt.a)
        if n_sub > 0:
            if n_sub >= tab_len:
                raise ToHost("n_sub")
            q_pe -= int(4.343 * math.log(n_sub + 1) + .499)
        if q_pe < 0:
            q_pe, tr.pe_clamp0 = 0, True
        if q_pe > 60:
            q_pe, tr.pe_clamp60 = 60, True
        q_se = [0, 0]
        if o > score_un:                                                      # :286-299
            sel["branch"], sel["z"], sel["proper"] = 1, list(z), 2
            for i in range(2):
                c = dict(a[i][z[i]])
                if c["secondary"] >= 0:
                    c["sub"] = a[i][c["secondary"]]["score"]
                    sel["promoted"][i] = 1
                sel["sub"][i] = c["sub"]
                q = approx_mapq_se(opt, c, tab_len)
                if q < 0:
                    raise ToHost("mapq")
                if q <= q_pe:
                    if q_pe < q + 40:
                        if q_pe > q:
                            tr.raised.append(i)
                        q = q_pe
                    else:
                        q = q + 40
                        tr.raised.append(i)
                        tr.cap40.append(i)
                cap = raw_mapq(c["score"] - c["csub"], opt.a)
                if not q < cap:
                    if cap < q:
                        tr.cap_csub.append(i)
                    q = cap
                q_se[i] = q
        else:                                                                 # :300-304
            sel["branch"] = 2
            for i in range(2):
                q_se[i] = approx_mapq_se(opt, a[i][0], tab_len)
                if q_se[i] < 0:
                    raise ToHost("mapq")
        sel["mapq"] = q_se
    except ToHost as e:
        tr.host = str(e)
        return dict(status=PAIR_HOST, branch=0, z=[0, 0], mapq=[0, 0], proper=0, o=0, subo=0, n_sub=0, sub=[0, 0],
                    promoted=[0, 0]), tr
    return sel, tr
