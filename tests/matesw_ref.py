"""Python restatement of mate rescue: mem_infer_dir (software/bwamem_pair.c:23-30),
mem_matesw (:109-175) and the rescue loop of mem_sam_pe (:252-263).

Every SW is oracle.ksw_align2 (pinned to the reference's ksw_align2 at long
targets by tests/test_ksw_align_long.py), every mem_sort_and_dedup is
regfin_ref.sort_and_dedup (comparison-for-comparison ks_introsort).  The GPU
stage (smem_matesw) is checked against matesw() list by list;
tests/test_matesw.py pins matesw() to the reference's own mem_matesw on the
hand-built lists (tests/golden/msw/hand) and to its SAM on the paired-end set.

Regions are dicts of regfin_ref.FIELDS.  What the stage leaves to the host
(SMEM_MSW_HOST: input lists copied through, n_sw = 0) is decided here the same
way: a mate of 0 or more than 256 bp, an input list above MAX_REGS, a window
above MAX_TLEN that an SW would run on, a list that would pass MAX_REGS.
"""
from dataclasses import dataclass, field

import numpy as np

from oracle import oracle
from tests import regfin_ref

MAX_TLEN = 2048      # SMEM_KSWA_MAX_TLEN
MAX_REGS = regfin_ref.MAX_REGS
MSW_HOST = 1         # SMEM_MSW_HOST
XBYTE, XSUBO, XSTART = 0x10000, 0x40000, 0x80000


@dataclass
class Opt:
    a: int = 1
    b: int = 4
    o_del: int = 6
    e_del: int = 1
    o_ins: int = 6
    e_ins: int = 1
    min_seed_len: int = 19
    pen_unpaired: int = 17
    max_matesw: int = 100
    mask_level_redun: float = 0.95


@dataclass
class Pes:
    """mem_pestat_t (software/bwamem.h:78-82); the stage reads low, high, failed"""
    low: int = 0
    high: int = 0
    failed: int = 1
    avg: float = 0.0
    std: float = 0.0


class ToHost(Exception):
    pass


@dataclass
class Trace:
    """what the loop met, per pair (the hand-built set asserts its groups by these)"""
    sw: int = 0            # SWs run
    inserted: int = 0      # candidate regions inserted
    below: int = 0         # SWs whose score stayed under min_seed_len (or qb < 0)
    bridged: int = 0       # windows across l_pac: no SW
    clipped: int = 0       # windows cut at 0 or 2 l_pac
    calls: int = 0         # mem_matesw calls that got past the skip test
    all_skipped: int = 0   # mem_matesw calls that returned at :121
    dedup_drop: int = 0    # regions mem_sort_and_dedup removed
    dirs: list = field(default_factory=list)   # orientations an SW ran for
    byte: int = 0
    word: int = 0
    host: str = ""         # why the pair is the host's: "mate", "window" or "list"
    at: list = field(default_factory=list)        # (insertion index, list length before) per insertion
    windows: list = field(default_factory=list)   # (orientation, rb, re) after the cuts, per open orientation


def infer_dir(l_pac, b1, b2):
    """mem_infer_dir (:23-30): (direction, distance)"""
    r1, r2 = b1 >= l_pac, b2 >= l_pac
    p2 = b2 if r1 == r2 else (l_pac << 1) - 1 - b2
    dist = p2 - b1 if p2 > b1 else b1 - p2
    return (0 if r1 == r2 else 1) ^ (0 if p2 > b1 else 3), dist


def get_seq(l_pac, fwd, beg, end):
    """bns_get_seq (software/bntseq.c:355-376) over the forward strand's codes: (sequence, len)"""
    if end < beg:
        beg, end = end, beg
    end = min(end, l_pac << 1)
    beg = max(beg, 0)
    if beg >= l_pac or end <= l_pac:
        if beg >= l_pac:
            bf, ef = (l_pac << 1) - 1 - end, (l_pac << 1) - 1 - beg
            return (3 - fwd[bf + 1:ef + 1][::-1]).astype(np.uint8), end - beg
        return fwd[beg:end].astype(np.uint8), end - beg
    return np.zeros(0, np.uint8), 0


def _new_reg():
    return {k: 0 for k in regfin_ref.FIELDS}


def matesw_one(opt, l_pac, fwd, pes, a, ms, ma, mat, tr):
    """mem_matesw (:109-175): anchor a, mate codes ms, the mate's list ma (changed in place);
    returns (n, ma)"""
    from smemgpu import synth
    l_ms = ms.size
    skip = [1 if pes[r].failed else 0 for r in range(4)]                     # :113-114
    for x in ma:                                                              # :115-120
        r, dist = infer_dir(l_pac, a["rb"], x["rb"])
        if pes[r].low <= dist <= pes[r].high:
            skip[r] = 1
    if sum(skip) == 4:                                                        # :121
        tr.all_skipped += 1
        return 0, ma
    tr.calls += 1
    n = 0
    for r in range(4):                                                        # :122
        if skip[r]:
            continue
        is_rev = (r >> 1) != (r & 1)                                          # :127
        is_larger = not (r >> 1)                                              # :128
        seq = np.where(ms < 4, 3 - ms, 4)[::-1].astype(np.uint8) if is_rev else ms   # :129-133
        if not is_rev:                                                        # :134-140
            rb = a["rb"] + pes[r].low if is_larger else a["rb"] - pes[r].high
            re = (a["rb"] + pes[r].high if is_larger else a["rb"] - pes[r].low) + l_ms
        else:
            rb = (a["rb"] + pes[r].low if is_larger else a["rb"] - pes[r].high) - l_ms
            re = a["rb"] + pes[r].high if is_larger else a["rb"] - pes[r].low
        if rb < 0 or re > l_pac << 1:
            tr.clipped += 1
        rb = max(rb, 0)                                                       # :141
        re = min(re, l_pac << 1)                                              # :142
        tr.windows.append((r, int(rb), int(re)))
        ref, ln = get_seq(l_pac, fwd, rb, re)                                 # :143
        if ln == re - rb:                                                     # :144
            if ln > MAX_TLEN:
                raise ToHost("window")
            xtra = XSUBO | XSTART | (XBYTE if l_ms * opt.a < 250 else 0) | (opt.min_seed_len * opt.a)   # :147
            if xtra & XBYTE:
                tr.byte += 1
            else:
                tr.word += 1
            kb = synth.KswBatch(np.array([(0, 0, l_ms, ln, xtra, 0)], dtype=synth.KSWA_TASK), seq, ref, mat,
                                opt.o_del, opt.e_del, opt.o_ins, opt.e_ins)
            aln = oracle.ksw_align2(kb)[0]                                    # :148
            tr.sw += 1
            tr.dirs.append(r)
            if aln["score"] >= opt.min_seed_len and aln["qb"] >= 0:           # :150
                b = _new_reg()
                b["qb"] = int(l_ms - (aln["qe"] + 1) if is_rev else aln["qb"])             # :151-154
                b["qe"] = int(l_ms - aln["qb"] if is_rev else aln["qe"] + 1)
                b["rb"] = int((l_pac << 1) - (rb + aln["te"] + 1) if is_rev else rb + aln["tb"])
                b["re"] = int((l_pac << 1) - (rb + aln["tb"]) if is_rev else rb + aln["te"] + 1)
                b["score"] = int(aln["score"])                                # :155-158
                b["csub"] = int(aln["score2"])
                b["secondary"] = -1
                b["seedcov"] = min(b["re"] - b["rb"], b["qe"] - b["qb"]) >> 1
                if len(ma) + 1 > MAX_REGS:
                    raise ToHost("list")
                at = len(ma)                                                  # :160-166
                for i, x in enumerate(ma):
                    if x["score"] < b["score"]:
                        at = i
                        break
                tr.at.append((at, len(ma)))
                ma.insert(at, b)
                tr.inserted += 1
            else:
                tr.below += 1
            n += 1                                                            # :168
        else:
            tr.bridged += 1
        if n:                                                                 # :170
            before = len(ma)
            ma = regfin_ref.sort_and_dedup(ma, opt.mask_level_redun)
            tr.dedup_drop += before - len(ma)
    return n, ma


def matesw_pair(opt, l_pac, fwd, pes, reads, lists, mat=None):
    """lines 252-263 for one pair: reads = (codes0, codes1), lists = (regions0, regions1), both
    left as they are.  Returns (lists after rescue, n, status, Trace)."""
    from smemgpu import synth
    if mat is None:
        mat = synth.bwa_scmat(opt.a, opt.b)
    tr = Trace()
    keep = [[dict(x) for x in lists[0]], [dict(x) for x in lists[1]]]
    if any(r.size < 1 or r.size > 256 for r in reads) or any(len(x) > MAX_REGS for x in lists):
        tr.host = "mate" if any(r.size < 1 or r.size > 256 for r in reads) else "list"
        return keep, 0, MSW_HOST, tr
    a = [[dict(x) for x in lists[0]], [dict(x) for x in lists[1]]]
    b = [[dict(x) for x in a[i] if x["score"] >= a[i][0]["score"] - opt.pen_unpaired] for i in range(2)]   # :255-258
    n = 0
    try:
        for i in range(2):                                                    # :259-261
            for j in range(min(len(b[i]), opt.max_matesw)):
                k, a[1 - i] = matesw_one(opt, l_pac, fwd, pes, b[i][j], reads[1 - i], a[1 - i], mat, tr)
                n += k
    except ToHost as e:
        tr.host = str(e)
        return keep, 0, MSW_HOST, tr
    return a, n, 0, tr


def matesw(opt, l_pac, fwd, pes, codes, offs, regs, reg_off):
    """every pair: (lists per read, n_sw per pair, status per pair, Trace per pair); regs is a list
    of dicts or an ALNREG_DT array"""
    n_pairs = (len(offs) - 1) // 2
    out, n_sw, status, traces = [], [], [], []
    for p in range(n_pairs):
        reads = tuple(np.asarray(codes[int(offs[2 * p + e]):int(offs[2 * p + e + 1])], dtype=np.uint8) for e in range(2))
        lists = tuple([_as_dict(regs[k]) for k in range(int(reg_off[2 * p + e]), int(reg_off[2 * p + e + 1]))]
                      for e in range(2))
        a, n, st, tr = matesw_pair(opt, l_pac, fwd, pes, reads, lists)
        out += [a[0], a[1]]
        n_sw.append(n)
        status.append(st)
        traces.append(tr)
    return out, n_sw, status, traces


def _as_dict(x):
    if isinstance(x, dict):
        return dict(x)
    return {k: int(x[k]) for k in regfin_ref.FIELDS}
