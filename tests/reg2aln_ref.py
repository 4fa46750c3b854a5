"""Python restatement of the alignment part of mem_reg2aln: infer_bw,
bwa_gen_cigar2, ksw_global2 and the band-doubling loop, squeeze and clips.
Line numbers cite the reference's software/ directory.  tests/test_reg2aln.py
pins it to reference-made SAM records and then uses it as the expectation for
what no SAM record covers (score, tries, status, synthetic regions)."""
from dataclasses import dataclass

import numpy as np

MINUS_INF = -0x40000000                       # ksw.c:487
UNMAPPED, NOCIGAR, REJECT = 1, 2, 3           # smem_aln_t.status
MAX_QLEN, MAX_TLEN = 1024, 2048               # the library's limits (include/smem_gpu.h)


@dataclass
class Opt:
    """the scoring mem_reg2aln reads from mem_opt_t (bwamem.c:50-52, 60)"""
    a: int = 1
    b: int = 4
    o_del: int = 6
    e_del: int = 1
    o_ins: int = 6
    e_ins: int = 1
    w: int = 100

    def mat(self):                            # bwa_fill_scmat, bwa.c:84-93
        m = [[self.a if i == j else -self.b for j in range(4)] + [-1] for i in range(4)]
        return m + [[-1] * 5]


@dataclass
class Aln:
    pos: int = -1
    is_rev: int = 0
    cigar: tuple = ()                         # (len << 4 | op, ...), clips included
    NM: int = 0
    score: int = 0
    tries: int = 0
    status: int = 0
    md: str = ""


def _c_div(x: int, r: int, add: float) -> int:
    """(int)((double)x / r + add): C truncates toward zero"""
    return int(x / r + add)


def infer_bw(l1, l2, score, a, q, r):         # bwamem.c:1194-1201
    if l1 == l2 and l1 * a - score < (q + r - a) << 1:
        return 0
    w = _c_div(min(l1, l2) * a - score - q, r, 2.)
    return max(w, abs(l1 - l2))


def ksw_global2(query, target, mat, o_del, e_del, o_ins, e_ins, w):   # ksw.c:501-584
    qlen, tlen = len(query), len(target)
    oe_del, oe_ins = o_del + e_del, o_ins + e_ins
    n_col = min(qlen, 2 * w + 1)
    z = bytearray(n_col * tlen)
    H = [MINUS_INF] * (qlen + 1)
    E = [MINUS_INF] * (qlen + 1)
    H[0] = 0                                                           # ksw.c:519-522
    for j in range(1, min(qlen, w) + 1):
        H[j] = -(o_ins + e_ins * j)
    for i in range(tlen):                                              # ksw.c:524-564
        f = MINUS_INF
        q = mat[target[i]]
        beg = i - w if i > w else 0
        end = min(i + w + 1, qlen)
        h1 = -(o_del + e_del * (i + 1)) if beg == 0 else MINUS_INF
        zi = i * n_col - beg
        for j in range(beg, end):
            m, e = H[j], E[j]
            H[j] = h1
            m += q[query[j]]
            if m >= e:
                d, h = 0, m
            else:
                d, h = 1, e
            if h < f:
                d, h = 2, f
            h1 = h
            t = m - oe_del
            e -= e_del
            if e > t:
                d |= 1 << 2
            else:
                e = t
            E[j] = e
            t = m - oe_ins
            f -= e_ins
            if f > t:
                d |= 2 << 4
            else:
                f = t
            z[zi + j] = d
        H[end], E[end] = h1, MINUS_INF
    score = H[qlen]
    cigar = []                                                         # ksw.c:566-580

    def push(op, n):
        if cigar and cigar[-1][0] == op:
            cigar[-1][1] += n
        else:
            cigar.append([op, n])
    which, i, k = 0, tlen - 1, min(tlen + w, qlen) - 1
    while i >= 0 and k >= 0:
        which = z[i * n_col + (k - (i - w if i > w else 0))] >> (which << 1) & 3
        if which == 0:
            push(0, 1)
            i, k = i - 1, k - 1
        elif which == 1:
            push(2, 1)
            i -= 1
        else:
            push(1, 1)
            k -= 1
    if i >= 0:
        push(2, i + 1)
    if k >= 0:
        push(1, k + 1)
    cigar.reverse()
    return score, cigar


def get_seq(pac, l_pac, rb, re):
    """bns_get_seq (bntseq.c) of [rb, re) inside one strand, then bwa_gen_cigar2's
    reversal on the reverse strand (bwa.c:109-114): the complement of the
    forward strand read upwards from 2 l_pac - re"""
    if rb >= l_pac:
        p = np.arange(2 * l_pac - re, 2 * l_pac - rb)
        return [3 - int(x) for x in (pac[p >> 2] >> ((~p & 3) << 1)) & 3]
    p = np.arange(rb, re)
    return [int(x) for x in (pac[p >> 2] >> ((~p & 3) << 1)) & 3]


def gen_cigar2(opt, mat, w_, l_pac, pac, query, rb, re):               # bwa.c:96-179
    """-> (score, cigar ops, NM, MD), or None where the reference returns 0"""
    lq = len(query)
    if lq <= 0 or rb >= re or (rb < l_pac and re > l_pac) or re > 2 * l_pac:   # bwa.c:106-108
        return None
    rseq = get_seq(pac, l_pac, rb, re)
    rlen = len(rseq)
    rev = rb >= l_pac
    if rev:
        query = query[::-1]
    if lq == rlen and w_ == 0:                                         # bwa.c:115-121
        cigar = [[0, lq]]
        score = sum(mat[rseq[i]][query[i]] for i in range(lq))
    else:                                                              # bwa.c:123-139
        max_ins = _c_div(((lq + 1) >> 1) * mat[0][0] - opt.o_ins, opt.e_ins, 1.)
        max_del = _c_div(((lq + 1) >> 1) * mat[0][0] - opt.o_del, opt.e_del, 1.)
        max_gap = max(max_ins, max_del, 1)
        w = min((max_gap + abs(rlen - lq) + 1) >> 1, w_)
        w = max(w, abs(rlen - lq) + 3)
        score, cigar = ksw_global2(query, rseq, mat, opt.o_del, opt.e_del, opt.o_ins, opt.e_ins, w)
    int2base = "TGCAN" if rev else "ACGTN"                             # bwa.c:141-171
    md, x, y, u, n_mm, n_gap = [], 0, 0, 0, 0, 0
    for k, (op, ln) in enumerate(cigar):
        if op == 0:
            for i in range(ln):
                if query[x + i] != rseq[y + i]:
                    md.append(str(u) + int2base[rseq[y + i]])
                    n_mm += 1
                    u = 0
                else:
                    u += 1
            x += ln
            y += ln
        elif op == 2:
            if 0 < k < len(cigar) - 1:
                md.append(str(u) + "^" + "".join(int2base[c] for c in rseq[y:y + ln]))
                u = 0
                n_gap += ln
            y += ln
        else:
            x += ln
            n_gap += ln
    md.append(str(u))
    return score, cigar, n_mm + n_gap, "".join(md)


def reg2aln(opt, l_pac, pac, read, reg) -> Aln:                        # bwamem.c:1481-1553
    """read: the read's codes (0..4); reg: anything with rb, re, qb, qe, truesc, w"""
    rb, re, qb, qe = int(reg["rb"]), int(reg["re"]), int(reg["qb"]), int(reg["qe"])
    truesc, reg_w = int(reg["truesc"]), int(reg["w"])
    if rb < 0 or re < 0:                                               # bwamem.c:1489
        return Aln(status=UNMAPPED)
    mat = opt.mat()
    query = [int(c) for c in read[qb:qe]] if qe > qb else []
    if qe <= qb or rb >= re or (rb < l_pac and re > l_pac) or re > 2 * l_pac:
        return Aln(status=NOCIGAR, NM=-1, tries=1)                     # bwa.c:106-108: no CIGAR (the reference goes on
                                                                       # with an unset score; here the region ends)
    if qe - qb > MAX_QLEN or re - rb > MAX_TLEN:
        return Aln(status=REJECT)
    tmp = infer_bw(qe - qb, re - rb, truesc, opt.a, opt.o_del, opt.e_del)      # bwamem.c:1504-1508
    w2 = infer_bw(qe - qb, re - rb, truesc, opt.a, opt.o_ins, opt.e_ins)
    w2 = max(w2, tmp)
    if w2 > opt.w:
        w2 = min(w2, reg_w)
    i, last_sc, tries = 0, -(1 << 30), 0
    while True:                                                        # bwamem.c:1511-1518
        score, cigar, NM, md = gen_cigar2(opt, mat, w2, l_pac, pac, query, rb, re)
        tries += 1
        if score == last_sc:
            break
        last_sc = score
        w2 <<= 1
        i += 1
        if not (i < 3 and score < truesc - opt.a):
            break
    is_rev = rb >= l_pac                                               # bwamem.c:1521 (bns_depos)
    pos = 2 * l_pac - re if is_rev else rb
    if cigar[0][0] == 2:                                               # bwamem.c:1523-1532
        pos += cigar[0][1]
        cigar = cigar[1:]
    elif cigar[-1][0] == 2:
        cigar = cigar[:-1]
    l_query = len(read)
    ops = [ln << 4 | op for op, ln in cigar]
    if qb != 0 or qe != l_query:                                       # bwamem.c:1533-1547
        clip5 = l_query - qe if is_rev else qb
        clip3 = qb if is_rev else l_query - qe
        if clip5:
            ops.insert(0, clip5 << 4 | 3)
        if clip3:
            ops.append(clip3 << 4 | 3)
    return Aln(pos=pos, is_rev=int(is_rev), cigar=tuple(ops), NM=NM, score=score, tries=tries, status=0, md=md)


# ---- where the GPU stage runs a region (csrc/global_kernels.h, g2a_prep_kernel) ----
GROUPS = (16, 32, 64)                          # lanes of class 0 / 1 / 2; class 3 is the scratch tier
LDS_BIG = 32768                                # G2A_LDS_BIG: the scratch-tier kernel's LDS
SCRATCH_CLASS = 3


def group_lds(group):                          # g2a_group_lds
    return 8192 if group == 64 else 4096


def first_w2(opt, ql, tl, truesc, reg_w):     # g2a_first_w2 (bwamem.c:1504-1508)
    w2 = max(infer_bw(ql, tl, truesc, opt.a, opt.o_ins, opt.e_ins), infer_bw(ql, tl, truesc, opt.a, opt.o_del, opt.e_del))
    return min(w2, reg_w) if w2 > opt.w else w2


def band(opt, ql, tl, w_):                     # g2a_band (bwa.c:125-132)
    max_gap = max(_c_div(((ql + 1) >> 1) * opt.a - opt.o_ins, opt.e_ins, 1.),
                  _c_div(((ql + 1) >> 1) * opt.a - opt.o_del, opt.e_del, 1.), 1)
    return max(min((max_gap + abs(tl - ql) + 1) >> 1, w_), abs(tl - ql) + 3)


def row_bytes(ql, w):                          # g2a_row_bytes: 4 bits a cell
    return (min(ql, 2 * w + 1) + 1) >> 1


def fixed_bytes(ql, tl):                       # g2a_fixed_bytes: column array, query, target
    return (ql + 1) * 8 + ((ql + 3) & ~3) + ((tl + 3) & ~3)


def scratch_need(opt, ql, tl):                 # g2a_scratch_need: the band uncapped
    return row_bytes(ql, band(opt, ql, tl, 0x7fffffff)) * tl


@dataclass
class Shape:
    cls: int                                   # 0..2: 16 / 32 / 64 lanes, 3: scratch tier
    n_col: list                                # per try; 0 where the try needs no DP (equal lengths, band 0)
    nbytes: list                               # per try: fixed bytes + direction matrix
    defer_try: int = 0                         # the 1-based try at which a lane-group kernel hands the region to
                                               # the scratch tier (its matrix outgrew the group's LDS); 0: never

    @property
    def group(self):
        return GROUPS[self.cls] if self.cls < SCRATCH_CLASS else 64

    @property
    def in_lds_tries(self):
        """the tries the region's first kernel runs itself"""
        return len(self.n_col) if not self.defer_try else self.defer_try - 1


def classify(opt, reg, tries=3) -> Shape:
    """The class g2a_prep_kernel gives an alignable region (from its first try's band), and
    the column count and LDS bytes of each of its first `tries` tries (the band doubles;
    how many tries there are is the scores' business: Aln.tries of reg2aln)."""
    ql, tl = int(reg["qe"]) - int(reg["qb"]), int(reg["re"]) - int(reg["rb"])
    w2 = first_w2(opt, ql, tl, int(reg["truesc"]), int(reg["w"]))
    fixed = fixed_bytes(ql, tl)
    n_col, nbytes = [], []
    for _ in range(tries):
        if ql == tl and w2 == 0:
            n_col.append(0)
            nbytes.append(fixed)
        else:
            w = band(opt, ql, tl, w2)
            n_col.append(min(ql, 2 * w + 1))
            nbytes.append(fixed + row_bytes(ql, w) * tl)
        w2 <<= 1
    cls = 0 if n_col[0] <= 16 else 1 if n_col[0] <= 32 else 2
    while cls < SCRATCH_CLASS and nbytes[0] > group_lds(GROUPS[cls]):
        cls += 1
    defer = 0
    if cls < SCRATCH_CLASS:
        defer = next((t + 1 for t in range(tries) if nbytes[t] > group_lds(GROUPS[cls])), 0)
    return Shape(cls, n_col, nbytes, defer)


def cigar_str(ops) -> str:
    return "".join(f"{int(c) >> 4}{'MIDS'[int(c) & 0xf]}" for c in ops)
