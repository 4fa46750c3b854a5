"""Python restatement of the reference's paired-end SAM text: mem_aln2sam with a mate
(software/bwamem.c:1214-1327; the mate's part is :1219-1229 and :1249-1260) and the tail of
mem_sam_pe (software/bwamem_pair.c:305-331) -- which records each read prints per branch, the
mate h[!e] of every line, and the rid AND of :321.  Everything from SEQ on is the single-end
restatement's (tests/samtext_ref.py, reused by import): a line is printed by samtext_ref.aln2sam
from the record as :1219-1229 leave it, and its three mate fields are replaced.

tests/test_samtext_pe.py pins pair_text() to the reference's own SAM, byte for byte;
tests/test_gpu_samtext_pe.py then uses it as the expectation for smem_sam_text_pe.
"""
from dataclasses import replace

from tests import samtext_ref as S

Rec = S.Rec
UNMAPPED = Rec(rid=-1, pos=-1, is_rev=0, cigar=(), mapq=0, flag=0, score=0, xs=0)   # mem_reg2aln(.., 0)


def get_rlen(cigar):                                       # bwamem.c:1203-1212
    return sum(w >> 4 for w in cigar if (w & 0xf) in (0, 2))


def tlen(p, m):
    """:1254-1258 for p->rid == m->rid: 0 when either side has no CIGAR, else -(p0 - p1 + sign)
    over the 5' ends"""
    if not p.cigar or not m.cigar:
        return 0
    p0 = p.pos + (get_rlen(p.cigar) - 1 if p.is_rev else 0)
    p1 = m.pos + (get_rlen(m.cigar) - 1 if m.is_rev else 0)
    return -(p0 - p1 + (1 if p0 > p1 else -1 if p0 < p1 else 0))


def aln2sam_pe(name, codes, qual, comment, ctg_names, ctg_offs, recs, which, mate, rg_id=None):
    """mem_aln2sam(bns, str, s, n, list, which, m) with m != 0 -> the line's bytes.  recs: the
    read's list with extra_flag already ORed into every flag (bwamem.c:1375, 1384;
    bwamem_pair.c:306-307) -- the unmapped record is a list of one UNMAPPED; mate: h[!e]."""
    p, m = replace(recs[which]), replace(mate)
    flag = p.flag | 0x1 | (0x4 if p.rid < 0 else 0) | (0x8 if m.rid < 0 else 0)        # :1221-1223
    if p.rid < 0 and m.rid >= 0:                                                         # :1224-1225
        p.rid, p.pos, p.is_rev, p.cigar = m.rid, m.pos, m.is_rev, ()
    if m.rid < 0 and p.rid >= 0:                                                         # :1226-1227
        m.rid, m.pos, m.is_rev, m.cigar = p.rid, p.pos, p.is_rev, ()
    p.flag = flag | (0x20 if m.is_rev else 0)                                            # :1229 (0x10: samtext_ref's)
    lst = list(recs)
    lst[which] = p
    f = S.aln2sam(name, codes, qual, comment, ctg_names, ctg_offs, lst, which, rg_id).split(b"\t", 9)
    assert f[6:9] == [b"*", b"0", b"0"]
    if m.rid >= 0:                                                                       # :1249-1259
        f[6] = b"=" if p.rid == m.rid else ctg_names[m.rid].encode("latin-1")
        f[7] = str(m.pos - int(ctg_offs[m.rid]) + 1).encode()
        f[8] = str(tlen(p, m) if p.rid == m.rid else 0).encode()
    return b"\t".join(f)


def printed(fin_opt, a, sel, e):
    """the regions end e of a pair prints, as (region, mapq, flag, xs), from the end's list `a`
    after mem_mark_primary_se and the pair's selection (tests/pair_ref.pair).  Branch 0:
    mem_reg2sam_se's own loop (bwamem.c:1367-1380; bwamem_pair.c:327-328).  Branch 1 and 2: the
    region z[e] alone (bwamem_pair.c:306-307) -- in branch 1 with the sub of line 291 --, MAPQ
    q_se[e], no flag of its own, XS max(sub, csub) (bwamem.c:1547: mem_reg2aln)."""
    from tests import regfin_ref
    if sel["branch"] == 0:
        sse, idx = regfin_ref.select(fin_opt, a)
        return [(a[k],) + tuple(int(v) for v in sse[k]) for k in idx]
    reg = dict(a[sel["z"][e]])
    if sel["branch"] == 1:
        reg["sub"] = sel["sub"][e]
    return [(reg, int(sel["mapq"][e]), 0, max(reg["sub"], reg["csub"]))]


def pair_host(reads, sel):
    """the pair is the caller's: the pairing stage left it, or either read meets one of the
    single-end stage's conditions (in branch 1 and 2 the pair's MAPQ stands for the record's)"""
    if sel["status"] != 0:
        return True
    for e, r in enumerate(reads):
        recs = r["recs"]
        if sel["branch"] != 0:
            recs = [replace(x, mapq=int(sel["mapq"][e])) for x in recs]
        if S.goes_to_host(recs, len(r["codes"]), r.get("fin_status", 0)):
            return True
    return False


def pair_text(reads, sel, ctg_names, ctg_offs, rg_id=None, qual=True, comments=True):
    """s[0].sam and s[1].sam as mem_sam_pe leaves them (bwamem_pair.c:305-331), or None for a pair
    that goes to the host.  reads: two dicts (name, codes, qual, comment, recs[, fin_status]);
    recs is what the read prints: in branch 0 mem_reg2sam_se's list (:1367-1380; empty: the
    unmapped record), in branch 1 and 2 the one alignment h[e] of region z[e], flag 0.  sel: the
    pair's branch, mapq[2], proper, status."""
    if pair_host(reads, sel):
        return None
    branch = int(sel["branch"])
    h = [r["recs"][0] if r["recs"] else UNMAPPED for r in reads]   # :306-307; :316-320 (record 0 is region 0 when score >= T)
    extra = 1
    if branch != 0:
        assert all(len(r["recs"]) == 1 for r in reads)
        extra |= 2 if sel["proper"] else 0                         # :296
    elif sel["proper"] and h[0].rid == h[1].rid and h[0].rid >= 0:  # :321 (the rest of the test is sel's)
        extra |= 2
    out = []
    for e, r in enumerate(reads):
        fl = (0x40 << e) | extra                                   # :306-307; 0x41 << e | extra_flag of :327-328
        args = (r["name"], r["codes"], r["qual"] if qual else None, r["comment"] if comments else None, ctg_names, ctg_offs)
        if not r["recs"]:                                          # bwamem.c:1381-1385
            t = [replace(UNMAPPED, flag=fl)]
            out.append(aln2sam_pe(*args, t, 0, h[e ^ 1], rg_id))
            continue
        lst = [replace(x, flag=x.flag | fl) for x in r["recs"]]    # bwamem.c:1375
        if branch != 0:
            lst[0].mapq = int(sel["mapq"][e])                      # h[e].mapq = q_se[e]
        out.append(b"".join(aln2sam_pe(*args, lst, k, h[e ^ 1], rg_id) for k in range(len(lst))))
    return out
