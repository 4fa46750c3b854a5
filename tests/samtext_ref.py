"""Python restatement of the reference's single-end SAM text: mem_reg2sam_se
(software/bwamem.c:1359-1393) through mem_aln2sam (:1214-1327) with extra_flag 0
and no mate, over the records the other restatements produce (tests/regfin_ref.py:
selection, MAPQ, flags, XS; tests/reg2aln_ref.py: CIGAR, NM, MD, position, strand;
tests/xref_ref.py: the contig).  Line numbers cite software/bwamem.c.

tests/test_samtext.py pins read_text() to the reference's own lines, byte for byte;
tests/test_gpu_samtext.py then uses it as the expectation for smem_batch_sam and
smem_sam_text.
"""
from dataclasses import dataclass

FIN_REJECT = 1                                # SMEM_FIN_REJECT


@dataclass
class Rec:
    """one mem_aln_t of a read's list as mem_reg2sam_se leaves it (:1373-1379), short of 0x10"""
    status: int = 0                           # smem_aln_t.status: 0, or the read goes to the host
    rid: int = -1
    pos: int = -1                             # concatenated forward-strand coordinate (smem_aln_t.pos)
    is_rev: int = 0
    cigar: tuple = ()                         # (len << 4 | op, ...), op 0 M 1 I 2 D 3 S
    NM: int = 0
    md: str = ""
    mapq: int = 0                             # finalize's capped value; -1: the caller's
    flag: int = 0                             # finalize's: 0x100, 0x800, 0x10000
    score: int = 0                            # the final region's score (AS)
    xs: int = -1                              # max(sub, csub); -1: none (:1376)


def cigar_text(ops, hard):                    # :1239-1243 (hard: which != 0), :1316-1318 (hard False)
    return "".join(f"{w >> 4}{'MIDSH'[(4 if hard else 3) if (w & 0xf) in (3, 4) else (w & 0xf)]}" for w in ops)


def goes_to_host(recs, l_seq, fin_status=0):
    """the reject -> CPU convention of smem_batch_sam: the whole read is the caller's"""
    return fin_status == FIN_REJECT or l_seq == 0 or any(r.status != 0 or r.mapq == -1 for r in recs)


def aln2sam(name, codes, qual, comment, ctg_names, ctg_offs, recs, which, rg_id=None):
    """mem_aln2sam(bns, str, s, n, list, which, 0) -> the line's bytes.  recs is None for the
    unmapped record t = mem_reg2aln(.., 0) (:1381-1385): rid -1, flag 4, score and sub 0."""
    unmapped = recs is None
    p = Rec(rid=-1, score=0, xs=0) if unmapped else recs[which]
    flag = p.flag | (0x4 if p.rid < 0 else 0) | (0x10 if p.is_rev else 0)          # :1222, 1228
    out = [name, "\t", str((flag & 0xffff) | (0x100 if flag & 0x10000 else 0)), "\t"]   # :1232-1233
    if p.rid >= 0:                                                                  # :1234-1244
        out += [ctg_names[p.rid], "\t", str(p.pos - int(ctg_offs[p.rid]) + 1), "\t", str(p.mapq), "\t"]
        out.append(cigar_text(p.cigar, which != 0) if p.cigar else "*")
    else:
        out.append("*\t0\t0\t*")                                                    # :1245
    out.append("\t*\t0\t0\t")                                                       # :1246, 1260-1261
    l_seq = len(codes)
    if flag & 0x100:                                                                # :1264-1265
        out.append("*\t*")
    else:
        qb, qe = 0, l_seq
        if p.cigar and which:                                                       # :1268-1271, 1282-1285
            first = (p.cigar[0] >> 4) if (p.cigar[0] & 0xf) in (3, 4) else 0
            last = (p.cigar[-1] >> 4) if (p.cigar[-1] & 0xf) in (3, 4) else 0
            if not p.is_rev:
                qb, qe = qb + first, qe - last
            else:
                qe, qb = qe - first, qb + last
        if not p.is_rev:                                                            # :1273-1279
            out.append("".join("ACGTN"[int(c)] for c in codes[qb:qe]))
            out.append("\t")
            out.append(bytes(qual[qb:qe]).decode("latin-1") if qual is not None else "*")
        else:                                                                       # :1287-1293
            out.append("".join("TGCAN"[int(c)] for c in codes[qb:qe][::-1]))
            out.append("\t")
            out.append(bytes(qual[qb:qe][::-1]).decode("latin-1") if qual is not None else "*")
    if p.cigar:                                                                     # :1297-1300
        out += ["\tNM:i:", str(p.NM), "\tMD:Z:", p.md]
    if p.score >= 0:                                                                # :1301
        out += ["\tAS:i:", str(p.score)]
    if p.xs >= 0:                                                                   # :1302
        out += ["\tXS:i:", str(p.xs)]
    if rg_id:                                                                       # :1303
        out += ["\tRG:Z:", rg_id]
    if not unmapped and not flag & 0x100:                                           # :1304-1323
        others = [r for i, r in enumerate(recs) if i != which and not r.flag & 0x100]
        if others:
            out.append("\tSA:Z:")
            for r in others:
                out.append(f"{ctg_names[r.rid]},{r.pos - int(ctg_offs[r.rid]) + 1},{'+-'[r.is_rev]},"
                           f"{cigar_text(r.cigar, False)},{r.mapq},{r.NM};")
    if comment:                                                                     # :1325 (an empty comment is none: kseq)
        out += ["\t", comment]
    out.append("\n")                                                                # :1326
    return "".join(out).encode("latin-1")


def read_text(name, codes, qual, comment, ctg_names, ctg_offs, recs, rg_id=None, fin_status=0):
    """mem_reg2sam_se's s->sam for one read (:1381-1391), or None when the read goes to the
    host (SMEM_SAM_HOST: zero bytes from the stage)"""
    if goes_to_host(recs, len(codes), fin_status):
        return None
    if not recs:
        return aln2sam(name, codes, qual, comment, ctg_names, ctg_offs, None, 0, rg_id)
    return b"".join(aln2sam(name, codes, qual, comment, ctg_names, ctg_offs, recs, k, rg_id)
                    for k in range(len(recs)))


def recs_of(row, fin_a, fin_sel):
    """Rec list of one read from xref_ref.expected_rows' row [(final region, Aln, rid)] and
    finalize()'s (a, sel): the region's place in `a` finds its (mapq, flag, xs)"""
    out = []
    for p, aln, rid in row:
        k = next(i for i, q in enumerate(fin_a) if q is p)
        mapq, flag, xs = (int(v) for v in fin_sel[k])
        out.append(Rec(status=aln.status, rid=rid, pos=aln.pos, is_rev=aln.is_rev, cigar=tuple(aln.cigar), NM=aln.NM,
                       md=aln.md, mapq=mapq, flag=flag, score=int(p["score"]), xs=xs))
    return out
