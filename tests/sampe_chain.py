"""From a paired read set's raw regions to the records and the per-pair selection the paired-end
SAM stage prints, shared by tests/test_samtext_pe.py, tests/test_gpu_samtext_pe.py and
tests/golden/make_golden_sampe.py.  Two sources give the same shape -- per pair ((read, read),
sel), a read a dict (name, codes, qual, comment, recs, fin_status) of samtext_ref.Rec:

  restated(F)      pair_chain.run_chain, then samtext_pe_ref.printed (regfin_ref.select in branch
                   0, region z[e] in branch 1 and 2) and reg2aln_ref.reg2aln with the contig lookup
                   of xref_ref;
  library(gpu, F)  Gpu.pestat -> matesw -> reg_finalize(id << 1 | end) -> pair -> reg2aln, with only
                   the assembly between the calls done here: the pairs rescue left to the host, the
                   regions each read prints, the contig of every alignment.

Sets: "sampe" (tests/golden/sampe) and the pairing sets "rep", "rep_a2" (tests/golden/pair), all on
the genome p1.  load(name)["want"] is the reference's SAM cut into one text per read.
"""
import functools
import gzip
import json
import os

import numpy as np

from tests import golden_data, pair_chain as PC, reg2aln_ref, samtext_pe_ref as R, xref_ref as X

SAMPE = os.path.join(golden_data.GOLDEN, "sampe")
SETS = ("sampe", "rep", "rep_a2")
# pairs the restated chain leaves to the host, pinned by number (at most PC.MAX_HOST_FRACTION of a set)
HOST_PAIRS = {"sampe": [], "rep": [], "rep_a2": []}


# the classes of lines a paired-end set must hold, MIN_CLASS lines each (tests/golden/make_golden_sampe.py
# refuses a set without them; tests/test_samtext_pe.py asserts them from the committed files)
MIN_CLASS = 10
CLASSES = ("mate_unmapped_on_mapped", "unmapped_placed_forward", "unmapped_placed_reverse", "unmapped_no_coordinate",
           "rnext_name", "supplementary_rnext_eq", "supplementary_rnext_name", "same_strand", "tlen_positive",
           "tlen_negative", "tlen_zero_rnext_eq", "proper", "not_proper_one_contig")


def classes(sam_bytes):
    """lines of the SAM per class of CLASSES"""
    c = {k: 0 for k in CLASSES}
    for line in sam_bytes.split(b"\n"):
        if not line or line.startswith(b"@"):
            continue
        f = line.split(b"\t")
        flag, rname, rnext, tlen = int(f[1]), f[2], f[6], int(f[8])
        c["mate_unmapped_on_mapped"] += bool(flag & 0x8) and not flag & 0x4
        c["unmapped_placed_forward"] += bool(flag & 0x4) and rname != b"*" and not flag & 0x10
        c["unmapped_placed_reverse"] += bool(flag & 0x4) and rname != b"*" and bool(flag & 0x10)
        c["unmapped_no_coordinate"] += bool(flag & 0x4) and rname == b"*"
        c["rnext_name"] += rnext not in (b"=", b"*")
        c["supplementary_rnext_eq"] += bool(flag & 0x800) and rnext == b"="
        c["supplementary_rnext_name"] += bool(flag & 0x800) and rnext not in (b"=", b"*")
        c["same_strand"] += not flag & 0xc and bool(flag & 0x10) == bool(flag & 0x20)
        c["tlen_positive"] += tlen > 0
        c["tlen_negative"] += tlen < 0
        c["tlen_zero_rnext_eq"] += tlen == 0 and rnext == b"="
        c["proper"] += bool(flag & 0x2)
        c["not_proper_one_contig"] += not flag & 0x2 and not flag & 0xc and rnext == b"="
    return {k: int(v) for k, v in c.items()}


def parse_fastq(fq_bytes):
    """(names, codes per read, qualities per read) of a FASTQ of four-line records"""
    from smemgpu import synth
    lines = fq_bytes.split(b"\n")
    names, reads, quals = [], [], []
    for k in range(0, len(lines) - 1, 4):
        names.append(lines[k][1:].split()[0].decode())
        reads.append(synth.NT4[np.frombuffer(lines[k + 1], dtype=np.uint8)].astype(np.uint8))
        quals.append(np.frombuffer(lines[k + 3], dtype=np.uint8))
    return names, reads, quals


def sam_texts(sam_bytes):
    """the SAM's lines cut into one text per read: a new read starts where QNAME or 0x80 changes"""
    out, last = [], None
    for line in sam_bytes.split(b"\n"):
        if not line or line.startswith(b"@"):
            continue
        f = line.split(b"\t", 2)
        key = (f[0], int(f[1]) & 0x80)
        if key != last:
            out.append(b"")
            last = key
        out[-1] += line + b"\n"
    return out


@functools.lru_cache(maxsize=None)
def load(name):
    d = SAMPE if name == "sampe" else PC.PAIR
    with open(os.path.join(d, name + ".json")) as fh:
        man = json.load(fh)
    raw = {}
    for ext in ("fq", "smrg", "sam"):
        with gzip.open(os.path.join(d, f"{name}.{ext}.gz"), "rb") as fh:
            raw[ext] = fh.read()
    return make(man, raw["fq"], raw["smrg"], raw["sam"])


def make(man, fq, smrg, sam):
    names, reads, quals = parse_fastq(fq)
    _, lists = PC.parse_set(fq, smrg)
    G, l_pac, pac, contigs = PC.genome(man["genome"])
    assert len(reads) == 2 * man["pairs"] == len(lists)
    want = sam_texts(sam)
    assert len(want) == len(reads)
    return dict(man=man, names=names, reads=reads, quals=quals, lists=lists, G=G, l_pac=l_pac, pac=pac, contigs=contigs,
                O=PC.OPTS[man.get("options", "default")], want=want)


def _read(F, r, recs, fin_status=0):
    return dict(name=F["names"][r], codes=F["reads"][r], qual=F["quals"][r], comment="", recs=recs, fin_status=fin_status)


def _rec(F, reg, aln, mapq, flag, xs):
    """a printed record: the alignment with its contig (a region across two contigs needs
    bwa_fix_xref2: the read is the host's)"""
    _n, offs, lens = X.table(F["contigs"])
    status, rid = aln.status, -1
    if status == 0 and X.needs_fix(offs, lens, F["l_pac"], reg["rb"], reg["re"]):
        status = X.XREF
    if status == 0:
        rid = X.pos2rid(offs, F["l_pac"], aln.pos)
    if status != 0:
        return R.Rec(status=status, rid=-1, pos=-1, mapq=mapq, flag=flag, score=reg["score"], xs=xs)
    return R.Rec(status=0, rid=rid, pos=aln.pos, is_rev=aln.is_rev, cigar=tuple(aln.cigar), NM=aln.NM, md=aln.md, mapq=mapq,
                 flag=flag, score=reg["score"], xs=xs)


def restated(F):
    """[((read, read), sel)] of every pair from the restated chain; a pair left to the host by the
    rescue or the pairing has sel["status"] 1 and no records"""
    fin, _pes, out, status = PC.run_chain(F["G"], F["l_pac"], F["reads"], F["lists"], F["O"])
    pairs = []
    for p, (sel, _tr) in enumerate(out):
        if sel["status"] or status[p]:
            pairs.append(((_read(F, 2 * p, []), _read(F, 2 * p + 1, [])), dict(status=1, branch=0, proper=0, mapq=[-1, -1])))
            continue
        rd = []
        for e in range(2):
            r = 2 * p + e
            recs = [_rec(F, reg, reg2aln_ref.reg2aln(F["O"]["g2a"], F["l_pac"], F["pac"], F["reads"][r], reg), mapq, flag, xs)
                    for reg, mapq, flag, xs in R.printed(F["O"]["fin"], fin[r], sel, e)]
            rd.append(_read(F, r, recs))
        pairs.append((tuple(rd), dict(status=0, branch=sel["branch"], proper=sel["proper"], mapq=list(sel["mapq"]))))
    return pairs


def texts(F, pairs):
    """samtext_pe_ref.pair_text of every pair: one text per read, None for a host pair's reads"""
    names, offs, _l = X.table(F["contigs"])
    out = []
    for rd, sel in pairs:
        t = R.pair_text(rd, sel, names, offs)
        out += t if t is not None else [None, None]
    return out


# ------------------------------------------------------------------ the library's own results
def library(gpu, F):
    """(SamResults of Gpu.sam_text_pe, sel as Gpu.pair returned it with the rescue's host pairs
    marked) from the set's regions through library calls alone"""
    from smemgpu.lib import ALNREG_DT, SAM_REC_DT
    from tests import pair_data
    import test_gpu_matesw
    import test_gpu_pair
    import test_gpu_regfin
    import test_reg2aln
    O, l_pac, pac = F["O"], F["l_pac"], F["pac"]
    n = len(F["reads"])
    codes = np.concatenate(F["reads"])
    lens = np.array([x.size for x in F["reads"]], dtype=np.int32)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    regs, reg_off = pair_data.arrays(F["lists"])
    pes, _n_cand, _ms = gpu.pestat(regs, reg_off, l_pac, test_gpu_pair.c_pestat_opt(O["pair"]))
    pes3 = [(int(x["low"]), int(x["high"]), int(x["failed"])) for x in pes]
    regs, reg_off, _n_sw, msw_status, _ms = gpu.matesw(pac, l_pac, codes, offs, regs, reg_off, pes3,
                                                       test_gpu_matesw.c_opt(O["msw"]))
    fin = gpu.reg_finalize(lens, regs, reg_off, test_gpu_regfin._c_opt(O["fin"]), ids=np.arange(n, dtype=np.int64))
    sel, _ms = gpu.pair(fin.regs, fin.out_off, l_pac, pes, test_gpu_pair.c_pair_opt(O["pair"]))
    sel = sel.copy()
    sel["status"] |= (np.asarray(msw_status) != 0).astype(np.int32)
    # the regions each read prints, and what the record carries beside its alignment
    pick, recs, aln_off = [], [], [0]
    for r in range(n):
        S = sel[r >> 1]
        lo = int(fin.out_off[r])
        if S["status"] == 0 and S["branch"] == 0:
            for k in fin.sel_idx[int(fin.sel_off[r]):int(fin.sel_off[r + 1])]:
                k = int(k)                                         # (an index into fin.regs)
                pick.append(fin.regs[k])
                recs.append((int(fin.sel[k]["mapq"]), int(fin.sel[k]["flag"]), int(fin.regs[k]["score"]), int(fin.sel[k]["xs"])))
        elif S["status"] == 0:
            e = r & 1
            reg = fin.regs[lo + int(S["z"][e])].copy()
            if S["branch"] == 1:
                reg["sub"] = S["sub"][e]                           # software/bwamem_pair.c:291
            pick.append(reg)
            recs.append((int(S["mapq"][e]), 0, int(reg["score"]), max(int(reg["sub"]), int(reg["csub"]))))
        aln_off.append(len(pick))
    pick = np.array(pick, dtype=ALNREG_DT) if pick else np.zeros(0, dtype=ALNREG_DT)
    aln_off = np.array(aln_off, dtype=np.uint64)
    alns, cigar, md, _ms = gpu.reg2aln(pac, l_pac, codes, offs, pick, aln_off, test_reg2aln._c_opt(O["g2a"]))
    alns = alns[:pick.size].copy()
    names, ctg_offs, ctg_lens = X.table(F["contigs"])
    rid = np.full(pick.size, -1, dtype=np.int32)
    for k in range(pick.size):                                     # bwa_fix_xref2's test and bns_pos2rid stay the caller's
        if alns[k]["status"] == 0 and X.needs_fix(ctg_offs, ctg_lens, l_pac, int(pick[k]["rb"]), int(pick[k]["re"])):
            alns[k]["status"] = X.XREF
        if alns[k]["status"] == 0:
            rid[k] = X.pos2rid(ctg_offs, l_pac, int(alns[k]["pos"]))
    got = gpu.sam_text_pe(sel, codes, offs, F["names"], np.concatenate(F["quals"]), None, aln_off, alns, rid,
                          np.array(recs, dtype=SAM_REC_DT) if recs else np.zeros(0, dtype=SAM_REC_DT), cigar, md, ctg_offs,
                          names, fin_status=fin.status)
    return got, sel
