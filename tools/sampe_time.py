"""Time the paired-end SAM text (smem_sam_text_pe) beside the single-end stage (smem_sam_text) on the
same records, on one device.

    python tools/sampe_time.py [--pairs 500000] [--chunk 100000] [--genome-bp 2000000] [--json OUT]

The batch of profiles/r18/pair rebuilt: synth.make_pairs, 150 bp, on a synthetic genome with
repeats, in chunks through the resident stages up to smem_batch_reg_finalize; smem_pestat and
smem_pair over the final lists; every read's printed regions (the finalize selection in branch
0, region z[e] in branch 1 and 2) through smem_reg2aln; then, after one untimed round, `--runs`
alternated calls of the two stages over those records.  kernel_ms is both passes (HIP events).
Reported: the medians, the bytes each stage writes, bytes per second, ns per line, the branches,
and whether the paired-end text equals tests/samtext_pe_ref.py's for the first `--check` pairs.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "bwa-mem-harp2_amd"), ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def pack(codes):
    c = np.concatenate([codes, np.zeros((-codes.size) % 4, np.uint8)]).reshape(-1, 4).astype(np.uint8)
    return (c[:, 0] << 6 | c[:, 1] << 4 | c[:, 2] << 2 | c[:, 3]).astype(np.uint8)


def final_lists(gpu, reads, l_pac, chunk_reads):
    """smem_batch_reg_finalize's results of every chunk, joined: (regs, out_off, sel, sel_idx, sel_off, status)"""
    import smemgpu
    from smemgpu.lib import FETCH_FIN
    opt = smemgpu.aln_opt()
    parts = []
    for a in range(0, reads.n, chunk_reads):
        n = min(chunk_reads, reads.n - a)
        o0, o1 = int(reads.offs[a]), int(reads.offs[a + n])
        b = gpu.batch(n, o1 - o0, int(reads.lens[a:a + n].max()))
        try:
            b.set_reads(reads.codes[o0:o1], reads.offs[a:a + n + 1] - reads.offs[a])
            b.run(smemgpu.Options())
            b.sa(19, 10000)
            b.chain(l_pac)
            b.chain2aln(opt)
            b.reg_finalize(ids=np.arange(a, a + n, dtype=np.int64))
            parts.append(b.fetch(FETCH_FIN).fin)
        finally:
            b.close()
    base = np.concatenate([[0], np.cumsum([f.regs.size for f in parts])]).astype(np.uint64)
    sbase = np.concatenate([[0], np.cumsum([f.sel_idx.size for f in parts])]).astype(np.uint64)
    out_off = np.concatenate([f.out_off[:-1] + base[i] for i, f in enumerate(parts)] + [base[-1:]])
    sel_off = np.concatenate([f.sel_off[:-1] + sbase[i] for i, f in enumerate(parts)] + [sbase[-1:]])
    return (np.concatenate([f.regs for f in parts]), out_off, np.concatenate([f.sel for f in parts]),
            np.concatenate([f.sel_idx + base[i] for i, f in enumerate(parts)]), sel_off,
            np.concatenate([f.status for f in parts]))


def printed(regs, out_off, fsel, sel_idx, sel_off, psel):
    """the regions every read prints and their smem_sam_rec_t, as tests/sampe_chain.library picks them"""
    from smemgpu.lib import SAM_REC_DT
    n = out_off.size - 1
    pr, e = np.arange(n) >> 1, np.arange(n) & 1
    br, st = psel["branch"][pr], psel["status"][pr]
    cnt = np.where(st != 0, 0, np.where(br == 0, (sel_off[1:] - sel_off[:-1]).astype(np.int64), 1))
    aln_off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64)
    read = np.repeat(np.arange(n), cnt)
    within = np.arange(read.size) - aln_off[read].astype(np.int64)
    b0 = br[read] == 0
    z = psel["z"][pr, e]
    k = np.where(b0, sel_idx[np.minimum(sel_off[read].astype(np.int64) + within, max(sel_idx.size - 1, 0))].astype(np.int64),
                 out_off[read].astype(np.int64) + z[read])
    pick = regs[k].copy()
    b1 = br[read] == 1
    pick["sub"][b1] = psel["sub"][pr, e][read][b1]
    rec = np.zeros(read.size, dtype=SAM_REC_DT)
    rec["mapq"] = np.where(b0, fsel["mapq"][k], psel["mapq"][pr, e][read])
    rec["flag"] = np.where(b0, fsel["flag"][k], 0)
    rec["score"] = pick["score"]
    rec["xs"] = np.where(b0, fsel["xs"][k], np.maximum(pick["sub"], pick["csub"]))
    return pick, rec, aln_off


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=500_000)
    ap.add_argument("--chunk", type=int, default=100_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--genome-bp", type=int, default=2_000_000)
    ap.add_argument("--repeat-frac", type=float, default=0.02)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--check", type=int, default=2000)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()

    import smemgpu
    from smemgpu import synth
    import samtext_ref as S
    from tests import samtext_pe_ref as R

    g = synth.make_genome(a.genome_bp, seed=1, repeat_frac=a.repeat_frac)
    idx, sa = smemgpu.Index.build_sa(g.codes, gpu=True, device=a.device)
    reads = synth.make_pairs(g.codes, a.pairs, a.read_len, seed=2)
    l_pac = int(g.codes.size)
    n = reads.n
    names = [f"r{i >> 1}" for i in range(n)]
    within = np.arange(reads.codes.size, dtype=np.int64) - np.repeat(reads.offs[:-1].astype(np.int64), reads.lens)
    quals = (33 + (7 * np.repeat(np.arange(n), reads.lens) + 3 * within) % 41).astype(np.uint8)
    gpu = smemgpu.Gpu(idx, device=a.device)
    try:
        gpu.load_sa(sa)
        gpu.load_pac(pack(g.codes), l_pac)
        gpu.load_contigs([0], [l_pac], l_pac)
        regs, out_off, fsel, sel_idx, sel_off, fstatus = final_lists(gpu, reads, l_pac, 2 * a.chunk)
        pes, _n_cand, _ms = gpu.pestat(regs, out_off, l_pac)
        psel, _ms = gpu.pair(regs, out_off, l_pac, pes)
        pick, rec, aln_off = printed(regs, out_off, fsel, sel_idx, sel_off, psel)
        alns, cigar, md, _ms = gpu.reg2aln(None, l_pac, reads.codes, reads.offs, pick, aln_off, smemgpu.aln_opt())
        alns = alns[:pick.size]
        rid = np.where(alns["status"] == 0, 0, -1).astype(np.int32)
        args = (reads.codes, reads.offs, names, quals, None, aln_off, alns, rid, rec, cigar, md, [0], ["ref"])
        pe = gpu.sam_text_pe(psel, *args, fin_status=fstatus)          # one untimed round of each
        se = gpu.sam_text(*args, fin_status=fstatus)
        t_pe, t_se = [], []
        for _ in range(a.runs):
            t_pe.append(gpu.sam_text_pe(psel, *args, fin_status=fstatus, text_cap=pe.text.size).kernel_ms)
            t_se.append(gpu.sam_text(*args, fin_status=fstatus, text_cap=se.text.size).kernel_ms)
    finally:
        gpu.close()
    # the first pairs against the restatement
    same = True
    for p in range(min(a.check, n // 2)):
        rd = []
        for r in (2 * p, 2 * p + 1):
            recs = []
            for k in range(int(aln_off[r]), int(aln_off[r + 1])):
                x, co, mo = alns[k], int(alns[k]["cigar_off"]), int(alns[k]["md_off"])
                recs.append(S.Rec(status=int(x["status"]), rid=int(rid[k]), pos=int(x["pos"]), is_rev=int(x["is_rev"]),
                                  cigar=tuple(int(w) for w in cigar[co:co + int(x["n_cigar"])]), NM=int(x["NM"]),
                                  md=md[mo:mo + int(x["md_len"])].tobytes().decode(), mapq=int(rec[k]["mapq"]),
                                  flag=int(rec[k]["flag"]), score=int(rec[k]["score"]), xs=int(rec[k]["xs"])))
            o = int(reads.offs[r])
            rd.append(dict(name=names[r], codes=reads.read(r), qual=quals[o:o + int(reads.lens[r])], comment="", recs=recs,
                           fin_status=int(fstatus[r])))
        s = psel[p]
        want = R.pair_text(rd, dict(status=int(s["status"]), branch=int(s["branch"]), proper=int(s["proper"]),
                                    mapq=s["mapq"].tolist()), ["ref"], [0])
        same &= [pe.read(2 * p), pe.read(2 * p + 1)] == (want or [b"", b""])
    med = lambda v: float(sorted(v)[len(v) // 2])   # noqa: E731
    lines_pe, lines_se = int((pe.text == 10).sum()), int((se.text == 10).sum())
    out = dict(pairs=a.pairs, read_len=a.read_len, genome_bp=a.genome_bp, repeat_frac=a.repeat_frac, regions=int(regs.size),
               records=int(pick.size), branches=[int((psel["branch"][psel["status"] == 0] == b).sum()) for b in range(3)],
               pairs_to_host_by_pairing=int((psel["status"] != 0).sum()),
               pe=dict(kernel_ms=t_pe, median_ms=med(t_pe), bytes=int(pe.text.size), lines=lines_pe,
                       host_reads=int((pe.status != 0).sum()), GBps=pe.text.size / (med(t_pe) * 1e-3) / 1e9,
                       ns_per_line=med(t_pe) * 1e6 / max(lines_pe, 1)),
               se=dict(kernel_ms=t_se, median_ms=med(t_se), bytes=int(se.text.size), lines=lines_se,
                       host_reads=int((se.status != 0).sum()), GBps=se.text.size / (med(t_se) * 1e-3) / 1e9,
                       ns_per_line=med(t_se) * 1e6 / max(lines_se, 1)),
               checked_pairs=min(a.check, n // 2), equals_restatement=bool(same))
    out["ms_per_GB_ratio_pe_over_se"] = (out["pe"]["median_ms"] / out["pe"]["bytes"]) / (out["se"]["median_ms"] / out["se"]["bytes"])
    line = json.dumps(out)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            fh.write(line + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
