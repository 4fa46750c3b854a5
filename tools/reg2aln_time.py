"""Time final regions -> alignments as a resident batch stage (smem_batch_reg2aln)
against the host round trip it replaces, on one device.

    python tools/reg2aln_time.py [--reads 98000] [--genome-bp 2000000] [--repeat-frac 0.02] [--json OUT]

The input of tools/regfin_time.py (a synthetic genome, 150-bp reads) goes through
the resident batch up to smem_batch_reg_finalize.  Then, in one process and
alternating `--runs` times:

  (a) the round trip: fetch(FETCH_FIN), the host gather regs[sel_idx], Gpu.reg2aln
      (smem_reg2aln: upload, kernels, download) -- wall time;
  (b) Batch.reg2aln() and fetch(FETCH_ALN) -- wall time.

Also reported: g2a_ms / g2a_prep_ms of (b) and smem_reg2aln's kernel_ms of (a) (the
DP kernels of the same regions; HIP events), the records, the CIGAR words and MD
bytes a record, and whether the two arms returned the same records.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "bwa-mem-harp2_amd"), ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def pack(codes):
    c = np.concatenate([codes, np.zeros((-codes.size) % 4, np.uint8)]).reshape(-1, 4).astype(np.uint8)
    return (c[:, 0] << 6 | c[:, 1] << 4 | c[:, 2] << 2 | c[:, 3]).astype(np.uint8)


def same_records(a, ac, am, b, bc, bm):
    """two results hold the same records: every field but the pool offsets, then the CIGAR
    words and MD bytes in record order"""
    for f in ("pos", "is_rev", "n_cigar", "NM", "score", "tries", "status", "md_len"):
        if not np.array_equal(a[f], b[f]):
            return False

    def gather(x, off, n):
        n = n.astype(np.int64)
        at = np.repeat(off.astype(np.int64) - np.concatenate([[0], np.cumsum(n)[:-1]]), n) + np.arange(int(n.sum()))
        return x[at]
    return np.array_equal(gather(ac, a["cigar_off"], a["n_cigar"]), gather(bc, b["cigar_off"], b["n_cigar"])) and \
        np.array_equal(gather(am, a["md_off"], a["md_len"]), gather(bm, b["md_off"], b["md_len"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=98_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--genome-bp", type=int, default=2_000_000)
    ap.add_argument("--repeat-frac", type=float, default=0.02)
    ap.add_argument("--sub", type=float, default=0.02)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()

    import smemgpu
    from smemgpu import synth
    from smemgpu.lib import FETCH_ALN, FETCH_FIN

    g = synth.make_genome(a.genome_bp, seed=1, repeat_frac=a.repeat_frac)
    idx, sa = smemgpu.Index.build_sa(g.codes, gpu=True, device=a.device)
    reads = synth.make_reads(g.codes, a.reads, a.read_len, seed=2, sub_rate=a.sub)
    l_pac = int(g.codes.size)
    gpu = smemgpu.Gpu(idx, device=a.device)
    out = dict(reads=reads.n, read_len=a.read_len, genome_bp=a.genome_bp, repeat_frac=a.repeat_frac)
    opt = smemgpu.aln_opt()
    try:
        gpu.load_sa(sa)
        gpu.load_pac(pack(g.codes), l_pac)
        gpu.load_contigs([0], [l_pac], l_pac)
        b = gpu.batch(reads.n, reads.codes.size, int(reads.lens.max()))
        b.set_reads(reads.codes, reads.offs)
        b.run(smemgpu.Options())
        b.sa(19, 10000)
        b.chain(l_pac)
        b.chain2aln(opt)
        b.reg_finalize()
        # one untimed round of each arm: buffers, pinned memory and code objects
        fin = b.fetch(FETCH_FIN).fin
        gpu.reg2aln(None, l_pac, reads.codes, reads.offs, fin.regs[fin.sel_idx.astype(np.int64)], fin.sel_off, opt)
        b.reg2aln(opt)
        b.fetch(FETCH_ALN)
        runs = []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            fin = b.fetch(FETCH_FIN).fin
            t1 = time.perf_counter()
            gathered = fin.regs[fin.sel_idx.astype(np.int64)]
            t2 = time.perf_counter()
            h_alns, h_cigar, h_md, h_ms = gpu.reg2aln(None, l_pac, reads.codes, reads.offs, gathered, fin.sel_off, opt)
            t3 = time.perf_counter()
            b.reg2aln(opt)
            t4 = time.perf_counter()
            res = b.fetch(FETCH_ALN).aln
            t5 = time.perf_counter()
            st = b.stats()
            runs.append(dict(a_wall_ms=(t3 - t0) * 1e3, a_fetch_fin_ms=(t1 - t0) * 1e3, a_gather_ms=(t2 - t1) * 1e3,
                             a_host_call_ms=(t3 - t2) * 1e3, a_kernel_ms=h_ms,
                             b_wall_ms=(t5 - t3) * 1e3, b_stage_ms=(t4 - t3) * 1e3, b_fetch_aln_ms=(t5 - t4) * 1e3,
                             g2a_ms=st["g2a_ms"], g2a_prep_ms=st["g2a_prep_ms"], passes=st["n_g2a_passes"]))
        same = same_records(h_alns, h_cigar, h_md, res.alns, res.cigar, res.md)
        b.close()
    finally:
        gpu.close()
    n_rec = int(res.alns.size)
    out.update(runs=runs, records=n_rec, final_regions=int(fin.regs.size), deferred=int(st["n_g2a_deferred"]),
               xref=int(st["n_g2a_xref"]), cigar_words_per_record=res.cigar.size / max(n_rec, 1),
               md_bytes_per_record=res.md.size / max(n_rec, 1),
               a_wall_ms_range=[min(r["a_wall_ms"] for r in runs), max(r["a_wall_ms"] for r in runs)],
               b_wall_ms_range=[min(r["b_wall_ms"] for r in runs), max(r["b_wall_ms"] for r in runs)],
               fetch_fin_bytes=16 * (reads.n + 1) + 4 * reads.n + (64 + 12) * int(fin.regs.size) + 8 * n_rec,
               fetch_aln_bytes=8 * (reads.n + 1) + (48 + 4) * n_rec + 4 * int(res.cigar.size) + int(res.md.size),
               arms_equal=bool(same))
    line = json.dumps(out)
    print(line)
    if a.json:
        with open(a.json, "w") as fh:
            fh.write(line + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
