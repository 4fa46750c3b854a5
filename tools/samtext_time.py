"""Time alignments -> SAM text as a resident batch stage (smem_batch_sam), on one device.

    python tools/samtext_time.py [--reads 98000] [--genome-bp 2000000] [--repeat-frac 0.02] [--json OUT]

The input of tools/reg2aln_time.py (a synthetic genome, 150-bp reads) goes through the
resident batch up to smem_batch_reg2aln, with names r<i> and qualities 33 + (7 i + 3 r) % 41.
Then `--runs` times after one untimed round: Batch.sam() and fetch(FETCH_SAM), and
fetch(FETCH_ALN) beside it for scale.

Reported per run: sam_ms and sam_write_ms (HIP events), the wall time of the stage, of each
fetch through the binding (which copies the result out of pinned memory) and of the library's
own copy (smem_batch_fetch_mask alone); once: the text's bytes, bytes a record, reads left to
the host, the write pass's achieved GB/s (bytes written / sam_write_ms), the bytes each fetch
copies, g2a_ms of the same batch, and whether the text equals tests/samtext_ref.py's for the
first `--check` reads.
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


def restated(reads, names, quals, res, n_check):
    """tests/samtext_ref.py over the fetched alignments of the first n_check reads"""
    import samtext_ref as S
    fin, aln = res.fin, res.aln
    out = []
    for r in range(n_check):
        recs = []
        for k in range(int(aln.aln_off[r]), int(aln.aln_off[r + 1])):
            a, j = aln.alns[k], int(fin.sel_idx[k])
            s = fin.sel[j]
            co, mo = int(a["cigar_off"]), int(a["md_off"])
            recs.append(S.Rec(status=int(a["status"]), rid=int(aln.rid[k]), pos=int(a["pos"]), is_rev=int(a["is_rev"]),
                              cigar=tuple(int(w) for w in aln.cigar[co:co + int(a["n_cigar"])]), NM=int(a["NM"]),
                              md=aln.md[mo:mo + int(a["md_len"])].tobytes().decode(), mapq=int(s["mapq"]),
                              flag=int(s["flag"]), score=int(fin.regs[j]["score"]), xs=int(s["xs"])))
        o = int(reads.offs[r])
        out.append(S.read_text(names[r], reads.read(r), quals[o:o + int(reads.lens[r])], None, ["ref"], [0], recs,
                               fin_status=int(fin.status[r])))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=98_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--genome-bp", type=int, default=2_000_000)
    ap.add_argument("--repeat-frac", type=float, default=0.02)
    ap.add_argument("--sub", type=float, default=0.02)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--check", type=int, default=2000)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()

    import smemgpu
    from smemgpu import synth
    from smemgpu.lib import FETCH_ALN, FETCH_FIN, FETCH_SAM

    g = synth.make_genome(a.genome_bp, seed=1, repeat_frac=a.repeat_frac)
    idx, sa = smemgpu.Index.build_sa(g.codes, gpu=True, device=a.device)
    reads = synth.make_reads(g.codes, a.reads, a.read_len, seed=2, sub_rate=a.sub)
    l_pac = int(g.codes.size)
    names = [f"r{i}" for i in range(reads.n)]
    within = np.arange(reads.codes.size, dtype=np.int64) - np.repeat(reads.offs[:-1].astype(np.int64), reads.lens)
    quals = (33 + (7 * np.repeat(np.arange(reads.n), reads.lens) + 3 * within) % 41).astype(np.uint8)
    gpu = smemgpu.Gpu(idx, device=a.device)
    lib = smemgpu.load()
    out = dict(reads=reads.n, read_len=a.read_len, genome_bp=a.genome_bp, repeat_frac=a.repeat_frac)
    opt = smemgpu.aln_opt()
    try:
        gpu.load_sa(sa)
        gpu.load_pac(pack(g.codes), l_pac)
        gpu.load_contigs([0], [l_pac], l_pac)
        gpu.load_contig_names(["ref"])
        b = gpu.batch(reads.n, reads.codes.size, int(reads.lens.max()))
        b.set_reads(reads.codes, reads.offs)
        b.set_read_text(names, quals)
        b.run(smemgpu.Options())
        b.sa(19, 10000)
        b.chain(l_pac)
        b.chain2aln(opt)
        b.reg_finalize()
        b.reg2aln(opt)
        b.sam()                                   # one untimed round: buffers, pinned memory, code objects
        b.fetch(FETCH_SAM)
        b.fetch(FETCH_ALN)
        runs = []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            b.sam()
            t1 = time.perf_counter()
            sam = b.fetch(FETCH_SAM).sam
            t2 = time.perf_counter()
            b.fetch(FETCH_ALN)
            t3 = time.perf_counter()
            # the library's copies alone (device -> pinned host memory), without the binding's copy out of it
            assert lib.smem_batch_fetch_mask(b._h, FETCH_SAM) == 0
            t4 = time.perf_counter()
            assert lib.smem_batch_fetch_mask(b._h, FETCH_ALN) == 0
            t5 = time.perf_counter()
            st = b.stats()
            runs.append(dict(sam_ms=st["sam_ms"], sam_write_ms=st["sam_write_ms"], stage_wall_ms=(t1 - t0) * 1e3,
                             fetch_sam_ms=(t2 - t1) * 1e3, fetch_aln_ms=(t3 - t2) * 1e3,
                             fetch_sam_copy_ms=(t4 - t3) * 1e3, fetch_aln_copy_ms=(t5 - t4) * 1e3))
        res = b.fetch(FETCH_ALN | FETCH_FIN)
        n_check = min(a.check, reads.n)
        want = restated(reads, names, quals, res, n_check)
        same = all(sam.read(r) == (w or b"") for r, w in enumerate(want))
        b.close()
    finally:
        gpu.close()
    n_rec, nb = int(res.aln.alns.size), int(st["n_sam_bytes"])
    wr = sorted(r["sam_write_ms"] for r in runs)[len(runs) // 2]
    out.update(runs=runs, records=n_rec, sam_bytes=nb, bytes_per_record=nb / max(n_rec, 1), host_reads=int(st["n_sam_host"]),
               g2a_ms=st["g2a_ms"], sam_ms_range=[min(r["sam_ms"] for r in runs), max(r["sam_ms"] for r in runs)],
               write_GBps=nb / (wr * 1e-3) / 1e9 if wr > 0 else None,
               fetch_sam_bytes=nb + 8 * (reads.n + 1) + 4 * reads.n,
               fetch_aln_bytes=8 * (reads.n + 1) + (48 + 4) * n_rec + 4 * int(res.aln.cigar.size) + int(res.aln.md.size),
               fetch_sam_ms_range=[min(r["fetch_sam_ms"] for r in runs), max(r["fetch_sam_ms"] for r in runs)],
               fetch_aln_ms_range=[min(r["fetch_aln_ms"] for r in runs), max(r["fetch_aln_ms"] for r in runs)],
               fetch_sam_copy_ms_range=[min(r["fetch_sam_copy_ms"] for r in runs), max(r["fetch_sam_copy_ms"] for r in runs)],
               fetch_aln_copy_ms_range=[min(r["fetch_aln_copy_ms"] for r in runs), max(r["fetch_aln_copy_ms"] for r in runs)],
               checked_reads=n_check, equals_restatement=bool(same))
    line = json.dumps(out)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            fh.write(line + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
