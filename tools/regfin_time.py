"""Time raw regions -> final regions (smem_batch_reg_finalize) on one device.

    python tools/regfin_time.py [--reads 98000] [--genome-bp 2000000] [--repeat-frac 0.02] [--json OUT]

A synthetic genome and 150-bp reads go through the resident batch (seeding, SA,
chains, smem_batch_chain2aln); the stage then runs `--runs` times over the
regions left in HBM.  Reported: its kernel time (HIP events, copies outside)
with the split between the lane and the wave tier, aln_ms of the same batch,
the raw -> final region counts, and the bytes a SMEM_FETCH_FIN fetch moves
against SMEM_FETCH_REGS.  `--check N` compares N reads with the Python
restatement (tests/regfin_ref.py).
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=98_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--genome-bp", type=int, default=2_000_000)
    ap.add_argument("--repeat-frac", type=float, default=0.02)
    ap.add_argument("--sub", type=float, default=0.02)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--check", type=int, default=300)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()

    import smemgpu
    from smemgpu import synth
    from smemgpu.lib import ALNREG_DT, FETCH_FIN, FETCH_REGS

    g = synth.make_genome(a.genome_bp, seed=1, repeat_frac=a.repeat_frac)
    idx, sa = smemgpu.Index.build_sa(g.codes, gpu=True, device=a.device)
    reads = synth.make_reads(g.codes, a.reads, a.read_len, seed=2, sub_rate=a.sub)
    l_pac = int(g.codes.size)
    gpu = smemgpu.Gpu(idx, device=a.device)
    out = dict(reads=reads.n, read_len=a.read_len, genome_bp=a.genome_bp, repeat_frac=a.repeat_frac)
    try:
        gpu.load_sa(sa)
        gpu.load_pac(pack(g.codes), l_pac)
        b = gpu.batch(reads.n, reads.codes.size, int(reads.lens.max()))
        b.set_reads(reads.codes, reads.offs)
        b.run(smemgpu.Options())
        b.sa(19, 10000)
        b.chain(l_pac)
        b.chain2aln(smemgpu.aln_opt())
        runs = []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            b.reg_finalize()
            wall = time.perf_counter() - t0
            st = b.stats()
            runs.append(dict(fin_ms=st["fin_ms"], lane_ms=st["fin_lane_ms"], wave_ms=st["fin_wave_ms"],
                             call_wall_ms=wall * 1e3))
        st = b.stats()
        raw = b.fetch(FETCH_REGS)
        fin = b.fetch(FETCH_FIN).fin
        b.close()
    finally:
        gpu.close()
    n, n_raw, n_fin, n_sel = reads.n, int(raw.reg_off[-1]), fin.regs.size, fin.sel_idx.size
    per_read = np.diff(raw.reg_off.astype(np.int64))
    out.update(runs=runs, aln_ms=st["aln_ms"], raw_regions=n_raw, final_regions=n_fin, records=n_sel,
               reads_lane_tier=int((per_read <= 16).sum()), reads_wave_tier=int((per_read > 16).sum()),
               max_regions_of_a_read=int(per_read.max()), rejected=int(fin.status.sum()),
               fetch_regs_bytes=8 * (n + 1) + 64 * n_raw,
               fetch_fin_bytes=16 * (n + 1) + 4 * n + (64 + 12) * n_fin + 8 * n_sel)
    if a.check:
        import regfin_data as D
        import regfin_ref as ref
        pick = np.sort(np.random.default_rng(3).choice(n, size=min(a.check, n), replace=False))
        big = np.argsort(per_read)[-8:]                      # and the reads with the most regions
        pick = np.unique(np.concatenate([pick, big]))
        regs = np.frombuffer(raw.regs.tobytes(), dtype=ALNREG_DT)
        bad = 0
        for r in pick:
            lo, hi = int(raw.reg_off[r]), int(raw.reg_off[r + 1])
            w = D.restate(ref.Opt(), regs[lo:hi], np.array([0, hi - lo], dtype=np.uint64),
                          reads.lens[r:r + 1].astype(np.int32), np.array([r]))
            o0, o1 = int(fin.out_off[r]), int(fin.out_off[r + 1])
            same = o1 - o0 == w["regs"].size and fin.regs[o0:o1].tobytes() == w["regs"].tobytes() and \
                np.array_equal(np.stack([fin.sel[f][o0:o1] for f in ("mapq", "flag", "xs")], axis=1).reshape(-1, 3),
                               w["sel"])
            bad += not same
        out.update(checked_reads=int(pick.size), checked_bad=int(bad))
    line = json.dumps(out)
    print(line)
    if a.json:
        with open(a.json, "w") as fh:
            fh.write(line + "\n")
    return 1 if out.get("checked_bad") else 0


if __name__ == "__main__":
    sys.exit(main())
