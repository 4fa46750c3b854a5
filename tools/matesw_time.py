"""Time mate rescue's two entry points on one device.

    python tools/matesw_time.py [--problems 50000] [--pairs 50000] [--genome-bp 2000000] [--json OUT]

1. smem_ksw_align2_long on `--problems` rescue-shaped problems -- a 150 bp read with 2 %
   substitutions against the 650 bp window that holds it, every second problem
   reverse-complemented, mem_matesw's xtra -- in cells per second (qlen x tlen per problem: the
   start pass's cells are not counted, on either side), beside smem_ksw_align2 on the same
   queries against the 256 bp of each window around the hit, in the same session.  The short
   routine on the same queries is the yardstick.
2. smem_matesw on `--pairs` pairs of the recipe of tests/golden/make_golden_msw.py scaled up: 80 %
   ordinary pairs (150 bp, insert N(500, 50), 2 % substitutions) and 20 % whose second mate has a
   substitution at every tenth base, hence no region of its own.  The regions come from the
   resident batch (seeding .. smem_batch_reg_finalize: the lists after mem_mark_primary_se, which
   hold the regions of mem_sort_and_dedup in another order with the marks set), the bounds are
   FR (269, 717), what the reference inferred from this insert distribution (tests/golden/msw).
   Reported: kernel ms (HIP events), wall ms of the call, the share of pairs the pre-pass settles
   without an SW, SWs run, pairs left to the host.
`--runs` timed runs of each after one untimed round.
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

XBYTE, XSUBO, XSTART = 0x10000, 0x40000, 0x80000


def pack(codes):
    c = np.concatenate([codes, np.zeros((-codes.size) % 4, np.uint8)]).reshape(-1, 4).astype(np.uint8)
    return (c[:, 0] << 6 | c[:, 1] << 4 | c[:, 2] << 2 | c[:, 3]).astype(np.uint8)


def sw_problems(G, n, qlen, wlen, seed):
    """(long batch, short batch): the same queries against wlen-bp windows and against 256 bp of them"""
    from smemgpu import synth
    rng = np.random.default_rng(seed)
    pos = rng.integers(0, G.size - wlen, size=n)
    at = rng.integers(0, wlen - qlen + 1, size=n)
    ar = np.arange(wlen)[None, :]
    T = G[pos[:, None] + ar]
    Q = np.take_along_axis(T, at[:, None] + np.arange(qlen)[None, :], axis=1).copy()
    hit = rng.random(Q.shape) < 0.02
    Q[hit] = (Q[hit] + rng.integers(1, 4, size=int(hit.sum()))) & 3
    lo = np.clip(at - (256 - qlen) // 2, 0, wlen - 256)
    S = np.take_along_axis(T, lo[:, None] + np.arange(256)[None, :], axis=1).copy()
    rev = np.arange(n) % 2 == 1
    Q[rev], T[rev], S[rev] = (3 - Q[rev])[:, ::-1], (3 - T[rev])[:, ::-1], (3 - S[rev])[:, ::-1]
    xtra = XSUBO | XSTART | (XBYTE if qlen < 250 else 0) | 19

    def batch(t, tl):
        tasks = np.zeros(n, dtype=synth.KSWA_TASK)
        tasks["q_off"], tasks["t_off"] = np.arange(n) * qlen, np.arange(n) * tl
        tasks["qlen"], tasks["tlen"], tasks["xtra"] = qlen, tl, xtra
        return synth.KswBatch(tasks, Q.reshape(-1).astype(np.uint8), t.reshape(-1).astype(np.uint8), synth.bwa_scmat())
    return batch(T, wlen), batch(S, 256)


def pair_reads(G, n_pairs, seed):
    from smemgpu import synth
    n_hard = n_pairs // 5
    plain = synth.make_pairs(G, n_pairs - n_hard, 150, seed=seed, sub_rate=0.02, n_rate=0.0)
    hard = synth.make_pairs(G, n_hard, 150, seed=seed + 1, sub_rate=0.0, n_rate=0.0)
    codes = hard.codes.copy().reshape(-1, 150)
    rng = np.random.default_rng(seed + 2)
    at = np.arange(5, 150, 10)
    codes[1::2][:, at] = (codes[1::2][:, at] + rng.integers(1, 4, size=(codes.shape[0] // 2, at.size))) & 3
    hard = synth.Reads(hard.lens, codes.reshape(-1).astype(np.uint8), hard.offs)
    return synth.concat_reads([plain, hard])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=50_000)
    ap.add_argument("--pairs", type=int, default=50_000)
    ap.add_argument("--genome-bp", type=int, default=2_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()

    import smemgpu
    from smemgpu import synth
    from smemgpu.lib import FETCH_FIN

    g = synth.make_genome(a.genome_bp, seed=1)
    G = g.codes
    l_pac = int(G.size)
    idx, sa = smemgpu.Index.build_sa(G, gpu=True, device=a.device)
    gpu = smemgpu.Gpu(idx, device=a.device)
    out = dict(problems=a.problems, pairs=a.pairs, genome_bp=a.genome_bp)
    try:
        long_b, short_b = sw_problems(G, a.problems, 150, 650, seed=3)
        r_long, _ = gpu.ksw_align2_long(long_b)     # untimed round
        r_short, _ = gpu.ksw_align2(short_b)
        ms_long = [gpu.ksw_align2_long(long_b)[1] for _ in range(a.runs)]
        ms_short = [gpu.ksw_align2(short_b)[1] for _ in range(a.runs)]
        ms_long256 = [gpu.ksw_align2_long(short_b)[1] for _ in range(a.runs)]
        cells_long, cells_short = a.problems * 150 * 650, a.problems * 150 * 256
        out["sw"] = dict(qlen=150, tlen_long=650, tlen_short=256, long_ms=ms_long, short_ms=ms_short,
                         long_on_256_ms=ms_long256,
                         long_gcups=cells_long / (min(ms_long) * 1e-3) / 1e9,
                         short_gcups=cells_short / (min(ms_short) * 1e-3) / 1e9,
                         long_on_256_gcups=cells_short / (min(ms_long256) * 1e-3) / 1e9,
                         same_score=float((r_long["score"] == r_short["score"]).mean()),
                         start_pass_share=float((r_long["tb"] >= 0).mean()))

        reads = pair_reads(G, a.pairs, seed=5)
        gpu.load_sa(sa)
        gpu.load_pac(pack(G), l_pac)
        b = gpu.batch(reads.n, reads.codes.size, int(reads.lens.max()))
        b.set_reads(reads.codes, reads.offs)
        b.run(smemgpu.Options())
        b.sa(19, 10000)
        b.chain(l_pac)
        b.chain2aln(smemgpu.aln_opt())
        b.reg_finalize()
        fin = b.fetch(FETCH_FIN).fin
        b.close()
        pes = [(0, 0, 1), (269, 717, 0), (0, 0, 1), (0, 0, 1)]
        args = (None, l_pac, reads.codes, reads.offs, fin.regs, fin.out_off, pes)
        res = gpu.matesw(*args)                     # untimed round (it also sizes the output)
        cap = int(res[1][-1])
        runs = []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            res = gpu.matesw(*args, regs_cap=cap)
            runs.append(dict(wall_ms=(time.perf_counter() - t0) * 1e3, kernel_ms=res[4]))
        n_sw, status = res[2], res[3]
        none = np.diff(fin.out_off.astype(np.int64)) == 0
        out["matesw"] = dict(runs=runs, regions_in=int(fin.regs.size), regions_out=cap,
                             reads_without_region=int(none.sum()),
                             reads_without_region_after=int((np.diff(res[1].astype(np.int64)) == 0).sum()),
                             pairs_without_sw_share=float((n_sw == 0).mean()), sw_total=int(n_sw.sum()),
                             pairs_left_to_host=int((status != 0).sum()),
                             kernel_ms_best=min(r["kernel_ms"] for r in runs),
                             wall_ms_best=min(r["wall_ms"] for r in runs))
    finally:
        gpu.close()
    line = json.dumps(out)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
