"""SMEM-seeding benchmark (BASELINE.json metric) on 1..N MI355X.

    python bench.py [--gpus N --steps K --warmup W] [--config c2|c3|c4|c5] [--genome-profile uniform|human]
                    [--dump-outputs DIR] [--full]
    torchrun --nproc-per-node N bench.py --gpus N ...   (one rank per GPU)

A plain run does what the headline needs and no more: it builds or loads the
index, puts the reads in HBM, warms up, times K steps, writes the last step's
outputs when --dump-outputs names a directory (dump_outputs below), and prints
one JSON line: metric, value, unit, ms_per_step (wall milliseconds per timed
step), the workload and the kernel's own times.  Everything else described
here -- `streaming`, `roofline`, `cpu_baseline`, `parity_sample`, the sa /
chain / alignment / sw stages, `e2e` and the other genome profile -- runs only
with --full, after the headline and never inside its timed region, and is
added to the same line.

Workload (BASELINE.json configs[1], the default --config c2): an FM index
resident in HBM and 1M x 150 bp single-end reads per GPU (2% substitutions,
0.1% N, both strands).  human_g1k_v37 is not available offline, so the index
is built from a seeded synthetic genome of its size by this repo's own
`bwa index -a is`-identical builder; its size is in `config`.  The headline
(--genome-profile human, the default since round 5) uses the human-like
profile of smemgpu/synth.py -- ~46 % interspersed repeats shaped like
RepeatMasker's classes plus 3 % satellites, the closer stand-in -- and the
line carries the same step on the uniform profile (random sequence with 2 %
repeat families, exact and tandem repeats: rounds 1-4's headline) beside it
(`uniform`).

A step = one pass of the seeding hot path (mem_insert_seed's smem_next2 loop
for every read, software/bwamem.c:453-460) over the resident batch: the
seeding kernel plus result compaction, outputs left in HBM.  As the
reference's kt_for_batch workers do, --streams host workers (default 2) each
own a batch (all the reads) and a HIP stream and run whole steps dealt
round-robin, so one step's tail overlaps the next step's start; K steps are
timed in total.  Reads shard across ranks with no collective in the data path
(index replicated): the read stream is cut into blocks of 256k reads dealt
round-robin to the ranks; scaling "weak".

`streaming`: the same path with host buffers -- bwa mem's chunk loop through
smem_gpu_seed_stream (chunks staged into pinned memory, H2D, seeding, D2H of
every interval into pinned memory, several workers overlapping) -- reported
beside `value`, never as it.  --config c3/c4/c5 stream the north_star's
target sizes (12.5M pairs = one GPU's shard of C3's 100M pairs, 10M x 250 bp,
10M x 150 bp at 5 %; c2 streams 4M); `value` stays the device-resident rate
on a 1M-read batch of the same reads.

roofline: dominant kernel = seed_wp_kernel (seed_kernel for variants < 40).  achieved = algorithmic bytes per
launch (64 B x distinct Occ buckets per extend + read length
+ 32 B x intervals out, counted by the CPU oracle on a sample of the same
reads) / the kernel's HIP-event duration measured here; frac_occ64 does the
same with the 32-B buckets this build actually reads.  The kernel is bound by
random-request rate, not bytes: request_roofline compares its L2 fabric read
requests per second (rocprofv3 TCC_EA0_RDREQ recorded by tools/traffic.py for
this build and workload) with the random-gather ceiling measured on this GPU
(tools/gather_ceiling.hip, profiles/gather_ceiling.json); sq_counters gives
the same kernel's VALU / SALU instructions per extend and its issue / wait
shares (SQ_* counters of the same tools/traffic.py run).

cpu_baseline: the reference's own C (oracle/_ref/ref_harness, compiled from
the reference sources) when present, else the C restatement, timed on this
host's physical cores on a bounded sample of the same reads, rank 0 only.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "bwa-mem-harp2_amd"))
sys.path.insert(0, ROOT)

METRIC = "SMEM reads/sec on human_g1k_v37 150bp at 1/2/4/8 MI355X; achieved HBM GB/s"
RT_TICKS_PER_MS = 1e5  # s_memrealtime: 100 MHz (checked against HIP events: chip_clock_check)
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md chip-level parameters (spec)
HUMAN_MBP = 3101.804739  # human_g1k_v37 l_pac
# VALU int32 peak (MI355X_MICROARCH.md: 256 CUs x 4 SIMDs x 32 lanes/clock x 2.4 GHz) and the DP stages' cell
# ceiling at 8 int32 ops per affine-gap cell (H = max(diag + score, E, F); E', F' = max(. - e, H - o - e); 0 floor)
VALU_INT32_OPS = 256 * 4 * 32 * 2.4e9
OPS_PER_CELL = 8
BLOCK = 1 << 18          # reads per block of the read stream (shards are whole blocks)

# BASELINE.json configs: per-GPU shapes
CONFIGS = {
    "c2": dict(read_len=150, sub=0.02, k=19, pairs=False, stream_reads=16_000_000,
               what="human_g1k_v37-sized index in HBM, 1M x 150 bp SE (BASELINE configs[1]); 16M streamed"),
    "c3": dict(read_len=150, sub=0.02, k=19, pairs=True, stream_reads=25_000_000,
               what="C3 on one GPU: its shard of 100M x 150 bp PE on 8 GPUs = 12.5M pairs, insert N(500, 50), "
                    "mates interleaved in one chunk"),
    # c4 / c5 stream in 256k-read chunks with 8 workers: their reads carry ~1.7x the intervals of
    # c2's, and a chunk's pinned results fetch slower the larger they are (2M-read chunks, 1.7 GB:
    # 10-15 GB/s; profiles/r06/stream/: 2M 15.8-18.3, 1M 23.3-32.5, 512k 25.1-33.5, 256k
    # 30.5-32.5 M reads/s at c5 over repeated sweeps -- the 256k chunks the steadiest)
    "c4": dict(read_len=250, sub=0.02, k=19, pairs=False, stream_reads=10_000_000, stream_chunk=1 << 18,
               stream_workers=8, what="C4: 10M x 250 bp, min-seed-len 19 with re-seeding"),
    "c5": dict(read_len=150, sub=0.05, k=19, pairs=False, stream_reads=10_000_000, stream_chunk=1 << 18,
               stream_workers=8, what="C5: 10M x 150 bp at 5 % substitutions"),
}


T_START = time.time()


def log(*a):
    print(f"[bench {time.time() - T_START:6.1f}s]", *a, file=sys.stderr, flush=True)


def parse(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--full", action="store_true",
                   help="after the headline, also run and report everything else: roofline and parity sample (CPU "
                        "oracle), CPU baselines, streaming, the sa / chain / alignment / sw stages, bwa mem end to end "
                        "against the reference, the other genome profile")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="write what the last timed step computed (the arrays Batch.fetch() returns: interval lists "
                        "and smem_next2 call counts) as DIR/<name>.npy in float64 / float32, at most 64 MB: per-read "
                        "counts of every read and the full lists of a fixed seeded sample of reads")
    p.add_argument("--config", choices=sorted(CONFIGS), default="c2")
    p.add_argument("--reads", type=int, default=1_000_000, help="resident reads per GPU (the metric's batch)")
    p.add_argument("--read-len", type=int, default=None)
    p.add_argument("--sub", type=float, default=None)
    p.add_argument("--genome-mbp", type=float, default=HUMAN_MBP,
                   help="synthetic genome size; default = human_g1k_v37 l_pac (6.2 G symbols with its reverse complement)")
    p.add_argument("--genome-profile", choices=["uniform", "human"], default="human",
                   help="human (the headline): ~46 %% interspersed repeats + satellites, the closer stand-in for "
                        "human_g1k_v37; uniform: random + 2 %% repeat families")
    p.add_argument("--seed", type=int, default=1)
    p.add_argument("--builder", choices=["gpu", "cpu"], default="gpu", help="index construction (same bytes)")
    p.add_argument("--lanes-per-cu", type=int, default=0)
    p.add_argument("--variant", type=int, default=0, help="seeding kernel variant (smem_gpu_set_kernel_variant)")
    p.add_argument("--kmer-k", type=int, default=0, help="k-mer bi-interval table of 1..K bases (variant 23)")
    p.add_argument("--streams", type=int, default=2, help="host workers, each with its own batch and HIP stream")
    p.add_argument("--stream-reads", type=int, default=None,
                   help="reads per GPU pushed through the streaming path (default: the config's; 0: the resident "
                        "reads; -1: no streaming leg)")
    p.add_argument("--stream-chunk", type=int, default=None,
                   help="reads per streamed chunk (default: the config's; c2 / c3 2M: 0.93 of the resident rate vs "
                        "0.86-0.88 at 1M, profiles/r04/stream; c4 / c5 1M)")
    p.add_argument("--stream-workers", type=int, default=None, help="streaming workers (default: the config's, 3 or 4)")
    p.add_argument("--stream-packed", type=int, default=1, help="1: 16-B wire entries (SMEM_STREAM_PACKED)")
    p.add_argument("--stream-passes", type=int, default=3, help="timed streaming passes; the median is reported")
    p.add_argument("--side-stages", type=int, default=1, help="0: skip the sa / chain / sw side reports")
    p.add_argument("--cpu-seconds", type=float, default=15.0, help="CPU baseline budget (0 = skip)")
    p.add_argument("--stats-sample", type=int, default=20000, help="reads counted by the oracle for bytes/read")
    p.add_argument("--parity", type=int, default=1,
                   help="1: seed the stats sample on the GPU too and compare (0: every seed_kernel launch is a "
                        "full resident batch, for rocprofv3 summaries)")
    p.add_argument("--e2e-reads", type=int, default=1_000_000,
                   help="reads of the end-to-end leg (bwa-gpu mem vs the reference pipeline; 0: skip; N=1 only)")
    p.add_argument("--e2e-pairs", type=int, default=250_000,
                   help="e2e: also this many interleaved pairs through bwa-gpu mem -p vs the reference (0: skip)")
    p.add_argument("--e2e-batch", type=int, default=0,
                   help="-b of bwa-gpu mem (0: none -- the binding's own per-device batch plan, the product default)")
    p.add_argument("--e2e-chunk-reads", type=int, default=3_200_000,
                   help="e2e.multi_chunk: this many SE reads (several bwa mem chunks of 10 Mbp x threads; 0: off)")
    p.add_argument("--other-profile", "--human-like", dest="other_profile", type=int, default=1,
                   help="1: also measure the seeding step on the other genome profile (uniform beside the human-like "
                        "headline; N=1 only)")
    p.add_argument("--cache", default=os.path.join(tempfile.gettempdir(), "smem_bench_cache"))
    p.add_argument("--traffic-json", default=None,
                   help="per-launch counters recorded by tools/traffic.py for this build + workload (default: "
                        "profiles/traffic.json, or profiles/traffic_human.json for the human-like profile)")
    p.add_argument("--ceiling-json", default=os.path.join(ROOT, "profiles", "gather_ceiling.json"))
    a = p.parse_args(argv)
    if a.steps < 1:
        p.error("--steps must be at least 1")
    cfg = CONFIGS[a.config]
    a.read_len = a.read_len or cfg["read_len"]
    a.sub = cfg["sub"] if a.sub is None else a.sub
    a.min_seed_len = cfg["k"]
    a.pairs = cfg["pairs"]
    if a.stream_reads is None:
        a.stream_reads = cfg["stream_reads"]
    if a.stream_chunk is None:
        a.stream_chunk = cfg.get("stream_chunk", 1 << 21)
    if a.stream_workers is None:
        a.stream_workers = cfg.get("stream_workers", 3)
    if a.traffic_json is None:
        a.traffic_json = traffic_path(a.genome_profile)
    return a


def traffic_path(profile: str) -> str:
    return os.path.join(ROOT, "profiles", "traffic_human.json" if profile == "human" else "traffic.json")


def kernel_name(variant: int) -> str:
    return "seed_wp_kernel" if variant >= 40 else "seed_kernel"


def genome_key(args) -> str:
    n_bp = int(args.genome_mbp * 1e6)
    prof = "" if args.genome_profile == "uniform" else "_human"
    return os.path.join(args.cache, f"genome_{n_bp}_{args.seed}{prof}")


def make_genome(args):
    from smemgpu import synth
    n_bp = int(args.genome_mbp * 1e6)
    if args.genome_profile == "human":
        return synth.make_genome_human_like(n_bp, seed=args.seed, n_chrom=24)
    return synth.make_genome(n_bp, seed=args.seed, n_chrom=24)


def get_index(args, rank, barrier, device=0, need_sa=True):
    """Index (+ .sa) and the genome codes, built once per host by rank 0 and
    cached; every rank then reads them (the genome through a memory map, so
    no rank regenerates it).  need_sa=False: the .sa is neither required in
    the cache nor read (None is returned in its place)."""
    import smemgpu
    os.makedirs(args.cache, exist_ok=True)
    base = genome_key(args)
    key, skey, gkey = base + ".bwt", base + ".sa", base + ".codes"
    built = None
    if rank == 0 and not all(os.path.exists(k) for k in ((key, skey, gkey) if need_sa else (key, gkey))):
        t = time.time()
        g = make_genome(args)
        t_g = time.time()
        idx, sa = smemgpu.Index.build_sa(g.codes, sa_intv=32, gpu=args.builder == "gpu", device=device)
        t_b = time.time()
        idx.write(key + ".tmp")
        sa.write(skey + ".tmp")
        g.codes.tofile(gkey + ".tmp")
        for k in (key, skey, gkey):
            os.replace(k + ".tmp", k)
        del g
        built = (idx, sa)
        log(f"index built ({args.builder}, {args.genome_profile}): {idx.words.nbytes / 1e6:.1f} MB .bwt + "
            f"{sa.samples.nbytes / 1e6:.1f} MB .sa in {time.time() - t:.1f} s (genome {t_g - t:.1f}, build "
            f"{t_b - t_g:.1f}, cache files {time.time() - t_b:.1f})")
    barrier()
    codes = np.memmap(gkey, dtype=np.uint8, mode="r")
    if built:   # the same bytes as the files just written
        return built[0], key, built[1] if need_sa else None, codes
    return smemgpu.Index.read(key), key, smemgpu.SA.read(skey) if need_sa else None, codes


def shard_blocks(n_reads: int, rank: int, world: int, block: int = BLOCK) -> list:
    """The blocks of the read stream rank `rank` seeds: ceil(n_reads / block)
    blocks per rank, dealt round-robin (block b goes to rank b % world)."""
    per = (n_reads + block - 1) // block
    return [rank + world * k for k in range(per)]


def make_reads(args, rank, genome_codes, world: int = 1, n_reads: int | None = None, salt: int = 0):
    """This rank's shard of the read stream: n_reads (default --reads) reads
    in whole blocks (the last one cut), blocks dealt round-robin over the
    ranks, so the shards reassembled in block order are the single-rank
    stream of the same total."""
    from smemgpu import synth
    n = args.reads if n_reads is None else n_reads
    block = getattr(args, "block", BLOCK)
    blocks = shard_blocks(n, rank, world, block)
    kw = dict(sub_rate=args.sub, n_rate=0.001)
    r = synth.make_read_blocks(np.asarray(genome_codes), blocks, block, args.read_len,
                               seed=1000 + args.seed * 7919 + salt, pairs=bool(getattr(args, "pairs", False)), **kw)
    if r.n > n:   # the first n reads (what r.subset(np.arange(n)) holds, without its pass over every read)
        r = synth.Reads(r.lens[:n].copy(), r.codes[:int(r.offs[n])].copy(), r.offs[:n + 1].astype(np.int64))
    return r


def cpu_leg(args, gpu, opt, idx, idx_path, reads, cores, sw_tasks=None):
    """The CPU leg of the bench (rank 0 only) -- the one place bench.py runs
    anything under oracle/, as the checker and the CPU baseline, never in the
    measured path:
      * SURVEY.md §8(d) algorithmic bytes/read, counted by the restatement on
        a sample of the benchmark's own reads (64 B per distinct
        reference-layout Occ bucket of each bwt_extend + read + 32 B per
        interval), and the same over the 32-B Occ64 buckets this build reads;
      * parity of that sample at full index size: the GPU's smem_next2 lists
        for those reads == the restatement's, bit for bit;
      * the CPU baseline: the compiled reference (oracle/_ref) -- or the
        restatement when it is absent -- timed on a bounded prefix of the
        same reads;
      * with sw_tasks, the SW stage's CPU baseline (sw_cpu)."""
    from oracle import oracle
    from smemgpu import synth
    oi = oracle.OracleIndex(words=idx.words, primary=idx.primary, L2=idx.L2)
    n = min(reads.n, args.stats_sample)
    s = reads.subset(np.arange(n))
    want, per, st = oracle.seed(oi, s.codes, s.offs, threads=min(16, os.cpu_count() or 1),
                                min_seed_len=opt.min_seed_len)
    bpr = float(per["bytes"].mean())
    b64 = (32.0 * st["n_bkt64"] + st["n_bases"] + 32.0 * st["n_intv"]) / max(n, 1)
    parity = None
    if args.parity:
        b = gpu.batch(s.n, int(s.codes.size), int(s.lens.max()))
        try:
            b.set_reads(s.codes, s.offs)
            b.run(opt)
            got = b.fetch().to_smgo()
        finally:
            b.close()
        parity = {"reads": n, "intervals": int(st["n_intv"]), "bit_exact": got == want,
                  "against": "C restatement of the seeding loop (oracle/, pinned to the compiled reference's streams)"}
    cpu = None
    if args.cpu_seconds > 0:
        # calibrate on a small slice, then size the sample for ~cpu_seconds
        cal = reads.subset(np.arange(min(reads.n, 2000)))
        t, _ = oracle.seed_timed(oi, cal.codes, cal.offs, threads=cores, min_seed_len=opt.min_seed_len)
        rate = cal.n / max(t, 1e-6)
        m = int(min(reads.n, max(cal.n, rate * args.cpu_seconds)))
        sample = reads.subset(np.arange(m))
        kind = "port"
        if oracle.ref_available():
            with tempfile.TemporaryDirectory() as d:
                p = os.path.join(d, "s.smrd")
                synth.write_smrd(p, sample)
                r = oracle.ref_bench(idx_path, p, cores, m, min_seed_len=opt.min_seed_len)
                secs, kind = r["seconds"], "reference"
        else:
            secs, _ = oracle.seed_timed(oi, sample.codes, sample.offs, threads=cores, min_seed_len=opt.min_seed_len)
        cpu = {"value": round(m / secs, 1), "unit": "reads/s", "cores": cores, "kind": kind,
               "host": cpu_inventory(),
               "per_core": round(m / secs / cores, 1),
               "sample": f"first {m} of the benchmark's {args.read_len} bp reads on rank 0, {secs:.1f} s wall, "
                         f"{cores} pthreads (one per physical core)"}
    oi.close()
    sw = sw_cpu(sw_tasks) if (sw_tasks is not None and args.cpu_seconds > 0) else None
    return bpr, b64, st, n, parity, cpu, sw


def cpu_inventory() -> dict:
    """The host's CPUs as this process may use them: logical CPUs, physical
    cores (distinct (package, core) pairs of /proc/cpuinfo), the affinity
    mask, the cgroup CPU quota, and the model.  `use` = the threads the CPU
    baseline runs: one per physical core, capped by the affinity mask and the
    cgroup quota (threads past the quota only time-slice)."""
    inv = {"logical": os.cpu_count() or 1, "model": None}
    try:
        inv["affinity"] = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        inv["affinity"] = inv["logical"]
    cores, pkg, core = set(), None, None
    try:
        with open("/proc/cpuinfo") as fh:
            for line in fh:
                k, _, v = line.partition(":")
                k, v = k.strip(), v.strip()
                if k == "model name" and inv["model"] is None:
                    inv["model"] = v
                elif k == "physical id":
                    pkg = v
                elif k == "core id":
                    core = v
                elif not k and pkg is not None:
                    cores.add((pkg, core))
                    pkg = core = None
        if pkg is not None:
            cores.add((pkg, core))
    except OSError:
        pass
    inv["physical_cores"] = len(cores) or inv["logical"]
    quota = None
    try:
        with open("/sys/fs/cgroup/cpu.max") as fh:
            q, per = fh.read().split()[:2]
            if q != "max":
                quota = max(1, int(int(q) / int(per)))
    except (OSError, ValueError):
        pass
    inv["cgroup_quota_cpus"] = quota
    inv["use"] = max(1, min(inv["physical_cores"], inv["affinity"], quota or 1 << 30))
    return inv


def traffic_for(args, path: str, build_id: str, kernel_id: str | None = None, launch: dict | None = None):
    """Per-launch memory-side counters of seed_kernel recorded by
    tools/traffic.py for this exact workload AND either this library build or
    this seeding kernel (smem_gpu_kernel_id: its sources and compile flags) at
    this launch shape (grid, block), or None.  The second form keeps the
    counters of a kernel that a runtime-only change did not touch."""
    if not path or not os.path.exists(path):
        return None
    with open(path) as fh:
        t = json.load(fh)
    w = t.get("workload", {})
    want = {"genome_mbp": args.genome_mbp, "reads": args.reads, "read_len": args.read_len, "seed": args.seed,
            "sub": args.sub, "genome_profile": args.genome_profile}
    if any(w.get(k) != v for k, v in want.items()):
        return None
    # the counted launches ran the kernel variant this line ran (files before round 5: variant 2)
    if launch is None or t.get("variant", 2) != launch.get("variant"):
        return None
    if t.get("build_id") == build_id:
        return dict(t, matched_on="build_id + variant")
    shape = {"grid": launch.get("grid"), "block": launch.get("block")}
    if kernel_id and t.get("kernel_id") == kernel_id and t.get("launch") == shape:
        return dict(t, matched_on="kernel_id + variant + launch shape")
    return None


def gather_ceiling(path: str):
    """The random 32-B-bucket gather ceiling measured on MI355X (requests/s)."""
    if not path or not os.path.exists(path):
        return None
    with open(path) as fh:
        return json.load(fh)


class Dist:
    """One process per GPU (torchrun env); no collective touches the data path:
    a barrier around the timed region and two scalar reductions for the
    report.  gloo on CPU (tests) or RCCL ("nccl") on the GPUs."""

    def __init__(self, backend: str | None = None):
        import torch
        import torch.distributed as dist
        self.dist = dist
        self.rank = int(os.environ.get("RANK", 0))
        self.world = int(os.environ.get("WORLD_SIZE", 1))
        self.local = int(os.environ.get("LOCAL_RANK", 0))
        self.device = "cpu"
        # the GPU this rank drives (local rank, wrapped when a rehearsal runs
        # more ranks than the node has GPUs)
        n_dev = torch.cuda.device_count()
        self.gpu = self.local % n_dev if n_dev > 0 else 0
        if self.world > 1:
            # RCCL when every rank has a GPU of its own; gloo on CPU for a
            # rehearsal with more ranks than GPUs (RCCL refuses two ranks on
            # one device) -- only a barrier and two scalars go through it
            local_world = int(os.environ.get("LOCAL_WORLD_SIZE", self.world))
            default = "nccl" if n_dev >= local_world and n_dev > 0 else "gloo"
            backend = backend or os.environ.get("SMEM_DIST_BACKEND") or default
            if backend == "nccl":
                torch.cuda.set_device(self.gpu)
                self.device = "cuda"
                dist.init_process_group(backend, device_id=torch.device("cuda", self.gpu))
            else:
                dist.init_process_group(backend)

    def barrier(self):
        if self.world > 1:
            self.dist.barrier()

    def _reduce(self, v: float, op) -> float:
        if self.world == 1:
            return v
        import torch
        t = torch.tensor([v], dtype=torch.float64, device=self.device)
        self.dist.all_reduce(t, op=op)
        return float(t.item())

    def allmax(self, v: float) -> float:
        return self._reduce(v, self.dist.ReduceOp.MAX)

    def allsum(self, v: float) -> float:
        return self._reduce(v, self.dist.ReduceOp.SUM)

    def close(self):
        if self.world > 1:
            self.dist.destroy_process_group()


def aggregate(d: Dist, elapsed: float, reads_per_rank: int, steps: int):
    """Whole-job throughput: all ranks' reads over the slowest rank's time."""
    elapsed_max = d.allmax(elapsed)
    total = d.allsum(float(reads_per_rank)) * steps
    return total / elapsed_max, elapsed_max


def streaming_report(gpu, reads, opt, args, resident_rate: float) -> dict:
    """bwa mem's chunk loop over host buffers (smem_gpu_seed_stream): chunks
    staged into pinned memory, H2D, seeding + compaction, every interval D2H
    into pinned memory; workers overlap.  One warm pass (buffer creation) is
    not timed."""
    chunk = min(args.stream_chunk, max(2, reads.n))
    # warm pass: creates the pooled worker batches (device buffers, ~1 GB of
    # pinned result memory each) outside the timed pass
    pk = bool(args.stream_packed)
    warm = reads.subset(np.arange(min(reads.n, chunk * args.stream_workers)))
    gpu.seed_stream(warm.codes, warm.offs, opt, chunk_reads=chunk, workers=args.stream_workers, pairs=args.pairs,
                    packed=pk)
    passes = []
    for _ in range(max(1, args.stream_passes)):
        st, _ = gpu.seed_stream(reads.codes, reads.offs, opt, chunk_reads=chunk, workers=args.stream_workers,
                                pairs=args.pairs, packed=pk)
        passes.append(st)
    passes.sort(key=lambda x: x["wall_s"])
    st = passes[len(passes) // 2]  # the median pass
    rate = st["n_reads"] / st["wall_s"]
    return {"reads": int(st["n_reads"]), "reads_per_s": round(rate, 1), "wall_s": round(st["wall_s"], 3),
            "passes_reads_per_s": [round(x["n_reads"] / x["wall_s"], 1) for x in passes],
            "stage_run_fetch_s": [round(st["stage_s"], 3), round(st["run_s"], 3), round(st["fetch_s"], 3)],
            "chunk_reads": chunk, "workers": int(st["workers"]), "chunks": int(st["n_chunks"]),
            "h2d_GB": round(st["h2d_bytes"] / 1e9, 3), "d2h_GB": round(st["d2h_bytes"] / 1e9, 3),
            "intervals": int(st["n_intv"]), "packed": pk,
            "ratio_to_resident": round(rate / resident_rate, 3) if resident_rate else None,
            "what": "PCIe-inclusive: host reads -> pinned staging -> H2D -> seed_kernel + compaction -> D2H of every "
                    "interval into pinned host memory (smem_gpu_seed_stream, kt_for_batch-style workers; packed: "
                    "16-B smem_pintv_t wire entries)"}


def sa_lookup(batch, opt, reps: int = 3) -> dict:
    """The next stage on the same index: bwt_sa of every seed
    occurrence of the batch (software/bwamem.c:462-474), on the GPU; reported
    beside the SMEM metric, not part of a step."""
    batch.run(opt)
    best, all_ms = None, []
    for _ in range(reps):
        batch.sa(opt.min_seed_len, 10000)
        st = batch.stats()
        all_ms.append(st["sa_ms"])
        if best is None or st["sa_ms"] < best["sa_ms"]:
            best = st
    return {"ms_per_batch": round(best["sa_ms"], 3), "ms_per_batch_mean": round(float(np.mean(all_ms)), 3),
            "ms_runs": [round(x, 3) for x in all_ms], "occurrences": int(best["n_occ"]),
            "occurrences_per_s": round(best["n_occ"] / (best["sa_ms"] * 1e-3), 1),
            "what": "bwt_sa of every seed occurrence (seed length >= 19, x2 <= max_occ 10000); "
                    ".sa sa_intv 32, device copy densified to every 4th row at load"}


def chain_report(batch, opt, l_pac: int, reps: int = 3) -> dict:
    """The stage after bwt_sa: mem_chain + mem_chain_flt of
    every read of the batch on the GPU (software/bwamem.c:593-690), over the
    SA positions left in HBM; reported beside the SMEM metric."""
    batch.run(opt)
    batch.sa(opt.min_seed_len, 10000)
    best, all_ms = None, []
    for _ in range(reps):
        batch.chain(l_pac)
        st = batch.stats()
        all_ms.append(st["chain_ms"])
        if best is None or st["chain_ms"] < best["chain_ms"]:
            best = st
    n = batch.n_reads
    return {"ms_per_batch": round(best["chain_ms"], 3), "ms_per_batch_mean": round(float(np.mean(all_ms)), 3),
            "ms_runs": [round(x, 3) for x in all_ms], "chains": int(best["n_chains"]),
            "seed_occurrences": int(best["n_occ"]), "reads_per_s": round(n / (best["chain_ms"] * 1e-3), 1),
            "what": "mem_chain (kbtree of chains, test_and_merge) + mem_chain_flt, w 100, max_chain_gap 10000"}


def pack_pac(codes) -> np.ndarray:
    """2-bit forward strand as bns_fasta2bntseq packs it (software/bntseq.c:303-309)."""
    c = np.asarray(codes, dtype=np.uint8)
    n = c.size
    out = np.zeros((n + 3) // 4, dtype=np.uint8)
    for k in range(4):
        part = c[k::4]
        out[:part.size] |= (np.minimum(part, 3) << (6 - 2 * k)).astype(np.uint8)
    return out


def dp_roofline(cells: float, ms: float) -> dict:
    achieved = cells / (ms * 1e-3)
    peak = VALU_INT32_OPS / OPS_PER_CELL
    return {"bound": "valu", "achieved": round(achieved, 1), "peak": round(peak, 1), "unit": "cells/s",
            "frac": round(achieved / peak, 5), "gcups": round(achieved / 1e9, 2),
            "peak_source": f"VALU int32 {VALU_INT32_OPS / 1e12:.1f} T ops/s (256 CUs x 4 SIMDs x 32 lanes x 2.4 GHz) / "
                           f"{OPS_PER_CELL} ops per affine-gap cell"}


def aln_report(gpu, batch, opt, l_pac: int, pac=None, reads=None, reps: int = 3, cell_sample: int = 50000) -> dict:
    """Chains -> alignment regions (mem_chain2aln_short /
    mem_chain2aln of every filtered chain, software/bwamem.c:1452-1460) on the
    GPU over the chains, seeds, reads and .pac already in HBM
    (smem_batch_chain2aln); reported beside the SMEM metric."""
    import smemgpu
    batch.run(opt)
    batch.sa(opt.min_seed_len, 10000)
    batch.chain(l_pac)
    best, all_ms = None, []
    for _ in range(reps):
        batch.chain2aln(smemgpu.aln_opt(min_seed_len=opt.min_seed_len))
        st = batch.stats()
        all_ms.append(st["aln_ms"])
        if best is None or st["aln_ms"] < best["aln_ms"]:
            best = st
    n = batch.n_reads
    cells = None
    if pac is not None and reads is not None:
        # the DP cells the stage computes, counted by the restatement (the
        # checker, not the measured path) on the first cell_sample reads
        # (same chains), scaled to the batch
        from oracle import oracle
        res = batch.fetch(mask=4)   # FETCH_CHAINS
        m = min(cell_sample, n)
        aopt = oracle.aln_opt(min_seed_len=opt.min_seed_len)
        oracle.dp_cells(True)
        oracle.ext_shapes(True)
        oracle.seed_uses(True)
        oracle.aln(pac, l_pac, reads.codes, reads.offs[:m + 1], res.chains, res.chain_off[:m + 1], res.seeds, aopt)
        ext, sw = oracle.dp_cells(True)
        shapes = oracle.ext_shapes(True)
        uses = oracle.seed_uses(True)
        cells = {"ksw_extend2_in_band": ext, "ksw_align2": sw, "sample_reads": m,
                 "per_read": round((ext + sw) / max(m, 1), 1),
                 "extensions_by_qlen": {lab: {"calls": c, "cells": x} for lab, (c, x) in
                                        zip(("<=16", "<=32", "<=64", "<=128", "<=256", ">256"), shapes)},
                 "seed_regions": uses}
    out = {"ms_per_batch": round(best["aln_ms"], 3), "ms_per_batch_mean": round(float(np.mean(all_ms)), 3),
           "ms_runs": [round(x, 3) for x in all_ms], "regions": int(best["n_regs"]), "chains": int(best["n_chains"]),
           "reads_per_s": round(n / (best["aln_ms"] * 1e-3), 1)}
    if cells:
        out["dp_cells"] = cells
        out["roofline"] = dp_roofline(cells["per_read"] * n, best["aln_ms"])
        out["roofline"]["cells_note"] = (f"cells per read counted by the restatement on the first {cells['sample_reads']} "
                                         "reads x the batch's reads")
    return dict(out, **{
            "what": "mem_chain2aln_short / mem_chain2aln (ksw_align2, ksw_extend2 both ways, MAX_BAND_TRY) of every "
                    "chain kept by mem_chain_flt, one wave per read, chains / seeds / reads / .pac resident in HBM"})


def aln_cpu(args, idx_path: str, reads, genome_codes, opt, n: int = 20000) -> dict:
    """The reference's own chain2aln loop (oracle/_ref ref_harness aln: mem_chain
    + mem_chain_flt untimed, then mem_chain2aln_short / mem_chain2aln timed),
    one thread, on the first n reads: the alignment stage's CPU baseline."""
    from oracle import oracle
    from smemgpu import synth
    if not oracle.ref_available():
        return None
    with tempfile.TemporaryDirectory() as d:
        pac = os.path.join(d, "g.pac")
        pack_pac(genome_codes).tofile(pac)
        p = os.path.join(d, "s.smrd")
        m = min(n, reads.n)
        synth.write_smrd(p, reads.subset(np.arange(m)))
        r = oracle.ref_aln_time(idx_path, idx_path[:-4] + ".sa", pac, p, opt.min_seed_len)
    return {"value": round(r["reads"] / r["chain2aln_seconds"], 1), "unit": "reads/s", "cores": 1,
            "kind": "reference", "regions": int(r["regions"]),
            "sample": f"first {m} reads, chain2aln loop {r['chain2aln_seconds']:.2f} s (chaining untimed)"}


def sw_report(gpu, genome_codes, n_unique: int = 20000, tile: int = 10, reps: int = 3):
    """SW extension: ksw_extend2 on the GPU over
    problems shaped like mem_chain2aln's left/right extensions, drawn from the
    bench genome (n_unique distinct problems, the batch tiled `tile` times);
    reported beside the SMEM metric.  Returns (report, the distinct problems)."""
    from smemgpu import synth
    kb = synth.make_ksw_tasks(genome_codes, n_unique, seed=771)
    big = synth.KswBatch(np.tile(kb.tasks, tile), kb.q, kb.t, kb.mat)
    best, all_ms = float("inf"), []
    for _ in range(reps):
        _, ms = gpu.ksw_extend(big)
        all_ms.append(ms)
        best = min(best, ms)
    cells = int(np.sum(kb.tasks["qlen"].astype(np.int64) * kb.tasks["tlen"])) * tile
    from oracle import oracle
    oracle.dp_cells(True)
    oracle.ksw(kb)
    band = oracle.dp_cells(True)[0] * tile   # in-band cells ksw_extend2 computes (restatement's count)
    return {"tasks": int(big.tasks.size), "kernel_ms": round(best, 3),
            "kernel_ms_mean": round(float(np.mean(all_ms)), 3), "dp_cells_in_band": band,
            "roofline": dp_roofline(band, best),
            "tasks_per_s": round(big.tasks.size / (best * 1e-3), 1),
            "what": "ksw_extend2 (software/ksw.c:379), one wave per problem; synthetic mem_chain2aln-shaped "
                    "left/right extensions of 100-250 bp reads (2-5% subs, 0.4% indels), w 100 (some 200 / narrow), "
                    "zdrop 100, end_bonus 5", "qlen_x_tlen_cells_upper_bound": cells}, kb


def sw_cpu(kb) -> dict:
    """The compiled reference's own ksw_extend2 (oracle/_ref ref_harness ksw,
    one thread) on the same distinct problems: the SW stage's CPU baseline
    (run from cpu_leg)."""
    from oracle import oracle
    from smemgpu import synth
    if not oracle.ref_available():
        return None
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "t.smkt")
        synth.write_smkt(p, kb)
        t = time.perf_counter()
        oracle.ref_ksw(p, os.path.join(d, "r.smkr"))
        secs = time.perf_counter() - t
    return {"value": round(kb.tasks.size / secs, 1), "unit": "tasks/s", "cores": 1, "kind": "reference",
            "sample": f"{kb.tasks.size} problems, {secs:.2f} s incl. file I/O"}


BWA_GPU = os.path.join(ROOT, "oracle", "_ref", "bwa-gpu")       # the reference's `bwa`, integration/ patch
REF_HARNESS = os.path.join(ROOT, "oracle", "_ref", "ref_harness")  # the unpatched reference pipeline


def _mem_times(stderr: str) -> tuple:
    """(reads, summed real seconds) of the reference's per-chunk
    "[M::mem_process_seqs] Processed N reads in C CPU sec, R real sec" lines
    (software/bwamem.c:1637-1638)."""
    import re
    n, real = 0, 0.0
    for m in re.finditer(r"\[M::mem_process_seqs\] Processed (\d+) reads in ([\d.]+) CPU sec, ([\d.]+) real sec",
                         stderr):
        n += int(m.group(1))
        real += float(m.group(3))
    return n, real


def _main_real(stderr: str):
    """main()'s "[main] Real time: R sec" (software/main.c), or None"""
    import re
    m = re.search(r"\[main\] Real time: ([\d.]+) sec", stderr)
    return float(m.group(1)) if m else None


def _mem_chunks(stderr: str) -> list:
    """(reads, real seconds) of each mem_process_seqs chunk: the first chunk
    also pays each worker batch's first-use device and pinned allocations."""
    import re
    return [(int(m.group(1)), float(m.group(3))) for m in re.finditer(
        r"\[M::mem_process_seqs\] Processed (\d+) reads in ([\d.]+) CPU sec, ([\d.]+) real sec", stderr)]


def _sam_body(path: str):
    """sha256 and line count of a SAM file without its @PG line."""
    import hashlib
    h = hashlib.sha256()
    n = 0
    with open(path, "rb") as fh:
        for line in fh:
            if line.startswith(b"@PG"):
                continue
            h.update(line)
            n += 1
    return h.hexdigest(), n


def e2e_report(args, base: str, genome_codes, reads, threads: int, gpu: int) -> dict | None:
    """The product path end to end (north_star: the `bwa mem` CLI unchanged):
    the reference's own `bwa mem` built with the integration/ patch against
    libsmemgpu.so (oracle/_ref/bwa-gpu: every kt_for_batch worker batch's
    seeding -> bwt_sa -> mem_chain + mem_chain_flt -> mem_chain2aln on the
    GPU, sort / pairing / SAM on the CPU) beside the unpatched reference
    pipeline on the same reads, index and threads (oracle/_ref/ref_harness
    mem: main_mem's body over mem_process_seqs with -b 1, every batch on the
    CPU path -- the only way the reference runs without its FPGA).  The index
    prefix is the bench's own .bwt / .sa plus .pac / .ann / .amb in `bwa
    index` format (synth.write_bwa_bns; byte-identical to bwa index,
    tests/test_bwa_integration.py).  Timed: each process's wall clock
    (index load + upload included) and the reference's own per-chunk
    mem_process_seqs real time.  SAM identity is checked on every read."""
    from smemgpu import synth
    if not (os.path.exists(BWA_GPU) and os.path.exists(REF_HARNESS)) or args.e2e_reads <= 0:
        return None
    if not all(os.path.exists(base + e) for e in (".pac", ".ann", ".amb")):
        t = time.time()
        synth.write_bwa_bns(base + ".tmp", genome_codes)
        for e in (".pac", ".ann", ".amb"):
            os.replace(base + ".tmp" + e, base + e)
        log(f"bwa .pac/.ann/.amb written in {time.time() - t:.1f} s")
    m = min(args.e2e_reads, reads.n)
    sub = reads.subset(np.arange(m))
    batch = args.e2e_batch or None  # None: no -b, the binding's batch plan (mem_gpu_auto_batch)
    bflag = ["-b", str(batch)] if batch else []
    out = {"reads": m, "read_len": args.read_len, "threads": threads, "batch": batch or "auto (per-device plan)",
           "what": "bwa-gpu mem (the reference's bwa mem with integration/patches, libsmemgpu.so: seeding -> "
                   "bwt_sa -> mem_chain + mem_chain_flt -> mem_chain2aln on the GPU, the regions copied back, "
                   "mem_sort_and_dedup / mem_mark_primary_se / mem_reg2sam_se on the CPU) vs the unpatched "
                   "reference pipeline (ref_harness mem = main_mem over mem_process_seqs, -b 1) on the same reads, "
                   "index, threads; seconds include loading the index"}
    with tempfile.TemporaryDirectory(dir=args.cache) as d:
        fq = os.path.join(d, "r.fq")
        synth.write_fastq(fq, sub)
        env_base = dict(os.environ, SMEM_GPU_DEVICES=str(gpu), SMEM_GPU_TIMES="1")
        legs = [("gpu", [BWA_GPU, "mem", "-t", str(threads), *bflag, base, fq], {}),
                ("gpu_chains_only", [BWA_GPU, "mem", "-t", str(threads), *bflag, base, fq],
                 {"SMEM_GPU_STAGES": "1"}),
                ("reference", [REF_HARNESS, "mem", base, fq, str(threads), "1", "0"], {})]
        runs = _e2e_legs(d, legs, env_base, m)
        if runs is None:
            return dict(out, error="a leg failed (see the bench log)")
        out.update(runs)
        out["sam_identical"] = runs["gpu"]["sam_sha256"] == runs["reference"]["sam_sha256"] == \
            runs["gpu_chains_only"]["sam_sha256"]
        out.update(_e2e_speedups(runs))
        if args.e2e_pairs > 0:
            # C3's shape at human size: interleaved pairs (insert N(500, 50)), `bwa mem -p`; the
            # reference pairs each chunk's mates itself (mem_sam_pe, insert statistics per chunk)
            t = time.time()
            pe = synth.make_pairs(genome_codes, args.e2e_pairs, args.read_len, seed=args.seed + 7)
            fq2 = os.path.join(d, "p.fq")
            synth.write_fastq(fq2, pe, prefix="p", pairs=True)
            log(f"e2e pe: {args.e2e_pairs} pairs made in {time.time() - t:.1f} s")
            pbatch = args.e2e_batch or None
            legs = [("gpu", [BWA_GPU, "mem", "-p", "-t", str(threads), *(["-b", str(pbatch)] if pbatch else []),
                             base, fq2], {}),
                    ("reference", [REF_HARNESS, "mem", base, fq2, str(threads), "1", "1"], {})]
            pr = _e2e_legs(d, legs, env_base, 2 * args.e2e_pairs, tag="pe ")
            if pr is None:
                out["pe"] = {"error": "a leg failed (see the bench log)"}
            else:
                out["pe"] = {"pairs": args.e2e_pairs, "reads": 2 * args.e2e_pairs,
                             "batch": pbatch or "auto (per-device plan)",
                             "insert": "N(500, 50)", **pr,
                             "sam_identical": pr["gpu"]["sam_sha256"] == pr["reference"]["sam_sha256"],
                             **_e2e_speedups(pr)}
    return out


def e2e_chunks_report(args, base: str, reads, threads: int, gpu: int) -> dict:
    """The product path over several `bwa mem` chunks (10 Mbp x threads each,
    software/fastmap.c:213): steady-state throughput with the patched chunk
    pipeline (the next chunk parsed and the last one printed while a chunk is
    processed), against the reference's sequential loop on the same reads."""
    from smemgpu import synth
    m = reads.n
    batch = args.e2e_batch or None
    out = {"reads": m, "read_len": args.read_len, "threads": threads, "batch": batch or "auto (per-device plan)",
           "what": "bwa-gpu mem vs the unpatched reference pipeline over several chunks of 10 Mbp x threads: "
                   "wall clock, and the reference's mem_process_seqs real time summed over the chunks"}
    with tempfile.TemporaryDirectory(dir=args.cache) as d:
        fq = os.path.join(d, "c.fq")
        synth.write_fastq(fq, reads, prefix="c")
        env_base = dict(os.environ, SMEM_GPU_DEVICES=str(gpu), SMEM_GPU_TIMES="1")
        legs = [("gpu", [BWA_GPU, "mem", "-t", str(threads), *(["-b", str(batch)] if batch else []), base, fq], {}),
                ("reference", [REF_HARNESS, "mem", base, fq, str(threads), "1", "0"], {})]
        runs = _e2e_legs(d, legs, env_base, m, tag="chunks ")
        if runs is None:
            return dict(out, error="a leg failed (see the bench log)")
        out.update(runs)
        out["sam_identical"] = runs["gpu"]["sam_sha256"] == runs["reference"]["sam_sha256"]
        out.update(_e2e_speedups(runs))
        out["reads_per_s_wall"] = {k: round(m / runs[k]["wall_s"], 1) for k in ("gpu", "reference")}
    return out


def _e2e_legs(d: str, legs, env_base: dict, m: int, tag: str = "") -> dict | None:
    """Run each (name, argv, env) leg with its SAM into d; wall clock, the
    reference's own mem_process_seqs real time, SAM digest (minus @PG)."""
    import subprocess
    runs = {}
    for name, cmd, env in legs:
        sam = os.path.join(d, name + ".sam")
        t = time.perf_counter()
        with open(sam, "wb") as fh:
            p = subprocess.run(cmd, stdout=fh, stderr=subprocess.PIPE, env=dict(env_base, **env), timeout=900)
        wall = time.perf_counter() - t
        err = p.stderr.decode(errors="replace")
        if p.returncode != 0:
            log(f"e2e {tag}{name} failed ({p.returncode}): {err[-800:]}")
            return None
        n_proc, real = _mem_times(err)
        import re
        gt = [float(x) for x in re.findall(r"\[M::mem_batch_gpu\] \d+ reads through the GPU stages in ([\d.]+) s", err)]
        gparts = [tuple(float(v) for v in m) for m in re.findall(
            r"\(seed ([\d.]+) sa ([\d.]+) chain ([\d.]+) regions ([\d.]+) fetch ([\d.]+)\)", err)]
        digest, n_lines = _sam_body(sam)
        os.unlink(sam)
        runs[name] = {"wall_s": round(wall, 3), "mem_process_seqs_real_s": round(real, 3),
                      "outside_mem_process_seqs_s": round(wall - real, 3),
                      # main()'s own "[main] Real time" (software/main.c): what is left of the wall
                      # clock after it is the process's exit (the runtime's teardown)
                      "main_real_s": _main_real(err),
                      "reads_per_s_wall": round(m / wall, 1),
                      "reads_per_s_mem_process_seqs": round(m / real, 1) if real > 0 else None,
                      "reads_processed": n_proc, "sam_sha256": digest, "sam_lines": n_lines,
                      "cpu_fallback": "seeding on the CPU" in err or "refused" in err}
        # the binding's start-up / teardown lines (SMEM_GPU_TIMES=1): where the
        # time outside mem_process_seqs goes
        tl = [ln for ln in err.splitlines()
              if ln.startswith(("[M::main_mem]", "[M::smem_gpu_", "[M::mem_gpu_")) and "reads through" not in ln
              and "smem_gpu_reserve_slots] device" not in ln and "smem_gpu_collect" not in ln]
        if tl:
            runs[name]["startup_lines"] = tl[:32]
        ch = _mem_chunks(err)
        if len(ch) > 1:
            runs[name]["mem_process_seqs_chunks"] = [[c, round(t, 3)] for c, t in ch]
            rest = ch[1:]
            runs[name]["reads_per_s_after_first_chunk"] = round(sum(c for c, _ in rest) / max(sum(t for _, t in rest), 1e-9), 1)
        if gt:  # the integration patch's per-batch wall time of mem_batch_gpu (SMEM_GPU_TIMES=1)
            if gparts:
                runs[name]["gpu_stage_s_sum_by_stage"] = {
                    k: round(sum(p[i] for p in gparts), 3)
                    for i, k in enumerate(("seed", "sa", "chain", "regions", "fetch"))}
            runs[name].update(gpu_batches=len(gt), gpu_stage_s_sum=round(sum(gt), 3),
                              gpu_stage_s_max=round(max(gt), 4),
                              gpu_stage_note="sum over the kt_for_batch workers' batches of the time each spent in "
                                             "mem_batch_gpu (seeding -> regions on the GPU, waits included); "
                                             "workers run concurrently, so sum / threads is the per-worker share of "
                                             "mem_process_seqs")
        log(f"e2e {tag}{name}: {wall:.1f} s wall, mem_process_seqs {real:.1f} s")
    return runs


def _e2e_speedups(runs: dict) -> dict:
    g, r = runs["gpu"], runs["reference"]
    out = {"speedup_wall": round(r["wall_s"] / g["wall_s"], 2)}
    if g["mem_process_seqs_real_s"] > 0:
        out["speedup_mem_process_seqs"] = round(r["mem_process_seqs_real_s"] / g["mem_process_seqs_real_s"], 2)
    return out


def span_union(spans) -> float:
    """Total time covered by the [start, end) intervals (chip-clock ticks)."""
    tot, cur = 0, None
    for a, b in sorted(spans):
        if cur is None or a > cur[1]:
            if cur is not None:
                tot += cur[1] - cur[0]
            cur = [a, b]
        else:
            cur[1] = max(cur[1], b)
    return float(tot + (cur[1] - cur[0] if cur else 0))


def roofline(args, bpr, bpr64, ostats, n_counted, reads_n, k_ms, a_ms, build_id, busy_ms, clock_check,
             launch: dict | None = None) -> dict:
    achieved = bpr * reads_n / (busy_ms * 1e-3) / 1e9
    out = {
        "bound": "hbm",
        "achieved": round(achieved, 2),
        "peak": HBM_PEAK_GBS,
        "unit": "GB/s",
        "frac": round(achieved / HBM_PEAK_GBS, 4),
        "traffic": None,
        "kernel": kernel_name((launch or {}).get("variant", 2)),
        "kernel_busy_ms": round(busy_ms, 3),
        "kernel_busy_ms_source": "time the GPU spent in seed_kernel over the timed region (union of every launch's "
                                 "first-wave-start .. last-wave-end on the chip's 100 MHz clock, s_memrealtime) / "
                                 "launches: the two workers' launches overlap, so this is the per-launch time of the "
                                 "kernel, and `achieved` = algorithmic bytes per launch / it",
        "kernel_ms": round(k_ms, 3),
        "kernel_ms_source": "HIP events on each worker's stream around every seed_kernel launch of the timed region "
                            "(mean; what rocprofv3 --stats averages): overlapping launches each last longer than the "
                            "kernel's share of the GPU",
        "frac_per_launch": round(bpr * reads_n / (k_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
        "chip_clock_check": round(clock_check, 4) if clock_check else None,
        "kernel_ms_alone": round(a_ms, 3),
        "frac_alone": round(bpr * reads_n / (a_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
        "bytes_per_read": round(bpr, 1),
        "bytes_per_read_occ64": round(bpr64, 1),
        "achieved_occ64": round(bpr64 * reads_n / (a_ms * 1e-3) / 1e9, 2),
        "frac_occ64": round(bpr64 * reads_n / (a_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
        "bytes_per_read_sample": n_counted,
        "extends_per_read": round(ostats["n_ext"] / max(n_counted, 1), 1),
        "occ64_buckets_per_read": round(ostats["n_bkt64"] / max(n_counted, 1), 1),
    }
    import smemgpu
    t = traffic_for(args, args.traffic_json, build_id, smemgpu.kernel_id(), launch)
    if t:
        out["traffic_build"] = {"build_id": t.get("build_id"), "kernel_id": t.get("kernel_id"),
                                "matched_on": t.get("matched_on")}
        rq = float(t["rdreq_per_launch"])
        out["traffic"] = round(rq * 64.0, 1)   # one 64-B line per fabric read request (FETCH_SIZE calibration)
        out["traffic_note"] = ("TCC_EA0_RDREQ x 64 B per launch (tools/traffic.py, " + t.get("measured", "?") +
                               "): each random 16/32-B chunk request moves one 64-B line -- FETCH_SIZE = 64 B x "
                               "requests, calibrated on known random 16-B and 32-B gathers (profiles/r02/probe)")
        out["traffic_over_occ64_bytes"] = round(rq * 64.0 / (bpr64 * reads_n), 3)
        out["dram_GBps"] = round(rq * 64.0 / (a_ms * 1e-3) / 1e9, 1)
        c = gather_ceiling(args.ceiling_json)
        if c:
            rate = rq / (a_ms * 1e-3)
            out["request_roofline"] = {
                "requests_per_launch": int(rq), "achieved_Greq_per_s": round(rate / 1e9, 2),
                "ceiling_Greq_per_s": c["occ64_3p1gb_Greq_per_s"], "frac": round(rate / 1e9 / c["occ64_3p1gb_Greq_per_s"], 3),
                "ceiling_source": c["source"]}
        if "write_bytes_per_launch" in t:
            out["write_bytes_per_launch"] = t["write_bytes_per_launch"]
        sq = t.get("sq")
        if sq:  # issue-side counters of the same kernel, build and workload (tools/traffic.py pass 3)
            n_ext = ostats["n_ext"] / max(n_counted, 1) * reads_n
            wc = max(sq.get("SQ_WAVE_CYCLES", 0.0), 1.0)
            out["sq_counters"] = {
                "valu_per_extend": round(sq["SQ_INSTS_VALU"] / n_ext, 2),
                "salu_per_extend": round(sq["SQ_INSTS_SALU"] / n_ext, 2),
                "valu_salu_per_extend": round((sq["SQ_INSTS_VALU"] + sq["SQ_INSTS_SALU"]) / n_ext, 2),
                "active_inst_any_frac": round(sq["SQ_ACTIVE_INST_ANY"] / wc, 3),
                "wait_any_frac": round(sq["SQ_WAIT_ANY"] / wc, 3),
                "per_launch": sq,
                "what": "SQ_INSTS_VALU / SALU per bwt_extend (extends per read from the restatement x reads), "
                        "SQ_ACTIVE_INST_ANY and SQ_WAIT_ANY over SQ_WAVE_CYCLES (all quad-cycles), one launch "
                        "alone, counted by rocprofv3 on this kernel_id + variant"}
    return out


DUMP_BYTES = 64_000_000   # --dump-outputs: all files together stay under this
DUMP_READS = 32768        # reads whose lists are written in full (fewer when they would not fit)


def _gather(off: np.ndarray, pick: np.ndarray) -> tuple:
    """(indices of the entries of the picked reads' lists in read order, their
    offsets rebased to 0) for lists laid out by off[n + 1]."""
    a = off[pick]
    ln = off[pick + 1] - a
    new_off = np.concatenate([[0], np.cumsum(ln)])
    return np.repeat(a - new_off[:-1], ln) + np.arange(int(new_off[-1])), new_off


def dump_outputs(path: str, batch, seed: int, rank: int = 0) -> None:
    """--dump-outputs: what the batch's last run left in HBM, as a caller gets
    it from Batch.fetch() (smem_batch_fetch + smem_batch_results), in float
    arrays (every value is an integer below 2^53, float64 holds it exactly):
      intv_per_read, calls_per_read   float32 [n_reads]: list lengths of every read
      sample_reads                    float64 [m]: a fixed seeded sample of read numbers, ascending
      intv, intv_off                  float64 [k, 4], [m + 1]: the sample's bwtintv_t (x0, x1, x2, info)
      call_n, call_off                float64 [c], [m + 1]: entries per smem_next2 call of the sample's reads
    Ranks past 0 write <name>_rank<r>.npy."""
    from smemgpu.lib import FETCH_INTV
    res = batch.fetch(mask=FETCH_INTV)
    intv_off, call_off = res.intv_off.astype(np.int64), res.call_off.astype(np.int64)
    n = intv_off.size - 1
    per_read, calls = np.diff(intv_off), np.diff(call_off)
    out = {}
    budget = DUMP_BYTES - 7 * 256   # .npy headers
    if 8 * n <= budget // 4:
        out["intv_per_read"] = per_read.astype(np.float32)
        out["calls_per_read"] = calls.astype(np.float32)
        budget -= 8 * n
    # the sample: the longest prefix of a seeded order of the reads whose lists fit
    order = np.random.default_rng([seed, 0x44554d50]).permutation(n)[:DUMP_READS]
    cost = np.cumsum(24 + 32 * per_read[order] + 8 * calls[order])
    pick = np.sort(order[:int(np.searchsorted(cost, budget - 16, side="right"))])
    ii, ioff = _gather(intv_off, pick)
    ci, coff = _gather(call_off, pick)
    out["sample_reads"] = pick.astype(np.float64)
    out["intv"] = res.intv[ii].astype(np.float64)
    out["intv_off"] = ioff.astype(np.float64)
    out["call_n"] = res.call_n[ci].astype(np.float64)
    out["call_off"] = coff.astype(np.float64)
    os.makedirs(path, exist_ok=True)
    for name, arr in out.items():
        np.save(os.path.join(path, name + (f"_rank{rank}" if rank else "") + ".npy"), arr)
    log(f"outputs of the last step written to {path}: {len(pick)} of {n} reads in full, "
        f"{sum(a.nbytes for a in out.values()) / 1e6:.1f} MB")


def time_seeding(args, d, gpu, reads, opt) -> dict:
    """The timed region of a seeding step (see the module docstring): W warmup
    steps (the alone launches give kernel_ms_alone), then K steps between
    barriers, --streams host workers each running whole steps on its own
    batch and stream.  Returns the step's numbers; the batches are closed."""
    import torch
    # one batch object (own HIP stream, own buffers) per host worker, each
    # holding the whole read set: a step is one full pass over the reads
    batches = []
    for _ in range(max(1, args.streams)):
        b = gpu.batch(reads.n, int(reads.codes.size), int(reads.lens.max()))
        b.set_reads(reads.codes, reads.offs)  # inputs resident in HBM before timing
        batches.append(b)
    batch = batches[0]
    torch.cuda.synchronize()
    # warmup; launches that run alone on the GPU (no other stream's kernels
    # beside them) give kernel_ms_alone
    alone_ms, alone_span = [], []
    compact_alone = 0.0
    for w in range(max(args.warmup, 2)):
        batch.run(opt)
        if w > 0:
            bs = batch.stats()
            alone_ms.append(bs["kernel_ms"])
            alone_span.append((bs["t_end"] - bs["t_start"]) / RT_TICKS_PER_MS)
            compact_alone = bs["compact_ms"]
    # the roofline's kernel time: HIP events on each worker's own stream around
    # every seed_kernel launch of the timed region (what rocprofv3 sees too)
    kernel_ms, spans = [], []
    for b in batches[1:]:
        b.run(opt)
    d.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if len(batches) == 1:
        for _ in range(args.steps):
            batch.run(opt)
            bs = batch.stats()
            kernel_ms.append(bs["kernel_ms"])
            spans.append((bs["t_start"], bs["t_end"]))
    else:
        # kt_for_batch-style workers (the reference's own host model,
        # software/kthread_batch.c:29-59): steps are dealt round-robin, each
        # worker runs whole steps on its own stream, so one step's tail and
        # compaction overlap the next step's seeding
        import threading
        errs = []

        def worker(wi):
            try:
                for k in range(wi, args.steps, len(batches)):
                    batches[wi].run(opt)
                    bs = batches[wi].stats()
                    kernel_ms.append(bs["kernel_ms"])
                    spans.append((bs["t_start"], bs["t_end"]))
            except Exception as e:  # surfaced below
                errs.append(e)

        th = [threading.Thread(target=worker, args=(wi,)) for wi in range(len(batches))]
        for t in th:
            t.start()
        for t in th:
            t.join()
        if errs:
            raise errs[0]
    torch.cuda.synchronize()
    d.barrier()
    elapsed = time.perf_counter() - t0
    st = batch.stats()
    value, elapsed_max = aggregate(d, elapsed, reads.n, args.steps)
    if getattr(args, "dump_outputs", None):
        # steps are dealt round-robin: the last one ran on this worker's batch
        dump_outputs(args.dump_outputs, batches[(args.steps - 1) % len(batches)], args.seed, d.rank)
    for b in batches[1:]:
        b.close()
    a_ms = float(np.mean(alone_ms))
    return {"batch": batch, "value": value, "elapsed_max": elapsed_max, "st": st,
            "k_ms": float(np.mean(kernel_ms)), "a_ms": a_ms,
            "busy_ms": span_union(spans) / RT_TICKS_PER_MS / max(len(spans), 1),
            "clock_check": float(np.mean(alone_span)) / a_ms if a_ms > 0 else None,
            "compact_alone": compact_alone}


def profile_report(args, d, cores, profile: str) -> dict:
    """The same step on the other genome profile (the headline runs the
    human-like one: ~46 % interspersed repeats + satellites, the closer
    stand-in for human_g1k_v37; beside it the uniform profile of rounds 1-4),
    same read seeds and sizes: value, busy time, roofline fraction, request
    fraction and counters (when tools/traffic.py recorded this kernel on this
    workload), extends per read, parity sample and the reference's CPU rate on
    a sample of these reads.  Its own index (cached like the headline's)."""
    import copy
    import smemgpu
    h = copy.copy(args)
    h.genome_profile = profile
    h.traffic_json = traffic_path(profile)
    h.dump_outputs = None   # the dump is the headline's
    t = time.time()
    idx, idx_path, sa, genome_codes = get_index(h, d.rank, d.barrier, d.gpu)
    t_index = time.time() - t
    reads = make_reads(h, d.rank, genome_codes, d.world)
    gpu = smemgpu.Gpu(idx, device=d.gpu, lanes_per_cu=args.lanes_per_cu, variant=args.variant, kmer_k=args.kmer_k)
    gpu_variant = gpu.variant
    opt = smemgpu.Options(min_seed_len=args.min_seed_len)
    T = time_seeding(h, d, gpu, reads, opt)
    h.cpu_seconds = min(args.cpu_seconds, 10.0)
    bpr, bpr64, ostats, n_counted, parity, cpu, _ = cpu_leg(h, gpu, opt, idx, idx_path, reads, cores)
    T["batch"].close()
    gpu.close()
    rf = roofline(h, bpr, bpr64, ostats, n_counted, reads.n, T["k_ms"], T["a_ms"], smemgpu.build_id(), T["busy_ms"],
                  T["clock_check"], {"grid": T["st"]["grid"], "block": T["st"]["block"], "variant": gpu_variant})
    out = {"value": round(T["value"], 1), "unit": "reads/s", "ms_per_step": round(T["elapsed_max"] / args.steps * 1e3, 3),
           "steps": args.steps, "genome_profile": profile, "reads": reads.n, "read_len": args.read_len,
           "kernel_busy_ms": rf["kernel_busy_ms"], "kernel_ms_alone": rf["kernel_ms_alone"],
           "frac": rf["frac"], "frac_alone": rf["frac_alone"], "achieved_GBps": rf["achieved"],
           "bytes_per_read": rf["bytes_per_read"], "extends_per_read": rf["extends_per_read"],
           "request_frac": (rf.get("request_roofline") or {}).get("frac"),
           "request_roofline": rf.get("request_roofline"),
           "traffic": rf.get("traffic"), "write_bytes_per_launch": rf.get("write_bytes_per_launch"),
           "sq_counters": rf.get("sq_counters"), "kernel": rf["kernel"], "kernel_variant": gpu_variant,
           "parity_sample": parity, "cpu_baseline": cpu,
           "index_s": round(t_index, 1),
           "what": ("the headline step on the human-like genome profile (~46 % interspersed repeats shaped like "
                    "RepeatMasker's classes + 3 % satellites)" if profile == "human" else
                    "the headline step on the uniform genome profile (random + 2 % diverged repeat families, exact "
                    "and tandem repeats: the headline profile of rounds 1-4)") + ", same sizes and read seeds"}
    del idx, sa, genome_codes
    return out


def main():
    args = parse()
    import torch
    import smemgpu

    d = Dist()
    rank, world = d.rank, d.world
    barrier = d.barrier
    if world > 1:  # the CPU baseline is an N=1 record (rank 0); N>1 lines carry null
        args.cpu_seconds = 0.0

    # the headline: set up, warm up, time the steps (and write their outputs);
    # everything after it that is not the line's own bookkeeping needs --full
    idx, idx_path, sa, genome_codes = get_index(args, rank, barrier, d.gpu, need_sa=args.full)
    reads = make_reads(args, rank, genome_codes, world)
    gpu = smemgpu.Gpu(idx, device=d.gpu, lanes_per_cu=args.lanes_per_cu, variant=args.variant, kmer_k=args.kmer_k)
    gpu_variant = gpu.variant
    opt = smemgpu.Options(min_seed_len=args.min_seed_len)
    log(f"index in HBM, {reads.n} reads made")
    T = time_seeding(args, d, gpu, reads, opt)
    batch, st, value, elapsed_max = T["batch"], T["st"], T["value"], T["elapsed_max"]
    log(f"{args.steps} steps timed: {elapsed_max / args.steps * 1e3:.3f} ms per step")

    out = None
    if rank == 0:
        cfg = CONFIGS[args.config]
        out = {
            "metric": METRIC,
            "value": round(value, 1),
            "unit": "reads/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed_max / args.steps * 1e3, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "u64",
            "data": "synthetic",
            "full": bool(args.full),
            "config": {
                "workload": f"{args.config}: synthetic {args.genome_mbp:g} Mbp genome index in HBM "
                            f"({args.genome_profile} repeat profile; stand-in for human_g1k_v37), "
                            f"{reads.n} x {args.read_len} bp {'PE (interleaved mates)' if args.pairs else 'SE'} reads "
                            f"resident per GPU, {args.sub:.0%} subs, 0.1% N, k={args.min_seed_len} r=1.5 s=10",
                "config": args.config,
                "config_what": cfg["what"],
                "genome_profile": args.genome_profile,
                "reads_per_gpu": reads.n,
                "read_len": args.read_len,
                "genome_bp": int(args.genome_mbp * 1e6),
                "index_bytes": int(idx.words.nbytes),
                "seed": args.seed,
                "parallelism": f"reads sharded over {world} GPU(s) in blocks of {BLOCK} dealt round-robin, index "
                               f"replicated, no collectives; {args.streams} host workers per GPU, each running whole "
                               f"steps on its own stream",
                "grid": st["grid"], "block": st["block"],
                "kernel_variant": gpu_variant, "kernel": kernel_name(gpu_variant), "kmer_k": args.kmer_k,
            },
            "kernel_ms": round(T["k_ms"], 3),
            "kernel_busy_ms": round(T["busy_ms"], 3),
            "kernel_ms_alone": round(T["a_ms"], 3),
            "compact_ms": round(T["compact_alone"], 3),
            "overflow_reads": st["n_overflow"],
            "build_id": smemgpu.build_id(),
            "kernel_id": smemgpu.kernel_id(),
            "build_id_matches_sources": smemgpu.build_id() == smemgpu.source_hash(),
        }
    if args.full:
        held = {"idx": idx, "sa": sa}
        del idx, sa
        full_report(args, d, out, held, idx_path, genome_codes, reads, gpu, gpu_variant, opt, T)
    else:
        batch.close()
        gpu.close()
    if rank == 0:
        print(json.dumps(out), flush=True)
    d.close()
    log("done")


def full_report(args, d, out, held, idx_path, genome_codes, reads, gpu, gpu_variant, opt, T) -> None:
    """--full: everything the benchmark measures and checks beside the
    headline, added to the line `out` (rank 0's; None on the other ranks).
    `held` holds the only references to the host index and .sa ("idx", "sa"),
    dropped before the other profile loads its own.  Closes the headline's
    batch and device handle on the way."""
    import smemgpu
    idx, sa = held["idx"], held["sa"]
    rank, world, barrier = d.rank, d.world, d.barrier
    batch, st, value = T["batch"], T["st"], T["value"]
    # the .sa upload + device densification, timed synchronously here (the
    # binding runs it in the background beside bwa's index load)
    os.environ["SMEM_GPU_SYNC_INIT"] = "1"
    t_sa = time.perf_counter()
    gpu.load_sa(sa)
    t_sa = time.perf_counter() - t_sa
    del os.environ["SMEM_GPU_SYNC_INIT"]

    # streaming (PCIe-inclusive) on every rank, then its aggregate; the
    # config's target read count, or the resident reads (c2)
    # (--stream-reads -1: no streaming leg)
    srep = None
    if args.stream_reads >= 0:
        sreads = reads if args.stream_reads == 0 else make_reads(args, rank, genome_codes, world, args.stream_reads,
                                                                 salt=1)
        barrier()
        srep = streaming_report(gpu, sreads, opt, args, value / world)
        s_rate = d.allsum(float(srep["reads"])) / d.allmax(srep["wall_s"])
        srep["reads_per_s_all_ranks"] = round(s_rate, 1)
        del sreads

    sa_rep = chain_rep = sw_rep = sw_tasks = aln_rep = None
    if rank == 0 and args.side_stages:
        sa_rep = sa_lookup(batch, opt)
        chain_rep = chain_report(batch, opt, idx.seq_len // 2)
        pac = pack_pac(genome_codes)
        gpu.load_pac(pac, idx.seq_len // 2)
        aln_rep = aln_report(gpu, batch, opt, idx.seq_len // 2, pac=pac, reads=reads)
        del pac
        sw_rep, sw_tasks = sw_report(gpu, np.asarray(genome_codes))

    cores = None
    if rank == 0:
        inv = cpu_inventory()
        cores = inv["use"]
        bpr, bpr64, ostats, n_counted, parity, cpu, sw_cpu_rep = cpu_leg(args, gpu, opt, idx, idx_path, reads, cores,
                                                                          sw_tasks)
        if sw_rep is not None:
            sw_rep["cpu_baseline"] = sw_cpu_rep
        if aln_rep is not None and args.cpu_seconds > 0:
            aln_rep["cpu_baseline"] = aln_cpu(args, idx_path, reads, genome_codes, opt)
        out.update({
            "roofline": roofline(args, bpr, bpr64, ostats, n_counted, reads.n, T["k_ms"], T["a_ms"], smemgpu.build_id(),
                                 T["busy_ms"], T["clock_check"], {"grid": st["grid"], "block": st["block"],
                                                                  "variant": gpu_variant}),
            "cpu_baseline": cpu,
            "parity_sample": parity,
            "streaming": srep,
            "sa_lookup": sa_rep,
            "chaining": chain_rep,
            "alignment": aln_rep,
            "sw_extension": sw_rep,
            "sa_load": {"s": round(t_sa, 3), "densify": os.environ.get("SMEM_GPU_DENSIFY", "hop"),
                        "what": ".sa upload (every 32nd row) + densification to every 4th row on the device, "
                                "synchronous"},
        })
    batch.close()
    gpu.close()
    # the product path end to end and the other genome profile: one GPU (the
    # driver's N=1 line), after the headline's GPU state is released
    if rank == 0 and world == 1:
        if args.e2e_reads > 0:
            out["e2e"] = e2e_report(args, genome_key(args), genome_codes, reads, cores, d.gpu)
            if out["e2e"] is not None and args.e2e_chunk_reads > 0:
                creads = make_reads(args, 0, genome_codes, 1, args.e2e_chunk_reads, salt=2)
                out["e2e"]["multi_chunk"] = e2e_chunks_report(args, genome_key(args), creads, cores, d.gpu)
                del creads
        if args.other_profile:
            del idx, sa
            held.clear()
            other = "uniform" if args.genome_profile == "human" else "human"
            out["uniform" if other == "uniform" else "human_like"] = profile_report(args, d, cores, other)


if __name__ == "__main__":
    main()
