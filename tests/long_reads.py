"""Reads of 321 bp to 70 kbp for the seeding, SA lookup and chaining tests
(tests/test_long_reads.py, tests/test_gpu_long_reads.py) and for the
tests/golden/long/ fixture (tests/golden/make_golden.py --long-only).

  class reads   two each of 321, 1000, 4095, 4096, 4097, 8191 and 8192 bp (the
                edges of the 13-bit query fields of the packed wire entry and
                one past them), one of 20,000 bp; either strand, 1 %
                substitutions, 0.05 % N
  chimera       about 70,000 collinear bases with 0.3 % substitutions (one chain
                whose weight passes 2^16), then three pieces of 200-300 bp from
                other loci, one of them reverse-complemented (chains of their own)

synthetic_reads() adds, on the planted genome of tests/test_gpu_seed_phases.py:

  long70k       three reads of 70,000 bp: thousands of intervals and hundreds of
                calls each
  gap           G[a:a+8000], 11,000 unrelated bases, G[a+19000:a+27000]: both
                parts on one diagonal 11,000 bases apart, so max_chain_gap 10000
                keeps two chains and 20000 merges them
  hp, di        a 5 kbp read centred on the homopolymer, exact for 400 bases to
                either side of the run's middle, and a 2 kbp read ending 20
                bases past the dinucleotide run, exact over its last 520 bases
                with a substitution before them: the match that covers the run
                has its middle inside it, so its re-seeding call starts there;
                1 % substitutions elsewhere
  empty, one    reads of 0 and 1 bp
  fill          100 reads of 150 bp
"""
import numpy as np

CLASS_LENGTHS = [321, 1000, 4095, 4096, 4097, 8191, 8192]
LONG_LEN = 20_000
CHIMERA_MAIN = 70_000
GAP_PART, GAP_JUNK = 8000, 11_000
# the synthetic chimera's collinear part: 150,700 .. 220,700 of the planted
# genome holds no copy of the repeat family and neither run, so no other
# chain's position falls inside it and mem_chain keeps it in one chain
CHIMERA_AT = 150_700


def _rc(r):
    r = np.asarray(r, np.uint8)
    return np.where(r < 4, 3 - r, r)[::-1].astype(np.uint8)


def _mutate(r, rng, sub, n_rate):
    r = np.array(r, dtype=np.uint8)
    hit = rng.random(r.size) < sub
    r[hit] = (r[hit] + rng.integers(1, 4, size=int(hit.sum()), dtype=np.uint8)) & 3
    r[rng.random(r.size) < n_rate] = 4
    return r


def _take(G, rng, n, sub=0.01, n_rate=0.0005):
    """n bases from a random place of G, either strand, with substitutions and N"""
    pos = int(rng.integers(0, G.size - n + 1))
    r = _mutate(G[pos:pos + n], rng, sub, n_rate)
    return _rc(r) if rng.random() < 0.5 else r


def chimera(G, rng, a=None):
    """CHIMERA_MAIN collinear bases from a (default: anywhere) with 0.3 %
    substitutions, then three pieces of 200-300 bp from loci at least 1000 bp
    away from them, the second one reverse-complemented"""
    if a is None:
        a = int(rng.integers(0, G.size - CHIMERA_MAIN + 1))
    parts = [_mutate(G[a:a + CHIMERA_MAIN], rng, 0.003, 0.0)]
    for k in range(3):
        n = int(rng.integers(200, 301))
        while True:
            p = int(rng.integers(0, G.size - n + 1))
            if p + n + 1000 < a or p > a + CHIMERA_MAIN + 1000:
                break
        piece = G[p:p + n].copy()
        parts.append(_rc(piece) if k == 1 else piece)
    return np.concatenate(parts).astype(np.uint8)


def class_reads(G, seed, chimera_at=None):
    """[(name, read)]: the length classes, the 20 kbp read and the chimera"""
    rng = np.random.default_rng(seed)
    out = []
    for n in CLASS_LENGTHS:
        for k in range(2):
            out.append((f"len{n}_{k}", _take(G, rng, n)))
    out.append((f"len{LONG_LEN}", _take(G, rng, LONG_LEN)))
    out.append(("chimera", chimera(G, rng, chimera_at)))
    return out


def gap_read(G, a, rng):
    junk = rng.integers(0, 4, size=GAP_JUNK).astype(np.uint8)
    far = a + GAP_PART + GAP_JUNK
    return np.concatenate([G[a:a + GAP_PART], junk, G[far:far + GAP_PART]]).astype(np.uint8)


def synthetic_reads(g, seed=511):
    """[(name, read)] on the planted genome g of test_gpu_seed_phases._genome"""
    from smemgpu import synth
    from test_gpu_seed_phases import DI0, DIN, HP0, HPN
    rng = np.random.default_rng(seed)
    out = class_reads(g, seed + 1, chimera_at=CHIMERA_AT)
    out += [(f"long70k_{k}", _take(g, rng, 70_000)) for k in range(3)]
    out.append(("gap", gap_read(g, 180_000, rng)))
    mid = HP0 + HPN // 2
    r = _mutate(g[mid - 2500:mid + 2500], rng, 0.01, 0.0)
    r[2100:2900] = g[mid - 400:mid + 400]
    out.append(("hp", r))
    d = DI0 + DIN
    r = _mutate(g[d + 20 - 2000:d + 20], rng, 0.01, 0.0)
    r[1480:] = g[d - 500:d + 20]
    r[1479] = (g[d - 501] + 1) & 3
    out.append(("di", r))
    out.append(("empty", np.zeros(0, np.uint8)))
    out.append(("one", g[777:778].copy()))
    fill = synth.make_reads(g, 100, 150, seed=seed + 2, sub_rate=0.02, n_rate=0.002)
    out += [(f"fill{i}", fill.read(i).copy()) for i in range(fill.n)]
    return out


def reads_of(named):
    """smemgpu.synth.Reads of [(name, read)] (or of plain arrays)"""
    from smemgpu import synth
    arrs = [x[1] if isinstance(x, tuple) else x for x in named]
    lens = np.array([a.size for a in arrs], np.int32)
    offs = np.concatenate([[0], np.cumsum(lens, dtype=np.int64)]).astype(np.int64)
    codes = np.concatenate([np.asarray(a, np.uint8) for a in arrs]) if arrs else np.zeros(0, np.uint8)
    return synth.Reads(lens, codes.astype(np.uint8), offs)


_world = None


def world():
    """The planted 300 kbp genome, its index and sampled SA from the host
    builder, the restatement's handles on them and the synthetic read set;
    made once per process.  truth(reads, **opt) keeps the restatement's
    streams, which no test changes."""
    global _world
    if _world is None:
        import smemgpu
        from oracle import oracle
        from test_gpu_seed_phases import _genome
        g = _genome()
        idx, sa = smemgpu.Index.build_sa(g, sa_intv=32)
        named = synthetic_reads(g)
        _world = dict(g=g, idx=idx, sa=sa, l_pac=idx.seq_len // 2, named=named, names=[n for n, _ in named],
                      reads=reads_of(named), seeded={},
                      oi=oracle.OracleIndex(words=idx.words, primary=idx.primary, L2=idx.L2),
                      osa=oracle.OracleSA(sa=sa.samples, sa_intv=32, seq_len=idx.seq_len))
    return _world


def seed_truth(w, key, reads, **opt):
    """oracle.seed of `reads` under opt, kept under (key, opt): (stream, per-read counts, counters)"""
    from oracle import oracle
    k = (key, tuple(sorted(opt.items())))
    if k not in w["seeded"]:
        w["seeded"][k] = oracle.seed(w["oi"], reads.codes, reads.offs, threads=4, **opt)
    return w["seeded"][k]


def sa_truth(oi, osa, lists, min_seed_len, max_occ):
    """(per-read counts, per-read bwt_sa positions) of the restatement for [read][call] lists"""
    from oracle import oracle
    counts, k = oracle.sa_queries(lists, min_seed_len, max_occ)
    pos = osa.lookup(oi, k)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return counts, [pos[off[i]:off[i + 1]] for i in range(len(lists))]


def chain_truth(oi, osa, lists, l_pac, min_seed_len=19, max_occ=10000, **kw):
    """the restatement's SMCH stream for [read][call] lists (its own bwt_sa positions)"""
    from oracle import oracle
    _, pos = sa_truth(oi, osa, lists, min_seed_len, max_occ)
    seeds, off = oracle.chain_seeds(lists, pos, min_seed_len, max_occ)
    return oracle.chain(seeds, off, l_pac, min_seed_len=min_seed_len, threads=4, **kw)


def chain_weight(seeds):
    """mem_chain_weight (software/bwamem.c:501-521), loop for loop: the query
    bases the seeds cover, then the same walk over rbeg that goes on adding to
    w and moves its end by the query coordinates, and the smaller of the two"""
    w = end = 0
    for s in seeds:
        qb, n = int(s["qbeg"]), int(s["len"])
        if qb >= end:
            w += n
        elif qb + n > end:
            w += qb + n - end
        end = max(end, qb + n)
    tmp, end = w, 0
    for s in seeds:
        rb, qb, n = int(s["rbeg"]), int(s["qbeg"]), int(s["len"])
        if rb >= end:
            w += n
        elif rb + n > end:
            w += rb + n - end
        end = max(end, qb + n)
    return min(w, tmp)
