"""Reads and option sets for the chains -> regions tests under non-default
`bwa mem` extension options (-d / -L / -B / -O / -E / -A / -w / -k).

The r1 / r2 golden reads carry substitutions only: a moderate z-drop never
fires on them and the clip penalty decides almost nothing.  option_reads()
makes the shapes on which each option decides the region:

  indel   2-3 % substitutions plus 1-3 indels of 1-40 bp (gap penalties, band)
  junk    two matching parts around 20-45 unrelated bases on (nearly) one
          diagonal: the extension runs through or stops by z-drop and b
  ends    the first or last 3-12 bases hold 1-3 mismatches: the clip penalty
          decides between a local end and an end-to-end alignment
  tail    30-60 unrelated bases at one end
  long    600-1000 bp with indels, mismatched ends, sometimes a tail, and 90-115
          unrelated bases at least 220 bp from either end (60 under 560 bp), where zdrop 100
          decides: across J unrelated bases the row maximum of ksw_extend2
          first follows the deletion that skips them, which the z-drop test
          forgives (it subtracts the distance from the diagonal), and comes
          back to the diagonal about 1.6 J below the maximum, so zdrop 100
          fires from J ~ 85 on, and both sides must score more than that drop
          for the run-through to win with z-drop off (-d 0).  No read of
          320 bp or less has room for that.

tests/golden/make_golden.py writes the r3 / r4 read sets with it and
tests/test_aln.py makes fresh problems of the same mix.
"""
import numpy as np

# name -> the mem_opt_t fields that differ from mem_opt_init's (a 1, b 4, gaps
# 6 + 1 both, zdrop 100, clip 5 / 5, w 100, min_seed_len 19).  Values are
# literal: no -A scaling.
OPTION_SETS = {
    "default": {},
    "d0": dict(zdrop=0),
    "d20": dict(zdrop=20),
    "d1": dict(zdrop=1),
    "L0": dict(pen_clip5=0, pen_clip3=0),
    "L0_9": dict(pen_clip5=0, pen_clip3=9),
    "L9_0": dict(pen_clip5=9, pen_clip3=0),
    "L30": dict(pen_clip5=30, pen_clip3=30),
    "B1": dict(b=1),
    "B9": dict(b=9),
    "gaps": dict(o_del=5, e_del=3, o_ins=8, e_ins=2),
    "A3": dict(a=3, b=5, o_del=7, e_del=2, o_ins=9, e_ins=3, zdrop=300, pen_clip5=15, pen_clip3=15),
    "A100": dict(a=100, b=100, o_del=127, e_del=100, o_ins=127, e_ins=100, zdrop=10000, pen_clip5=500,
                 pen_clip3=500),
    "w1": dict(w=1),
    "w7": dict(w=7),
    "k10": dict(min_seed_len=10),
}
DEFAULTS = dict(w=100, min_seed_len=19, a=1, b=4, o_del=6, e_del=1, o_ins=6, e_ins=1, zdrop=100, pen_clip5=5,
                pen_clip3=5)


def full_options(name: str) -> dict:
    """every field of the option set (what the manifest records)"""
    return dict(DEFAULTS, **OPTION_SETS[name])


def _rand(rng, n):
    return rng.integers(0, 4, size=int(n)).astype(np.uint8)


def _subs(r, rng, rate):
    r = r.copy()
    hit = rng.random(r.size) < rate
    r[hit] = (r[hit] + rng.integers(1, 4, size=int(hit.sum())).astype(np.uint8)) & 3
    return r


def _indels(r, rng, n, lo=1, hi=40):
    """n indels of lo..hi bp, insertions of unrelated bases or deletions, each at
    least 25 bp from the ends"""
    for _ in range(n):
        k = int(rng.integers(lo, hi + 1))
        if r.size < 60 + k:
            break
        at = int(rng.integers(25, r.size - 25 - k + 1))
        if rng.random() < 0.5:
            r = np.concatenate([r[:at], _rand(rng, k), r[at:]])
        else:
            r = np.concatenate([r[:at], r[at + k:]])
    return r


def _junk(r, rng, lo=20, hi=45, margin=30):
    """lo..hi unrelated bases in place of as many (+-3) of the read's, at least margin bp from the ends"""
    k = int(rng.integers(lo, hi + 1))
    d = int(rng.integers(-3, 4)) if rng.random() < 0.4 else 0
    cut = max(1, k + d)
    if r.size < 2 * margin + cut + 2:
        return r
    at = int(rng.integers(margin, r.size - margin - cut + 1))
    return np.concatenate([r[:at], _rand(rng, k), r[at + cut:]])


def _end_mismatches(r, rng):
    """1-3 mismatches within the first or the last 3-12 bases"""
    r = r.copy()
    span = int(rng.integers(3, 13))
    n = int(rng.integers(1, 4))
    pos = rng.choice(span, size=min(n, span), replace=False)
    if rng.random() < 0.5:
        pos = r.size - 1 - pos
    r[pos] = (r[pos] + rng.integers(1, 4, size=pos.size).astype(np.uint8)) & 3
    return r


def _tail(r, rng):
    t = _rand(rng, rng.integers(30, 61))
    return np.concatenate([t, r]) if rng.random() < 0.5 else np.concatenate([r, t])


def one_read(G, rng, kind: str, length: int) -> np.ndarray:
    """one read of `kind` cut from genome codes G (either strand), about `length` bp"""
    span = min(G.size, length + 60)
    pos = int(rng.integers(0, G.size - span + 1))
    src = G[pos:pos + span]
    if rng.random() < 0.5:
        src = (3 - src)[::-1]
    r = np.ascontiguousarray(src[:length]).astype(np.uint8)
    if kind == "indel":
        r = _indels(_subs(r, rng, float(rng.uniform(0.02, 0.03))), rng, int(rng.integers(1, 4)))
    elif kind == "junk":
        r = _junk(_subs(r, rng, 0.01), rng)
    elif kind == "ends":
        r = _end_mismatches(_subs(r, rng, 0.005), rng)
    elif kind == "tail":
        r = _tail(_subs(r, rng, 0.02), rng)
    elif kind == "long":
        r = _indels(_subs(r, rng, 0.01), rng, int(rng.integers(1, 3)), 1, 12)
        r = _end_mismatches(_junk(r, rng, 90, 115, 220 if r.size >= 560 else 60), rng)
        if rng.random() < 0.5:
            r = _tail(r, rng)
    else:
        raise ValueError(kind)
    return r


KINDS = ("indel", "junk", "ends", "tail")


def option_reads(G, n: int, seed: int, len_range=(60, 320), n_long: int = 28, long_range=(600, 1000),
                 max_len: int = 0):
    """n reads of len_range bp cycling through KINDS plus n_long "long" reads,
    shuffled; max_len > 0 cuts every read to that many bases.  Returns
    smemgpu.synth.Reads."""
    from smemgpu import synth
    rng = np.random.default_rng(seed)
    parts = []
    for i in range(n):
        kind = KINDS[i % len(KINDS)]
        # room for what the kind adds, so the read stays inside len_range
        grow = {"indel": 0, "junk": 3, "ends": 0, "tail": 60}[kind]
        lo, hi = len_range[0], max(len_range[0], len_range[1] - grow)
        r = one_read(G, rng, kind, int(rng.integers(lo, hi + 1)))
        parts.append(r[:len_range[1]])
    for _ in range(n_long):
        r = one_read(G, rng, "long", int(rng.integers(long_range[0], long_range[1] - 100)))
        parts.append(r[:long_range[1]])
    order = rng.permutation(len(parts))
    parts = [parts[int(k)][:max_len] if max_len else parts[int(k)] for k in order]
    lens = np.array([p.size for p in parts], dtype=np.int32)
    return synth.Reads(lens, np.concatenate(parts).astype(np.uint8),
                       np.concatenate([[0], np.cumsum(lens, dtype=np.int64)]))
