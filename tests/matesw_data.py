"""The hand-built pairs of the mate-rescue tests: one group per branch of
mem_matesw (software/bwamem_pair.c:109-175) and of the loop around it (:252-263),
on a 200 kbp genome of two contigs.  Each pair's regions are written by hand --
a read copied from position p gets the region a full-length hit would give --
so a group controls exactly which end has regions and where.

Orientations (mem_infer_dir, :23-30), for an anchor on the forward strand at p:
  0 FF  the mate on the same strand, further along
  1 FR  the mate reverse-complemented, further along
  2 RF  the mate reverse-complemented, behind the anchor
  3 RR  the mate on the same strand, behind the anchor
"""
from dataclasses import dataclass, field

import numpy as np

from tests import matesw_ref, regfin_ref

L_PAC = 200_000
CONTIGS = [(0, 120_000), (120_000, 80_000)]   # (offset, length): the stage reads l_pac only
LOW, HIGH = 100, 700
PES_ALL = [matesw_ref.Pes(LOW, HIGH, 0) for _ in range(4)]
PES_FR = [matesw_ref.Pes(0, 0, 1), matesw_ref.Pes(LOW, HIGH, 0), matesw_ref.Pes(0, 0, 1), matesw_ref.Pes(0, 0, 1)]
PES_WIDE = [matesw_ref.Pes(LOW, 3000, 0) for _ in range(4)]   # windows of 2900 + l_ms bases: past MAX_TLEN


def rc(x):
    return np.where(x < 4, 3 - x, 4)[::-1].astype(np.uint8)


def genome():
    rng = np.random.default_rng(2201)
    g = rng.integers(0, 4, size=L_PAC).astype(np.uint8)
    return g


def pack(codes):
    c = np.concatenate([codes, np.zeros((-codes.size) % 4, np.uint8)]).reshape(-1, 4).astype(np.uint8)
    return (c[:, 0] << 6 | c[:, 1] << 4 | c[:, 2] << 2 | c[:, 3]).astype(np.uint8)


def region(rb, re, qb, qe, score):
    r = {k: 0 for k in regfin_ref.FIELDS}
    r.update(rb=int(rb), re=int(re), qb=int(qb), qe=int(qe), score=int(score), truesc=int(score), w=100,
             seedcov=int(qe - qb))
    return r


def fwd_read(G, p, L):
    """(read, its full-length region) for a read copied from the forward strand at p"""
    return G[p:p + L].copy(), region(p, p + L, 0, L, L)


def rev_read(G, q, L):
    """the same for the reverse complement of G[q:q + L]"""
    return rc(G[q:q + L]), region(2 * L_PAC - (q + L), 2 * L_PAC - q, 0, L, L)


@dataclass
class Pairs:
    reads: list = field(default_factory=list)     # 2 per pair
    lists: list = field(default_factory=list)     # 2 per pair
    group: list = field(default_factory=list)     # 1 per pair

    def add(self, name, r0, l0, r1, l1):
        self.reads += [r0, r1]
        self.lists += [l0, l1]
        self.group.append(name)

    def arrays(self):
        from smemgpu.lib import ALNREG_DT
        offs = np.concatenate([[0], np.cumsum([r.size for r in self.reads])]).astype(np.uint64)
        codes = np.concatenate(self.reads).astype(np.uint8)
        reg_off = np.concatenate([[0], np.cumsum([len(x) for x in self.lists])]).astype(np.uint64)
        regs = np.zeros(int(reg_off[-1]), dtype=ALNREG_DT)
        k = 0
        for lst in self.lists:
            for r in lst:
                for f in regfin_ref.FIELDS:
                    regs[k][f] = r[f]
                k += 1
        return codes, offs, regs, reg_off

    def of(self, name):
        return [p for p, g in enumerate(self.group) if g == name]


def mutate(x, rng, rate):
    x = x.copy()
    hit = rng.random(x.size) < rate
    x[hit] = (x[hit] + rng.integers(1, 4, size=int(hit.sum()))) & 3
    return x.astype(np.uint8)


def build(G):
    """the pairs for PES_ALL (every orientation open, bounds LOW..HIGH)"""
    rng = np.random.default_rng(2202)
    P = Pairs()
    L = 150
    mid = lambda: int(rng.integers(5_000, 90_000))

    # the mate unseeded and placed in each orientation: four SWs from the one anchor, one finds it
    for r, name in enumerate(("FF", "FR", "RF", "RR")):
        for _ in range(10):
            p = mid()
            d = int(rng.integers(LOW + 160, HIGH - 160))
            a, la = fwd_read(G, p, L)
            if r == 0:
                m, _ = fwd_read(G, p + d, L)
            elif r == 1:
                m, _ = rev_read(G, p + d - L + 1, L)       # dist = q + L - 1 - p = d
            elif r == 2:
                m, _ = rev_read(G, p - d - L + 1, L)       # p2 = q + L - 1 = p - d
            else:
                m, _ = fwd_read(G, p - d, L)
            P.add("rescue_" + name, a, [la], mutate(m, rng, 0.03), [])
    # the same with the pair's ends swapped: the anchor is end 1, the rescue goes into a[0]
    for _ in range(10):
        p = mid()
        d = int(rng.integers(LOW + 160, HIGH - 160))
        a, la = fwd_read(G, p, L)
        m, _ = rev_read(G, p + d - L + 1, L)
        P.add("rescue_end0", mutate(m, rng, 0.03), [], a, [la])
    # a reverse-strand anchor (its mate forward, behind it on the forward strand)
    for _ in range(10):
        q = mid()
        d = int(rng.integers(LOW + 160, HIGH - 160))
        a, la = rev_read(G, q, L)
        m, _ = fwd_read(G, q + L - 1 - d, L)
        P.add("rescue_rev_anchor", a, [la], mutate(m, rng, 0.03), [])
    # anchors within HIGH of position 0 and of 2 l_pac: windows cut at the ends
    for _ in range(10):
        p = int(rng.integers(0, HIGH - 100))
        d = int(rng.integers(LOW + 160, HIGH - 160))
        a, la = fwd_read(G, p, L)
        m, _ = rev_read(G, p + d - L + 1, L)
        P.add("clip_0", a, [la], mutate(m, rng, 0.03), [])
    for _ in range(10):
        q = int(rng.integers(0, HIGH - 300))      # the anchor's rb = 2 l_pac - (q + L)
        d = int(rng.integers(LOW + 160, HIGH - 160))
        a, la = rev_read(G, q, L)
        m, _ = fwd_read(G, max(0, q + L - 1 - d), L)
        P.add("clip_2l", a, [la], mutate(m, rng, 0.03), [])
    # an anchor just below l_pac: the windows ahead of it bridge l_pac (no SW, n unchanged)
    for _ in range(10):
        p = L_PAC - int(rng.integers(LOW + 200, HIGH))
        a, la = fwd_read(G, p, L)
        m, _ = rev_read(G, p - 400, L)
        P.add("bridge", a, [la], mutate(m, rng, 0.03), [])
    # a mate that matches nowhere: every SW stays below min_seed_len, nothing is inserted, n counts
    for _ in range(10):
        a, la = fwd_read(G, mid(), L)
        P.add("below", a, [la], rng.integers(0, 4, size=L).astype(np.uint8), [])
    # no region on either end
    for _ in range(5):
        a, _ = fwd_read(G, mid(), L)
        b, _ = fwd_read(G, mid(), L)
        P.add("empty", a, [], b, [])
    # a 250 bp mate: 16-bit scores at a = 1
    for _ in range(10):
        p = mid()
        d = int(rng.integers(LOW + 260, HIGH - 10))
        a, la = fwd_read(G, p, 250)
        m, _ = rev_read(G, p + d - 250 + 1, 250)
        P.add("long250", a, [la], mutate(m, rng, 0.03), [])
    # an existing partial hit of the mate that starts outside the bounds although the full hit is inside:
    # the SW runs, finds the full hit, and mem_sort_and_dedup drops the partial one (lower score) ...
    for _ in range(10):
        p = mid()
        a, la = fwd_read(G, p, L)
        q = p + LOW + 20 - L + 1                          # full hit: dist = LOW + 20
        m, lm = rev_read(G, q, L)
        part = region(lm["rb"] + 50, lm["re"], 50, L, 100)   # query [50, 150): dist = LOW - 30
        P.add("dedup_drops_old", a, [la], m, [part])
    # ... or drops the rescued hit, when the existing one claims a higher score
    for _ in range(10):
        p = mid()
        a, la = fwd_read(G, p, L)
        q = p + LOW + 2 - L + 1                           # full hit: dist = LOW + 2
        m, lm = rev_read(G, q, L)
        part = region(lm["rb"] + 5, lm["re"], 5, L, 200)      # dist = LOW - 3, score above any SW's
        P.add("dedup_drops_new", a, [la], mutate(m, rng, 0.02), [part])
    # a 300 bp mate: left to the host
    for _ in range(3):
        p = mid()
        a, la = fwd_read(G, p, L)
        m, _ = rev_read(G, p + 200, 300)
        P.add("host_300", a, [la], m, [])
    return P


def build_fr(G):
    """the pairs for PES_FR (only FR open)"""
    rng = np.random.default_rng(2203)
    P = Pairs()
    L = 150
    mid = lambda: int(rng.integers(5_000, 90_000))
    # both ends seeded and consistent: no SW, the lists as they came
    for _ in range(20):
        p = mid()
        d = int(rng.integers(LOW + 160, HIGH - 10))
        a, la = fwd_read(G, p, L)
        m, lm = rev_read(G, p + d - L + 1, L)
        extra = region(int(rng.integers(100_000, 110_000)), 0, 0, 60, 60)
        extra["re"] = extra["rb"] + 60
        P.add("consistent", a, [la, extra], m, [lm])
    # a tandem duplicate: two anchors 200 bp apart, equal scores; the hit the first rescues is in bounds
    # for the second, whose mem_matesw returns at once
    for _ in range(10):
        p = mid()
        a, la = fwd_read(G, p, L)
        lb = region(p + 200, p + 200 + L, 0, L, L - int(rng.integers(0, 10)))
        m, _ = rev_read(G, p + 450 - L + 1, L)
        P.add("second_anchor_skips", a, [la, lb], mutate(m, rng, 0.03), [])
    # two anchors far apart within pen_unpaired: both run their SW, the second finds nothing
    for _ in range(10):
        p = mid()
        a, la = fwd_read(G, p, L)
        lb = region(p + 50_000, p + 50_000 + L, 0, L, L - 10)
        lc = region(p + 60_000, p + 60_000 + L, 0, L, L - 40)     # below the floor of pen_unpaired = 17
        m, _ = rev_read(G, p + 450 - L + 1, L)
        P.add("two_anchors", a, [la, lb, lc], mutate(m, rng, 0.03), [])
    # the mate unseeded, in FR: one SW
    for _ in range(10):
        p = mid()
        d = int(rng.integers(LOW + 160, HIGH - 160))
        a, la = fwd_read(G, p, L)
        m, _ = rev_read(G, p + d - L + 1, L)
        P.add("rescue_FR", a, [la], mutate(m, rng, 0.03), [])
    return P
