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

build and build_fr are the first groups; build_edges adds what they never reach
(lists past 64 regions and at the limit, roll-back after an insertion, both ends
rescued, N in the mate, l_pac no multiple of 4, windows at the limit, equal
scores, short mates).  fixtures() names every batch whose result under the
reference's own mem_matesw is kept in tests/golden/msw/hand.
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


# ---- the edges: what the groups above never reach -------------------------------------------------
_OFF = matesw_ref.Pes(0, 0, 1)
PES_ROLL = [_OFF, matesw_ref.Pes(LOW, HIGH, 0), _OFF, matesw_ref.Pes(LOW, 2100, 0)]   # RR windows of 2000 + l_ms bases
PES_WIN = [_OFF, matesw_ref.Pes(LOW, LOW + 1898, 0), _OFF, _OFF]                     # FR windows of 1898 + l_ms bases
LONG_SIZES = (63, 64, 65, 128, 129, 1000, 1022, 1023, 1024)
L_PAC_ODD = (200_001, 200_002, 200_003)
SHORT_SIZES = (1, 18, 19, 20, 249, 250, 256)


@dataclass
class Case:
    """a batch of pairs with the bounds and options it was built for"""
    pes: list
    opt: matesw_ref.Opt
    pairs: Pairs


def genome_odd(l_pac):
    """the first l_pac bases of a second genome of 200 003: the last .pac byte is partly filled"""
    return np.random.default_rng(2204).integers(0, 4, size=max(L_PAC_ODD)).astype(np.uint8)[:l_pac].copy()


def long_list(n, at, twins, hit=150, base=120_000, run=8):
    """n regions of 30 bases, 40 apart on the forward strand from `base` on -- far from every anchor, and
    no two of them redundant -- with scores that descend in runs of `run` equals, the first score below
    `hit` at index `at`.  With twins every eighth region is its predecessor moved by one base, with the
    same end and score: the two are redundant, and which of them mem_sort_and_dedup keeps hangs on the
    order in which the unstable sort by `re` met them, so on the list's order after the insertion."""
    out = []
    for k in range(n):
        sc = hit + (at - 1 - k) // run if k < at else hit - 1 - (k - at) // run
        rb, qb = base + 40 * k, 35 * (k % 4)
        r = region(rb, rb + 30, qb, qb + 30, sc)
        if twins and k % 8 == 7:
            t = out[-1]
            r = region(t["rb"] + 1, t["re"], t["qb"] + 1, t["qe"], t["score"])
        out.append(r)
    return out


def build_edges(G, l_pac):
    """name -> Case.  Every anchor and mate is placed by rule, none at random, apart from substitutions.
    long      the mate's list holds LONG_SIZES regions (long_list); the rescued hit scores 150 exactly and
              goes in at an index named per size.  PES_FR, max_matesw = 2.  Groups long_<n>; then pairs
              of two anchors and a mate whose halves match behind one anchor each, so both insert:
              two_1022 (ends at MAX_REGS), two_1023_host (the second passes it), two_1023_twin (a pair of
              twins in the list: the first dedup drops one and the second fits) and long_1024_host
    roll      FR ordinary, RR wide: roll_window inserts and sorts at r = 1 and meets the window limit at
              r = 3; roll_second has RR found for end 0's anchor, whose FR rescue changes end 1's list,
              and the limit is met from end 1's anchor
    both      each end has a region of its first half, 50 kbp apart, and its second half matches unseeded
              in FR bounds of the other end's region: both lists gain a region
    n         1, 5 and 30 N in the mate, placed FF (as it is) and FR (reverse-complemented), with an N at
              q = 0 and at q = l_ms - 1.  PES_ALL
    lpac      windows that end at l_pac, start at l_pac, end at l_pac + 1 and are cut at 2 l_pac; the
              mates are the last 150 bases of the forward strand and the first 150 of the reverse.  PES_ALL
    window    FR bounds 1898 apart: a mate of 150 gives 2048 rows, one of 151 gives 2049, one of 202 near
              position 0 gives 2100 cut to 2028
    equal     the mate's list holds two (and a lower third) regions of the score the SW returns
    short     mates of SHORT_SIZES bases: around min_seed_len, around the byte / word switch at 250, and the longest"""
    Opt = matesw_ref.Opt
    L = 150
    two = 2 * l_pac

    def fwd(p, n=L):
        return G[p:p + n].copy(), region(p, p + n, 0, n, n)

    def rev(q, n=L):
        return rc(G[q:q + n]), region(two - (q + n), two - q, 0, n, n)

    cases = {}

    P = Pairs()
    ats = {63: 40, 64: 64, 65: 64, 128: 72, 129: 100, 1000: 700, 1022: 900, 1023: 950, 1024: 70}
    for k, n in enumerate(LONG_SIZES):
        p = 10_000 + 1_000 * k
        a, la = fwd(p)
        m, _ = rev(p + 400 - L + 1)
        P.add(f"long_{n}" + ("_host" if n == 1024 else ""), a, [la], m, long_list(n, ats[n], n < 1000))

    def two_anchors(name, p, lst):
        a, la = fwd(p)
        lb = region(p + 50_000, p + 50_000 + L, 0, L, L - 5)
        halves = np.concatenate([G[p + 300:p + 375], G[p + 50_300:p + 50_375]])
        P.add(name, a, [la, lb], rc(halves), lst)

    two_anchors("two_1022", 20_000, long_list(1022, 900, False, hit=75))
    two_anchors("two_1023_host", 21_000, long_list(1023, 900, False, hit=75))
    twin = long_list(1023, 900, False, hit=75)
    t = twin[500]
    twin[501] = region(t["rb"] + 1, t["re"], t["qb"] + 1, t["qe"], t["score"])
    two_anchors("two_1023_twin", 22_000, twin)
    cases["long"] = Case(PES_FR, Opt(max_matesw=2), P)

    P = Pairs()
    far = lambda: region(150_000, 150_060, 0, 60, 60)
    for k in range(3):
        p = 30_000 + 1_000 * k
        a, la = fwd(p)
        m, _ = rev(p + 300 + 100 * k - L + 1)
        P.add("roll_window", a, [la], m, [far()])
    for k in range(2):
        p = 40_000 + 1_000 * k
        a, la = fwd(p)
        m, _ = rev(p + 350 - L + 1)
        P.add("roll_second", a, [la], m, [region(p - 500, p - 440, 0, 60, 60)])
    cases["roll"] = Case(PES_ROLL, Opt(), P)

    P = Pairs()
    for k in range(3):
        p = 50_000 + 1_000 * k
        x = p + 50_000
        r0 = np.concatenate([G[p:p + 75], rc(G[x + 300:x + 375])])
        r1 = np.concatenate([rc(G[p + 300:p + 375]), G[x:x + 75]])
        P.add("both", r0, [region(p, p + 75, 0, 75, 75)], r1, [region(x, x + 75, 75, 150, 75)])
    cases["both"] = Case(PES_FR, Opt(), P)

    P = Pairs()
    at_n = {1: ([0], [L - 1]), 5: ([0, 31, 77, 78, L - 1],) * 2, 30: ([0, L - 1] + list(range(20, 132, 4)),) * 2}
    for k, n in enumerate((1, 5, 30)):
        for o, name in enumerate(("FF", "FR")):
            p = 60_000 + 2_000 * k + 1_000 * o
            a, la = fwd(p)
            m = fwd(p + 400)[0] if name == "FF" else rev(p + 400 - L + 1)[0]
            assert len(at_n[n][o]) == n
            m[at_n[n][o]] = 4
            P.add(f"n_{n}_{name}", a, [la], m, [])
    cases["n"] = Case(PES_ALL, Opt(), P)

    P = Pairs()
    last_rev, last_fwd = rc(G[l_pac - L:l_pac]), G[l_pac - L:l_pac].copy()   # the hit [l_pac - 150, l_pac), either strand
    a, la = fwd(l_pac - HIGH)                           # FR: [.., rb + HIGH) ends at l_pac
    P.add("ends_at_l_pac", a, [la], last_rev, [])
    a, la = rev(l_pac - HIGH - L)                       # rb = l_pac + HIGH; RR: [rb - HIGH, ..) starts at l_pac
    P.add("starts_at_l_pac", a, [la], last_rev, [])
    a, la = fwd(l_pac - HIGH + 1)                       # FR: ends at l_pac + 1, bridged
    P.add("ends_past_l_pac", a, [la], last_rev, [])
    a, la = rev(L)                                      # rb = 2 l_pac - 300; FR: cut at 2 l_pac, the hit [0, 150)
    P.add("clip_2l", a, [la], G[:L].copy(), [])
    a, la = rev(l_pac - 50 - L)                         # rb = l_pac + 50; FR: [rb + LOW - 150, ..) starts at l_pac
    P.add("starts_at_l_pac_fr", a, [la], last_fwd, [])
    cases["lpac"] = Case(PES_ALL, Opt(), P)

    P = Pairs()
    for k in range(2):
        p = 70_000 + 3_000 * k
        a, la = fwd(p)
        P.add("win_2048", a, [la], rev(p + 1_000 - 150 + 1, 150)[0], [])
        a, la = fwd(p + 10_000)
        P.add("win_2049", a, [la], rev(p + 11_000 - 151 + 1, 151)[0], [])
        a, la = fwd(30 + 10 * k)
        P.add("win_clip0", a, [la], rev(800 + 100 * k, 202)[0], [])
    cases["window"] = Case(PES_WIN, Opt(), P)

    P = Pairs()
    for k in range(3):
        p = 80_000 + 1_000 * k
        a, la = fwd(p)
        m, _ = rev(p + 400 - L + 1)
        lst = [region(130_000, 130_000 + L, 0, L, L), region(140_000, 140_000 + L, 0, L, L)]
        if k:
            lst.append(region(145_000, 145_100, 0, 100, 100))
        P.add("equal", a, [la], m, lst)
    cases["equal"] = Case(PES_FR, Opt(), P)

    P = Pairs()
    for k, n in enumerate(SHORT_SIZES):
        p = 85_000 + 1_000 * k
        a, la = fwd(p)
        P.add(f"short_{n}", a, [la], rev(p + 400 - n + 1, n)[0], [])
    cases["short"] = Case(PES_FR, Opt(), P)
    return cases


EDGE_SIZES = {
    "long": dict({f"long_{n}": 1 for n in LONG_SIZES[:-1]}, long_1024_host=1, two_1022=1, two_1023_host=1,
                 two_1023_twin=1),
    "roll": {"roll_window": 3, "roll_second": 2},
    "both": {"both": 3},
    "n": {f"n_{n}_{o}": 1 for n in (1, 5, 30) for o in ("FF", "FR")},
    "lpac": {"ends_at_l_pac": 1, "starts_at_l_pac": 1, "ends_past_l_pac": 1, "clip_2l": 1, "starts_at_l_pac_fr": 1},
    "window": {"win_2048": 2, "win_2049": 2, "win_clip0": 2},
    "equal": {"equal": 3},
    "short": {f"short_{n}": 1 for n in SHORT_SIZES},
}

# ---- the reference's own mem_matesw on these batches (ref_harness msw) ---------------------------
OPTS = {"base": {}, "a2": dict(a=2, b=8, o_del=12, e_del=2, o_ins=12, e_ins=2), "one_anchor": dict(max_matesw=1),
        "no_margin": dict(pen_unpaired=0), "no_anchor": dict(max_matesw=0)}


def fixtures():
    """name -> (G, l_pac, Case): every batch tests/golden/msw/hand holds the reference's result for.  build and
    build_fr under every set of OPTS; each case of build_edges as built, under -A 2 scaling and with one anchor
    an end; and the lpac case on the genomes whose length is no multiple of 4."""
    import dataclasses
    G = genome()
    out = {}
    for o, kw in OPTS.items():
        out[f"all_{o}"] = (G, L_PAC, Case(PES_ALL, matesw_ref.Opt(**kw), build(G)))
        out[f"fr_{o}"] = (G, L_PAC, Case(PES_FR, matesw_ref.Opt(**kw), build_fr(G)))
    for name, c in build_edges(G, L_PAC).items():
        out[f"{name}_base"] = (G, L_PAC, c)
        for o in ("a2", "one_anchor"):
            out[f"{name}_{o}"] = (G, L_PAC, Case(c.pes, dataclasses.replace(c.opt, **OPTS[o]), c.pairs))
    for l in L_PAC_ODD:
        g = genome_odd(l)
        out[f"lpac{l}_base"] = (g, l, build_edges(g, l)["lpac"])
    return out


def smmi_bytes(G, l_pac, case):
    """the input of `ref_harness msw` (SMMI, oracle/ref_harness.c) for a batch"""
    import struct
    o = case.opt
    codes, offs, regs, reg_off = case.pairs.arrays()
    pac = pack(G)
    assert pac.size == (l_pac + 3) // 4 and regs.dtype.itemsize == 64
    head = b"SMMI0001" + struct.pack("<q", l_pac)
    head += struct.pack("<12i", *[v for p in case.pes for v in (p.low, p.high, p.failed)])
    head += struct.pack("<10i", o.a, o.b, o.o_del, o.e_del, o.o_ins, o.e_ins, o.min_seed_len, o.pen_unpaired, o.max_matesw, 0)
    head += struct.pack("<f", o.mask_level_redun)
    head += struct.pack("<4Q", len(case.pairs.group), pac.size, codes.size, regs.size)
    return head + pac.tobytes() + codes.tobytes() + offs.astype("<u8").tobytes() + reg_off.astype("<u8").tobytes() + \
        regs.tobytes()


def smmo_parse(data):
    """the output of `ref_harness msw` (SMMO) -> (regions as ALNREG_DT, reg_off, n per pair)"""
    import struct
    from smemgpu.lib import ALNREG_DT
    assert data[:8] == b"SMMO0001"
    n_pairs, n_regs = struct.unpack_from("<2Q", data, 8)
    at = 24
    n = np.frombuffer(data, dtype="<i4", count=n_pairs, offset=at)
    at += 4 * n_pairs
    reg_off = np.frombuffer(data, dtype="<u8", count=2 * n_pairs + 1, offset=at)
    at += 8 * (2 * n_pairs + 1)
    regs = np.frombuffer(data, dtype=ALNREG_DT, count=n_regs, offset=at)
    assert at + 64 * n_regs == len(data) and int(reg_off[-1]) == n_regs
    return regs, reg_off, n
