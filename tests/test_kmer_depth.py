"""The host's two choices for the seeding kernel's virtual short entries, on hand-made level tables (no
GPU): smem_kmer_depth (D from the per-level minimum sizes) and smem_kmer_call_depth (a call's probe
depth from D, minsz and its min_intv)."""
import numpy as np


def _mn(levels):
    a = np.zeros(16, np.uint64)
    a[1:1 + len(levels)] = levels
    return a


def _depth(levels, k=None):
    import smemgpu
    a = _mn(levels)
    return smemgpu.load().smem_kmer_depth(a.ctypes.data, len(levels) if k is None else k)


def _call(levels, d, min_intv):
    import smemgpu
    a = _mn(levels)
    return smemgpu.load().smem_kmer_call_depth(a.ctypes.data, d, min_intv)


def test_depth_needs_the_next_level_complete():
    # every level complete: the deepest one only vouches for the level before it
    assert _depth([900, 200, 50, 9, 2]) == 4
    assert _depth([900]) == 0
    # a missing string at level 3: levels 1, 2 are complete, so strings of 1 base always shrink
    assert _depth([900, 200, 0, 0, 0]) == 1
    # ... at level 2: nothing may be skipped; at level 1 (a letter absent from the index) neither
    assert _depth([900, 0, 0]) == 0
    assert _depth([0, 0, 0]) == 0
    # a table cut short by k is judged on its k levels
    assert _depth([900, 200, 50, 9, 2], k=3) == 2
    assert _depth([900, 200, 50, 9, 2], k=15) == 4
    # a level after a gap does not count (cannot happen in a real table: minima do not increase)
    assert _depth([900, 0, 50, 9]) == 0


def test_call_depth_follows_min_intv():
    lv = [900, 200, 50, 9, 2, 0]
    d = _depth(lv)
    assert d == 4
    assert _call(lv, d, 1) == 4          # minsz[4] = 9 >= 1
    assert _call(lv, d, 0) == 4 and _call(lv, d, -3) == 4   # bwt_smem1 raises min_intv to 1
    assert _call(lv, d, 9) == 4          # equal: the size may touch min_intv
    assert _call(lv, d, 10) == 3         # minsz[4] below, minsz[3] = 50 above
    assert _call(lv, d, 51) == 2
    assert _call(lv, d, 201) == 1        # below 2: the kernel runs the plain path
    assert _call(lv, d, 901) == 0
    assert _call(lv, 0, 1) == 0
    assert _call(lv, 2, 1) == 2          # never past D
