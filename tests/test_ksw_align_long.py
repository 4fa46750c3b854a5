"""ksw_align2 (software/ksw.c:342-364) with the targets mem_matesw builds
(software/bwamem_pair.c:127-144): 257..SMEM_KSWA_MAX_TLEN bases.

Golden: tests/golden/kswa_msw_a1 / _a2 (.smat / .smar), the compiled
reference's own ksw_align2 (tests/golden/make_golden_msw.py --kswa-only), 552
problems in groups that tests/golden/kswa_msw.json locates:
  grid    target lengths around the 64-row fetch and at the limit x query
          lengths around the vector widths and the wave's 64-column chunk
  rescue  100..250 bp reads against 400..1500 bp windows, both strands
  tandem  a list b of 150, 300 and tlen / 2 = 1024 entries
  late    score2 / te2 from an entry late in the list
  tie     two entries of the same score: the first wins
Bar: all seven kswr_t fields bit-exact for the restatement (here) and for
smem_ksw_align2_long on the GPU (test_gpu_ksw_align_long.py)."""
import numpy as np
import pytest

from oracle import oracle
from tests import msw_data

XBYTE, XSTOP, XSUBO, XSTART = 0x10000, 0x20000, 0x40000, 0x80000
GRID_TLEN = [257, 319, 320, 321, 511, 512, 513, 1000, msw_data.MAX_TLEN - 1, msw_data.MAX_TLEN]
GRID_QLEN = [1, 16, 17, 64, 65, 150, 250, 256]


def test_kswa_msw_fixture_shape():
    """The sets still hold the cases they were made for."""
    meta = msw_data.kswa_meta()
    assert meta["max_tlen"] == msw_data.MAX_TLEN >= 2048
    total = 0
    for name in msw_data.KSWA_SETS:
        a = int(name[-1])
        kb, want = msw_data.load_kswa(name)
        m = meta[name]
        T = kb.tasks
        total += T.size
        assert T.size == want.size == m["n"]
        assert int(kb.mat[0]) == a and (kb.o_del, kb.e_del, kb.o_ins, kb.e_ins) == (6 * a, a, 6 * a, a)
        assert T["tlen"].min() >= 257 and T["tlen"].max() == msw_data.MAX_TLEN
        byte = (T["xtra"] & XBYTE) != 0
        assert byte.sum() >= 50 and (~byte).sum() >= 50          # both branches
        lo, hi = m["groups"]["grid"]
        g = T[lo:hi]
        assert sorted(set(g["tlen"])) == GRID_TLEN and sorted(set(g["qlen"])) == GRID_QLEN
        for tl in GRID_TLEN:
            for ql in GRID_QLEN:
                sel = (g["tlen"] == tl) & (g["qlen"] == ql)
                if a == 1:   # each shape byte-scored and 16-bit
                    assert sorted((g["xtra"][sel] & XBYTE).tolist()) == [0, XBYTE]
                else:
                    assert sel.sum() == 1
        assert (want["tb"][lo:hi] >= 0).sum() >= (hi - lo) // 2  # the start pass over a long target
        lo, hi = m["groups"]["rescue"]
        g, w = T[lo:hi], want[lo:hi]
        assert hi - lo == 110
        assert g["qlen"].min() >= 100 and g["qlen"].max() <= 250
        assert g["tlen"].min() >= 400 and g["tlen"].max() <= 1500
        assert ((g["xtra"] & 0xffff) == 19 * a).all() and ((g["xtra"] & (XSUBO | XSTART)) == (XSUBO | XSTART)).all()
        assert (((g["xtra"] & XBYTE) != 0) == (g["qlen"] * a < 250)).all()
        assert (w["tb"] >= 0).sum() >= 100 and (w["te"] >= 256).sum() >= 50   # hits that end past the short limit
        lo, hi = m["groups"]["tandem"]
        for k in range(lo, hi):
            n_ent = m["tandem_entries"][k - lo]
            assert T[k]["tlen"] == 2 * n_ent and T[k]["xtra"] == XSUBO | XSTART | XBYTE | 1
            assert (want[k]["score"], want[k]["score2"]) == ((a, a) if T[k]["qlen"] == 1 else (2 * a, 2 * a))
        assert max(m["tandem_entries"]) == msw_data.MAX_TLEN // 2 and sorted(set(m["tandem_entries"]))[:2] == [150, 300]
        assert (want[lo]["te"], want[lo]["te2"]) == (0, 2)        # `A`: the first entry outside the window
        lo, hi = m["groups"]["late"]
        w = want[lo:hi]
        assert hi - lo == 20
        frm = np.array(m["late_from"])
        assert (w["te"] < 260).all()                              # the best copy is early
        assert (w["te2"] >= frm).sum() >= 15                      # score2 / te2 from the weak copy at the end
        assert (w["score2"] > 4 * 4).sum() >= 15
        lo, hi = m["groups"]["tie"]
        w = want[lo:hi]
        assert hi - lo == 20
        first, second = np.array(m["tie_first"]), np.array(m["tie_second"])
        assert (first + 45 < second).all()
        # both blocks score the 40 bases they repeat; the reference reports the first
        hit = w["score2"] == 40 * a
        assert hit.sum() >= 15
        # (unless the best hit's window, te +- ceil(score / a), covers it: software/ksw.c:219-221)
        d = (w["score"] + a - 1) // a
        inside = (first >= w["te"] - d) & (first <= w["te"] + d)
        assert inside.sum() <= 2
        assert (w["te2"][hit] == np.where(inside, second, first)[hit]).all()
    assert total <= 600


@pytest.mark.parametrize("name", msw_data.KSWA_SETS)
def test_kswa_msw_oracle_vs_reference(name):
    kb, want = msw_data.load_kswa(name)
    msw_data.same(oracle.ksw_align2(kb), want, kb)
