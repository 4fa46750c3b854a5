"""Loaders of the mate-rescue fixtures (tests/golden/make_golden_msw.py)."""
import gzip
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KSWA_SETS = ["kswa_msw_a1", "kswa_msw_a2"]
MAX_TLEN = 2048   # SMEM_KSWA_MAX_TLEN


def kswa_meta() -> dict:
    with open(os.path.join(GOLDEN, "kswa_msw.json")) as fh:
        return json.load(fh)


def load_kswa(name):
    """(KswBatch, the reference's results)"""
    from smemgpu import synth
    with gzip.open(os.path.join(GOLDEN, name + ".smat.gz"), "rb") as fh:
        kb = synth.read_smat(fh.read())
    with gzip.open(os.path.join(GOLDEN, name + ".smar.gz"), "rb") as fh:
        want = synth.read_smar(fh.read())
    return kb, want


def same(got, want, kb=None):
    import numpy as np
    bad = np.nonzero(got != want)[0]
    if bad.size and kb is not None:
        for k in bad[:5]:
            print(f"task {k}: {kb.tasks[k]}\n  got  {got[k]}\n  want {want[k]}")
    for f in want.dtype.names:
        fb = np.nonzero(got[f] != want[f])[0]
        assert fb.size == 0, f"{f}: {fb.size} differ ({bad.size} results in all), first {fb[:5]}"
