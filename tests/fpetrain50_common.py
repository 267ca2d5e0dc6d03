"""Shared by the 50-host offline FPE training tests: the fixture of
tests/golden/make_golden_fpetrain50.py (three files), its initial weights
(stored as a seed and a checksum) and the comparison of a tensor with its
record, whole or through tests/golden/digest.py."""
import functools

import numpy as np

from preganplus_amd import weights as W
from tests.golden import digest as D

GOLD = "tests/golden"
H = 50
N_WIN = 24


@functools.lru_cache(maxsize=None)
def fixture():
    """(epochs record, AdamW moments, single steps, initial weights, initial
    prototypes).  Loaded once; nothing in it is written to."""
    z = dict(np.load(f"{GOLD}/fpe_train_h50.npz"))
    zo = dict(np.load(f"{GOLD}/fpe_train_h50_opt.npz"))
    zs = dict(np.load(f"{GOLD}/fpe_train_h50_steps.npz"))
    w = W.synth_fpe_weights(H, seed=int(z["weights_seed"]))
    assert W.fpe_weights_checksum(w) == float(z["weights_checksum"])
    for d in (z, zo, zs):
        for a in d.values():
            a.setflags(write=False)
    return z, zo, zs, w["fpe"], w["prototypes"]


def recorded(z, name, got, cmp, sum_rel=None, key=None):
    """cmp(got, want, label) on the tensor recorded under `name`: stored whole,
    or as a digest (sampled entries; row and column sums when sum_rel is given)."""
    if name in z:
        cmp(np.asarray(got, dtype=np.float64).reshape(z[name].shape), z[name], name)
    else:
        D.check(z, name, got, cmp, sum_rel=sum_rel, key=key)


def close(rtol, atol):
    def f(got, want, what):
        np.testing.assert_allclose(got, want, rtol=rtol, atol=atol, err_msg=what)
    return f
