"""Seeded weights whose decisions depend on the input — TEST INFRASTRUCTURE.

With ``weights.synth_weights`` the per-host anomaly margin l1 - l0 averages
0.5-0.7 and moves by 2e-3 (8 hosts) to 2e-4 (64 hosts) across windows of the
c2 input distribution: every window flags the same hosts, ``any`` is 1
everywhere and the discriminator gate comes out lopsided, so a test on those
weights compares the decisions of a constant function of the input.

``branch_weights`` moves two biases, as ``branches16_weights``
(tests/test_oracle_golden.py) does with its stored offsets, so that both gates
of run_model open and close within one batch (PreGANPlus.py:125-127: no
flagged host, the early return; :87-88: the discriminator keeps the original
decision):

- per host, the odd entry of ``transformer/anomaly_decoder.0.bias`` loses the
  1 - q quantile over windows of that host's margin, q = 1 - 0.5 ** (1 / H)
  (moved into the widest gap between the margins next to it): each host is
  flagged in a share q of the windows, so about half the windows flag no host;
- ``disc/probs.2.bias[0]`` gains the median over windows of log p1 - log p0:
  about half the windows keep.

Everything is seeded numpy and the fp64 oracle; every value is rounded to an
fp32-representable double so that an fp32 kernel and the oracle start from the
same numbers.
"""
import copy

import numpy as np

from oracle import pregan_oracle as O
from preganplus_amd import weights as W
from tests.test_gpu_parity import c2

N_WINDOWS = 293
_cache = {}


def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def inputs(H, n=N_WINDOWS):
    windows, sched = c2(np.random.Generator(np.random.PCG64(700 + H)), n, H, dense=9)
    return _f32(windows), _f32(sched)


def _thresholds(margin, p):
    """Per host (column) a threshold near the p quantile of its margins, placed
    in the middle of the widest of the three gaps between neighbouring sorted
    margins around that quantile (one window more or fewer flagged than the
    quantile itself gives): the decisions nearest the threshold sit as far from
    it as the draw allows.  The interpolated quantile itself can land almost
    on a sample (at 50 hosts, 292 (1 - q) = 287.98: 2 % of a gap from the 288th
    margin of every host), which put 47 decisions of 14,650 within 1e-6 of
    their threshold and 39 windows at the mercy of fp32 rounding; in the gap
    none is within 1e-6 and 2 are within 3e-6.  The share of decisions inside
    the rigorous band (rtol 1e-4 on both logits) is the same either way."""
    m = np.sort(margin, axis=0)[::-1]                                     # descending
    k0 = (margin > np.quantile(margin, p, axis=0)).sum(axis=0)            # flagged by the quantile
    thr = np.empty(margin.shape[1])
    for h in range(margin.shape[1]):
        ks = [k for k in (k0[h] - 1, k0[h], k0[h] + 1) if 1 <= k < m.shape[0]]
        k = max(ks, key=lambda k: m[k - 1, h] - m[k, h])
        thr[h] = 0.5 * (m[k - 1, h] + m[k, h])
    return thr


def branch_weights(H, seed=7, n=N_WINDOWS):
    """(weights, windows [n,3,3H], sched [n,H,H], ref): ``ref`` is the fp64
    oracle's forward on the shifted weights (with 'sched32').  Cached per
    (H, seed, n) within a session: callers must not modify what they get."""
    key = (H, seed, n)
    if key in _cache:
        return _cache[key]
    windows, sched = inputs(H, n)
    w = copy.deepcopy(W.synth_weights(H, seed))
    r = O.forward(w, windows, sched)
    margin = r["logits"][..., 1] - r["logits"][..., 0]                    # [n, H]
    q = 1.0 - 0.5 ** (1.0 / H)
    b = np.array(w["transformer"]["anomaly_decoder.0.bias"], dtype=np.float64)
    b[1::2] -= _thresholds(margin, 1.0 - q)
    w["transformer"]["anomaly_decoder.0.bias"] = _f32(b)
    r = O.forward(w, windows, sched)
    db = np.array(w["disc"]["probs.2.bias"], dtype=np.float64)
    db[0] += np.median(np.log(r["probs"][:, 1]) - np.log(r["probs"][:, 0]))
    w["disc"]["probs.2.bias"] = _f32(db)
    ref = O.forward(w, windows, sched)
    ref["sched32"] = sched.astype(np.float32)
    _cache[key] = (w, windows, sched, ref)
    return _cache[key]
