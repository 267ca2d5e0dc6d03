"""accuracy()'s scores over a leading cell axis (train.accuracy_scores_many, the
host statement of pgp_tune_scores_many) against the per-cell
``accuracy_scores``, bit for bit, and the new entry's place in the C-ABI.  No
device."""
import re
from fractions import Fraction

import numpy as np
import pytest

from preganplus_amd import _native
from preganplus_amd import train as TR

K = 16


def _dists(p, P3, fused):
    """The three class distances of proto p as accuracy_scores computes them, or (fused) as a compiler that
    contracts a*a + b*b into fma(a, a, b*b) would: the sum in exact rational arithmetic, rounded once."""
    out = []
    for k in range(3):
        a, b = float(p[0] - P3[k, 0]), float(p[1] - P3[k, 1])
        out.append(float(Fraction(a) * Fraction(a) + Fraction(b * b)) / 2.0 if fused else (a * a + b * b) / 2.0)
    return out


def _hit(d, c):
    return d[c] <= (d[1] if c == 0 else d[0]) and d[c] <= (d[1] if c == 2 else d[2])


def crafted_cells(H, n=4):
    """Three cells [3,n,H,...] with the cases the scores can go wrong on (n >= 4):
    cell 0: protos on the bisectors of its prototypes up to rounding, so that distances agree to ~1e-16
            relative and a contracted multiply-add flips pos <= n0 / n1; a tie lg[1] == lg[0]; hosts exactly
            equidistant from prototypes 0 = (0.25, 0.25) and 1 = (0.75, 0.75) (pos == n0: a hit); window 2
            without positives among windows that have them; cls outside 0..2 on non-anomalous hosts;
    cell 1: random;
    cell 2: no positive label in any window (accuracy_scores divides by zero)."""
    r = np.random.default_rng(1000 + H)
    lg = r.normal(size=(3, n, H, 2))
    pr = r.uniform(0.05, 0.95, (3, n, H, 2))
    y = (r.uniform(size=(3, n, H)) < 0.4).astype(np.int32)
    cls = r.integers(0, 3, (3, n, H)).astype(np.int32)
    P = r.uniform(0.1, 0.9, (3, K, 2))
    P[0, 0], P[0, 1], P[0, 2] = (0.25, 0.25), (0.75, 0.75), (0.875, 0.125)
    # points on the bisector of prototypes 0/1 or 1/2; of a few draws per host the first on which the
    # contracted distance decides the hit differently (where one is found)
    for w in range(n):
        for h in range(H):
            a, b = (0, 1) if (w + h) % 2 == 0 else (1, 2)
            c = a if h % 3 else b
            mid = (P[0, a] + P[0, b]) / 2.0
            d = P[0, b] - P[0, a]
            for _ in range(40):
                q = mid + r.uniform(-0.3, 0.3) * np.array([-d[1], d[0]]) * (1 + 1e-3 * r.uniform())
                if _hit(_dists(q, P[0], False), c) != _hit(_dists(q, P[0], True), c):
                    break
            pr[0, w, h] = q
            cls[0, w, h] = c
    y[0] = 1
    lg[0, 0, 0] = (0.375, 0.375)                       # tie -> res 0
    y[0, 0, 0] = 0
    pr[0, 0, 1], cls[0, 0, 1] = (0.5, 0.5), 0          # pos == n0 -> hit
    pr[0, 1, 2], cls[0, 1, 2] = (0.5, 0.5), 1          # the same from class 1's side
    y[0, 2] = 0                                        # a window without positives
    y[0, 3, 3], y[0, 1, 0] = 0, 0
    cls[0, 3, 3], cls[0, 2, 1], cls[0, 1, 0] = 7, -2, 3     # outside 0..2 on non-anomalous hosts
    y[2] = 0
    cls[2, 0, 0] = 5
    return lg, pr, y, cls, P


def per_cell(lg, pr, y, cls, P):
    """The reference: a loop over accuracy_scores; (scores, flag) with NaN where it raises."""
    M = lg.shape[0]
    sc, flag = np.full((M, 2), np.nan), np.zeros(M, dtype=np.int32)
    for m in range(M):
        try:
            sc[m] = TR.accuracy_scores(lg[m], pr[m], y[m], cls[m], P[m])
        except ZeroDivisionError:
            flag[m] = 1
    return sc, flag


def check_equal(got, want):
    (gs, gf), (ws, wf) = got, want
    assert gs.dtype == np.float64 and gs.shape == ws.shape
    assert np.array_equal(gf, wf)
    ok = wf == 0
    assert (gs[ok, 0] == ws[ok, 0]).all() and (gs[ok, 1] == ws[ok, 1]).all()   # == on the doubles
    assert gs[ok].tobytes() == ws[ok].tobytes()


@pytest.mark.parametrize("H", [8, 16])
@pytest.mark.parametrize("n", [1, 4, 10])
def test_random_cells_equal_the_per_cell_loop(H, n):
    r = np.random.default_rng(7 * H + n)
    M = 9
    lg = r.normal(size=(M, n, H, 2))
    pr = r.uniform(0, 1, (M, n, H, 2))
    y = (r.uniform(size=(M, n, H)) < 0.3).astype(np.int32)
    y[2] = 0                                           # a cell that raises
    if n > 1:
        y[3, 0] = 0                                    # a window without positives
    cls = r.integers(-1, 5, (M, n, H)).astype(np.int32)
    P = r.uniform(0.1, 0.9, (M, K, 2))
    want = per_cell(lg, pr, y, cls, P)
    assert want[1][2] == 1 and want[1].sum() == 1
    check_equal(TR.accuracy_scores_many(lg, pr, y, cls, P), want)


@pytest.mark.parametrize("H", [8, 16])
def test_crafted_cells_equal_the_per_cell_loop(H):
    lg, pr, y, cls, P = crafted_cells(H)
    want = per_cell(lg, pr, y, cls, P)
    assert want[1].tolist() == [0, 0, 1]
    got = TR.accuracy_scores_many(lg, pr, y, cls, P)
    check_equal(got, want)
    # the equidistant hosts of cell 0 are hits: with them missed, windows 0 and 1 would score lower
    d0 = np.mean((pr[0, 0, 1] - P[0, 0]) ** 2)
    d1 = np.mean((pr[0, 0, 1] - P[0, 1]) ** 2)
    assert d0 == d1


def test_crafted_cell_0_is_sensitive_to_contraction():
    """The near-bisector protos of cell 0 are what they are made for: on some host the comparison
    pos <= n0 comes out differently when the distance is evaluated with one fused multiply-add (emulated in
    exact rational arithmetic, rounded once)."""
    for H in (8, 16):
        _, pr, y, cls, P = crafted_cells(H)
        flips = sum(_hit(_dists(pr[0, w, h], P[0], False), int(np.clip(cls[0, w, h], 0, 2)))
                    != _hit(_dists(pr[0, w, h], P[0], True), int(np.clip(cls[0, w, h], 0, 2)))
                    for w in range(pr.shape[1]) for h in range(H) if y[0, w, h] > 0)
        assert flips >= H


def test_entry_is_in_the_header_and_the_signature_table():
    assert "pgp_tune_scores_many" in _native.SIGNATURES
    restype, argtypes = _native.SIGNATURES["pgp_tune_scores_many"]
    assert len(argtypes) == 13
    text = open("include/preganplus.h").read()
    m = re.search(r"int\s+pgp_tune_scores_many\s*\(([^)]*)\)\s*;", text)
    assert m is not None
    assert len(m.group(1).split(",")) == 13
    assert "train.py:60-109" in text[text.index("pgp_tune_forward_cells("):m.start()]
    assert re.search(r"#define\s+PGP_ABI_VERSION\s+1\b", text)
