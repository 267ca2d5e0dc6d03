"""An fp64 replay of one AdamW step from a kernel's own gradient bits, and the
fp32 rounding bound an evaluation of that step must stay inside.

Every training kernel of the project leaves its gradient in a ``G`` buffer the
host can read.  Given ``P``, ``m``, ``v`` from before a step and ``G`` from
after it, ``replay`` restates torch's single-tensor AdamW (torch/optim/adamw.py,
decoupled decay) in fp64 on exactly those bits, and ``bounds`` says how far an
fp32 evaluation may be from it.  The same ``G`` enters both sides, so a
comparison carries no gradient noise: it tests the update and nothing else.

The scalars are taken as torch takes them when the parameter is an fp32
tensor: python doubles (``beta2``, ``1 - beta2``, ``1 - beta1``,
``1 - lr*wd``, ``lr / (1 - beta1**t)``, ``sqrt(1 - beta2**t)``, ``eps``), each
rounded ONCE to fp32 where it meets the tensor.  In particular the moment
weights are ``float32(1 - beta)``, not ``float32(1) - float32(beta)``: with
beta2 = 0.999 these differ by 1.29e-5 relative.  The replay therefore defines
the target bits up to the bound below.

The bound (``bounds``), u = 2**-24 (half an fp32 ulp, the relative error of one
round-to-nearest operation), written for the evaluation order of
``adamw_update`` (csrc/pgp_train.hpp); a fused multiply-add only removes
roundings.

* ``m1 = m0 + w1*(g - m0)``: three roundings (the difference, the product, the
  sum), each relative to a quantity of at most ``|m0| + |w1*(g - m0)|``::

      tol_m = 3 u (|m0| + |w1 (g - m0)|)

  (the operands' size, not ``|m1|``: the sum may cancel).
* ``v1 = b2*v0 + w2*g*g``: four roundings (three products, the sum) of
  non-negative terms, so each is relative to at most ``v1``::

      tol_v = 4 u v1

* ``p1 = p0*(1 - lr*wd) - step*m1 / (sqrt(v1)/bc2s + eps)``.  Call the update
  term D.  Roundings that are relative to D: v1's four (the square root halves
  them, counted in full), sqrtf, the division by bc2s, the sum with eps, the
  product step*m1, the division by the denominator, and the final subtraction
  (relative to ``|p1| <= |p0| + |D|``): 10.  Relative to ``|p0|``: the decay
  product, its factor (``lr*wd`` is formed in fp32 before ``1 - lr*wd``, which
  can land one fp32 neighbour from torch's ``float32(1 - lr*wd)``) and the
  final subtraction: 3.  The error of m1 enters D linearly, through
  ``step / denominator``::

      tol_p = 3 u |p0| + 10 u |D| + step/denominator * tol_m

  Where m1 does not cancel, ``step/denominator * tol_m = 3 u |D|`` and the
  D part is 13 u |D|: one u per rounding of the function on that path (lerp 3,
  v 4, sqrtf, two divisions, the eps sum, a product, the subtraction).  After
  an old gradient spike ``m-hat / sqrt(v-hat)`` exceeds 1, so |D|, not lr, is
  the scale.

Each tolerance gets an absolute floor of 2**-100 (7.9e-31) for fp32 subnormals
(a flushed or denormal product such as (1e-30)**2); it cannot hide an error in
any value above 1e-22.  No floor is needed in ``p`` for an underflowed ``v``:
then ``sqrt(v) <= 2e-19``, against ``eps = 1e-8`` the denominator equals eps to
2e-11 relative, far below u.

An inactive tensor and every element outside all tensors are returned
unchanged with tolerance 0: they must keep their bits.
"""
import numpy as np

U = 2.0 ** -24
FLOOR = 2.0 ** -100
C_M, C_V, C_P0, C_D = 3.0, 4.0, 3.0, 10.0

f32 = lambda x: float(np.float32(x))


def scalars(lr, wd, b1, b2, eps, step):
    """The step's scalars as torch applies them to an fp32 tensor: computed in
    double, each rounded once to fp32.  (decay, w1, b2, w2, step_size, bc2_sqrt, eps)."""
    step = float(step)
    return (f32(1.0 - lr * wd), f32(1.0 - b1), f32(b2), f32(1.0 - b2), f32(lr / (1.0 - b1 ** step)),
            f32(np.sqrt(1.0 - b2 ** step)), f32(eps))


def _tensor(p0, m0, v0, g, sc):
    decay, w1, b2, w2, step_size, bc2s, eps = sc
    lerp = w1 * (g - m0)
    m1 = m0 + lerp
    v1 = b2 * v0 + w2 * g * g
    denom = np.sqrt(v1) / bc2s + eps
    d = step_size * m1 / denom
    p1 = p0 * decay - d
    tol_m = C_M * U * (np.abs(m0) + np.abs(lerp))
    tol_v = C_V * U * v1
    tol_p = U * (C_P0 * np.abs(p0) + C_D * np.abs(d)) + step_size / denom * tol_m
    return p1, m1, v1, np.abs(d), tol_p + FLOOR, tol_m + FLOOR, tol_v + FLOOR


def _run(P0, m0, v0, G, tensors, lr, wd, b1, b2, eps):
    P0, m0, v0, G = (np.asarray(a) for a in (P0, m0, v0, G))
    for a in (P0, m0, v0, G):
        assert a.dtype == np.float32 and a.ndim == 1 and a.shape == P0.shape
    out = [P0.astype(np.float64), m0.astype(np.float64), v0.astype(np.float64)]
    out += [np.zeros(P0.shape) for _ in range(4)]          # |D|, tol_p, tol_m, tol_v
    g64 = G.astype(np.float64)
    for off, n, active, step, *own_lr in tensors:
        if not active or n == 0:
            continue
        assert 0 <= off and off + n <= P0.size and step >= 1
        sl = slice(off, off + n)
        sc = scalars(own_lr[0] if own_lr else lr, wd, b1, b2, eps, step)
        res = _tensor(out[0][sl], out[1][sl], out[2][sl], g64[sl], sc)
        for o, r in zip(out, res):
            o[sl] = r
    return out


def replay(P0, m0, v0, G, tensors, lr, wd, b1, b2, eps):
    """One AdamW step in fp64 on fp32 inputs (widened exactly).  tensors: a list
    of (offset, n, active, step) or (offset, n, active, step, lr) (a tensor with
    its own learning rate), step the count INCLUDING this step (>= 1); tensors
    must not overlap.  Returns P1, m1, v1, |D| as float64 arrays;
    inactive tensors and everything outside the tensors are unchanged, |D| 0."""
    return tuple(_run(P0, m0, v0, G, tensors, lr, wd, b1, b2, eps)[:4])


def bounds(P0, m0, v0, G, tensors, lr, wd, b1, b2, eps):
    """Per-element tolerances (tol_p, tol_m, tol_v) of an fp32 evaluation of
    that step around ``replay`` (derivation: module docstring); 0 where nothing
    may change."""
    return tuple(_run(P0, m0, v0, G, tensors, lr, wd, b1, b2, eps)[4:])


def ratios(got, P0, m0, v0, G, tensors, lr, wd, b1, b2, eps):
    """error / tolerance per element for got = (P1, m1, v1) fp32 arrays over the
    ACTIVE tensors' elements: three float64 arrays (0 elsewhere)."""
    r = _run(P0, m0, v0, G, tensors, lr, wd, b1, b2, eps)
    out = []
    for a, ref, tol in zip(got, r[:3], r[4:]):
        a = np.asarray(a)
        assert a.dtype == np.float32
        err = np.abs(a.astype(np.float64) - ref)
        out.append(np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), 0.0))
    return out


def active_mask(size, tensors):
    m = np.zeros(size, dtype=bool)
    for off, n, active, *_ in tensors:
        if active:
            m[off:off + n] = True
    return m


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_step(what, before, after, tensors, lr, wd, b1, b2, eps):
    """The whole check of one step.  before / after: dicts of fp32 arrays "P",
    "m", "v" (+ "G" in after, and in before if G must be unchanged).  Active
    elements inside the bounds, NaN-free; everything else bit-identical.
    Returns the worst error/tolerance of (P, m, v)."""
    G = after["G"]
    if "G" in before:
        assert np.array_equal(bits(before["G"]), bits(G)), f"{what}: G changed"
    act = active_mask(G.size, tensors)
    got = [after[k] for k in "Pmv"]
    rs = ratios(got, before["P"], before["m"], before["v"], G, tensors, lr, wd, b1, b2, eps)
    worst = []
    for k, a, r in zip("Pmv", got, rs):
        same = bits(before[k]) == bits(a)
        assert same[~act].all(), (f"{what}: {k} changed outside the active tensors at",
                                  np.flatnonzero(~same & ~act)[:8].tolist())
        assert np.isfinite(a[act]).all(), f"{what}: {k} not finite"
        w = float(r.max()) if r.size else 0.0
        i = int(r.argmax()) if r.size else -1
        assert w < 1.0, (f"{what}: {k} outside the AdamW bound: error/tolerance {w:.3g} at element {i}, "
                         f"{int((r >= 1).sum())} of {int(act.sum())} elements outside; p0 {before['P'][i]!r} "
                         f"g {G[i]!r} m0 {before['m'][i]!r} v0 {before['v'][i]!r} got {a[i]!r}")
        worst.append(w)
    return worst


# ---------------------------------------------------------------------------
# the synthetic generator the CPU and GPU tests share
# ---------------------------------------------------------------------------
G_EDGES = np.array([0.0] + [s * x for x in (1e-30, 1e-12, 1e-8, 1e-3, 1e4) for s in (1.0, -1.0)], dtype=np.float32)
P_EDGES = np.array([0.0, 1e-6, -1e-6], dtype=np.float32)


def synthetic(n, seed, fresh):
    """Seeded fp32 (P, m, v, G) of n elements.  G: a third cycles through exact
    zero and +-1e-30, 1e-12, 1e-8 (eps), 1e-3, 1e4, the rest log-uniform in
    [1e-7, 1] with random signs.  P: a quarter exact 0 / +-1e-6 (so the update
    is not hidden under |p| u), a quarter N(0, 1e-3), the rest N(0, 0.1).
    fresh: zero moments (step 1).  Otherwise m = +-10^U(-8,-1) with signs
    independent of G's (both agreements), v = 10^U(-14,-2), independent of m:
    ratios m/sqrt(v) far above 1 (an old spike) and far below occur; an eighth
    of the elements have small moments (|m| <= 1e-6, v <= 1e-12) under
    whatever G they got, 1e4 included (a spike now); some v are exact 0."""
    r = np.random.default_rng(seed)
    sign = lambda k: np.where(r.random(k) < 0.5, -1.0, 1.0)
    G = sign(n) * 10.0 ** r.uniform(-7, 0, n)
    e = r.random(n) < 1 / 3
    G[e] = G_EDGES[r.integers(0, len(G_EDGES), int(e.sum()))]
    P = r.normal(0, 0.1, n)
    q = r.random(n)
    P[q < 0.25] = P_EDGES[r.integers(0, len(P_EDGES), int((q < 0.25).sum()))]
    small = (q >= 0.25) & (q < 0.5)
    P[small] = r.normal(0, 1e-3, int(small.sum()))
    if fresh:
        m, v = np.zeros(n), np.zeros(n)
    else:
        m = sign(n) * 10.0 ** r.uniform(-8, -1, n)
        v = 10.0 ** r.uniform(-14, -2, n)
        s = r.random(n) < 0.125
        m[s] *= 1e-6 / 0.1
        v[s] *= 1e-12 / 1e-2
        v[r.random(n) < 0.02] = 0.0
    return tuple(a.astype(np.float32) for a in (P, m, v, G))


# the project's hyper-parameters (train.Trainer) and a set whose decay is visible in fp32
HYPERS = {"project": dict(lr=1e-4, wd=1e-5, b1=0.9, b2=0.999, eps=1e-8),
          "decay": dict(lr=1e-3, wd=1e-2, b1=0.9, b2=0.999, eps=1e-8)}
STEPS = (1, 2, 10, 10000)
