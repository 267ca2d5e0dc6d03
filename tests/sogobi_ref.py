"""CPU statements of second-order GOBI — TEST INFRASTRUCTURE ONLY.

so_opt() (scheduler/BaGTI/src/opt.py:35-51) with Adahessian
(scheduler/BaGTI/src/adahessian.py:49-168) over the energy_latency_16 surrogate,
with the Hutchinson probes v given instead of drawn:

* restate(): a functional restatement in torch (autograd.grad twice, the
  scalars as Python doubles), fp32 or fp64.  In fp32 it is bit-equal to the
  reference's own so_opt on tests/golden/sogobi_h16.npz (test_sogobi_oracle.py).
* Trajectory64: the same in fp64 for a batch, forward-over-reverse written out
  (no autograd), recording each step's g, hv, pre-projection x and how far every
  row's decision is from flipping under a given error of g and hv.  The GPU
  tests compare the kernel with it.
"""
from __future__ import annotations

import functools
import math
import os

import numpy as np
import torch

from oracle import gobi_oracle as GO

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "gobi_h16.npz")
GOLD_SO = os.path.join(HERE, "golden", "sogobi_h16.npz")
GOLD_SO_TAPS = os.path.join(HERE, "golden", "sogobi_h16_taps.npz")
WEIGHTS = os.path.join(os.path.dirname(HERE), "preganplus_amd", "data", "gobi_energy_latency_16.npz")

H = 16
LR, BETAS, EPS = 0.8, (0.9, 0.999), 1e-4
MAX_IT, PATIENCE = 200, 30
# The reference's own error at step 1 on the 240 fixture environments: its fp32
# g and hv (the fixture's taps) against fp64, max-normalised per environment,
# the worst of the 240.  test_sogobi_oracle.py measures both and holds them to
# these figures; the GPU tolerances are TOL_FACTOR times them: a different
# association of the 288- and 128-term sums can err the other way.
REF_ERR_G, REF_ERR_HV = 1.06e-6, 1.98e-6
TOL_FACTOR = 4.0
TOL_G, TOL_HV = TOL_FACTOR * REF_ERR_G, TOL_FACTOR * REF_ERR_HV


def unpack_signs(words):
    """uint32 [..., 9] -> float64 [..., 16, 18] of +-1 (bit k of word k >> 5 set: +1)."""
    w = np.asarray(words, dtype=np.uint32)
    bits = (w[..., None] >> np.arange(32, dtype=np.uint32)) & 1
    return 2.0 * bits.reshape(*w.shape[:-1], H, H + 2).astype(np.float64) - 1.0


@functools.lru_cache(maxsize=None)
def fixture():
    """inits [240,16,18], the fixture's arrays, and signs padded to [240, 200, 9]
    (an environment's unused steps are zero words: never read by a run that
    follows the fixture's trajectory, and valid probes (-1) for one that does not)."""
    z, t = np.load(GOLD_SO), np.load(GOLD_SO_TAPS)
    inits = np.load(GOLD)["inits"]
    off = z["sign_offsets"]
    signs = np.zeros((len(inits), MAX_IT, 9), np.uint32)
    for e in range(len(inits)):
        signs[e, :off[e + 1] - off[e]] = z["sign_words"][off[e]:off[e + 1]]
    return {"inits": inits, "signs": signs, "steps": np.diff(off), "results": z["results"],
            "iterations": z["iterations"], "fitness": z["fitness"], "g": t["g"], "hv": t["hv"], "pre": t["pre"]}


def restate(sd, x0, vs, dtype=torch.float32, max_it=MAX_IT, taps=None):
    """so_opt on one init [16,18] with the probes vs[step] ([16,18] of +-1).
    Returns (result, iterations); taps collects each step's (g, hv, pre)."""
    sd = {k: v.to(dtype) for k, v in sd.items()}
    lrs = GO.cosine_lrs()
    x = torch.as_tensor(np.asarray(x0), dtype=dtype)
    ea, es = torch.zeros_like(x), torch.zeros_like(x)
    eq = it = step = 0
    while it < max_it:
        cpu_old, alloc_old = x[:, :2].clone(), x[:, 2:].clone()
        xr = x.clone().requires_grad_(True)
        g, = torch.autograd.grad(GO.surrogate(sd, xr), xr, create_graph=True)
        hv, = torch.autograd.grad(g, xr, grad_outputs=torch.as_tensor(vs[step], dtype=dtype))
        g, hut = g.detach(), hv.abs()
        step += 1
        # the in-place forms of adahessian.py:153-164 (add_ with alpha fuses the multiply-add)
        ea.mul_(BETAS[0]).add_(g, alpha=1 - BETAS[0])
        es.mul_(BETAS[1]).addcmul_(hut, hut, value=1 - BETAS[1])
        bc1, bc2 = 1 - BETAS[0] ** step, 1 - BETAS[1] ** step
        denom = (es.sqrt() ** 1 / math.sqrt(bc2) ** 1).add_(EPS)
        p = x - lrs[step - 1] * (ea / bc1 / denom + 0 * x)
        if taps is not None:
            taps.append((g.clone(), hv.clone(), p.clone()))
        a = p[:, 2:]
        oh = torch.zeros_like(a)
        oh[torch.arange(H), GO.first_argmax(a)] = 1
        x = torch.cat((cpu_old, oh), 1)
        eq = eq + 1 if torch.equal(alloc_old, x[:, 2:]) else 0
        if eq > PATIENCE:
            break
        it += 1
    return x, it


def grad_hv64(sd, x, v):
    """g = dz/dx and hv = H v of z = 0.8 o0 + 0.2 o1 for a batch, fp64,
    forward-over-reverse: x, v [E, 288] -> (g, hv) [E, 288]."""
    W = [sd[f"find.{i}.weight"].double() for i in (0, 2, 4, 6)]
    b = [sd[f"find.{i}.bias"].double() for i in (0, 2, 4, 6)]
    c = torch.tensor([GO.COEFF_ENERGY, GO.COEFF_LATENCY], dtype=torch.float64)
    a, da, p1, p2 = x, v, [], []   # per layer: phi'(a), phi''(a)
    for l in range(3):
        pre, dpre = a @ W[l].T + b[l], da @ W[l].T
        if l < 2:   # softplus, torch's threshold 20
            s = torch.sigmoid(pre)
            d1 = torch.where(pre > 20, torch.ones_like(s), s)
            d2 = torch.where(pre > 20, torch.zeros_like(s), s * (1 - s))
            a = torch.nn.functional.softplus(pre)
        else:       # tanhshrink
            th = torch.tanh(pre)
            d1, d2 = th * th, 2 * th * (1 - th * th)
            a = pre - th
        p1.append(d1)
        p2.append(d2 * dpre)
        da = d1 * dpre
    o = torch.sigmoid(a @ W[3].T + b[3])
    d = c * o * (1 - o)
    dd = d * (1 - 2 * o) * (da @ W[3].T)
    for l in (2, 1, 0):
        g, dg = d @ W[l + 1], dd @ W[l + 1]
        d, dd = g * p1[l], dg * p1[l] + g * p2[l]
    return d @ W[0], dd @ W[0]


class Trajectory64:
    """so_opt in fp64 for a batch: inits [E,16,18], signs uint32 [E, >= steps, 9].

    result [E,16,18], iterations [E]; for the first `keep` steps g, hv, pre
    [keep][E,16,18] and after[s] = x after step s + 1's projection; margin
    [E, steps] = min over the rows of gap / (2 max_row B), the fp64 top-2 gap of
    the row's pre-projection values over twice the bound of its change under an
    error tol_g max|g|, tol_hv max|hv| of g and hv (nan once the environment
    has stopped):
        B = lr_t (dg + |m^| / denom dh) / denom.
    At step t, dg and dh take the maxima of |g| and |hv| over steps 1..t: m^ and
    denom are normalised averages of those steps' g and hv^2, so their errors are
    bounded by the largest of theirs.  A row with margin > 1 keeps its argmax under
    any such error."""

    def __init__(self, sd, inits, signs, max_it=MAX_IT, keep=3, tol_g=TOL_G, tol_hv=TOL_HV):
        lrs = GO.cosine_lrs()
        x = torch.as_tensor(np.asarray(inits), dtype=torch.float64).clone()
        E = x.shape[0]
        ea, es = torch.zeros_like(x), torch.zeros_like(x)
        eq = np.zeros(E, int)
        self.iterations = np.full(E, max_it)
        self.margin = np.full((E, max_it), np.nan)
        self.g, self.hv, self.pre, self.after = [], [], [], []
        mg, mh = torch.zeros(E, dtype=torch.float64), torch.zeros(E, dtype=torch.float64)
        active = np.ones(E, bool)
        for it in range(max_it):
            if not active.any():
                break
            idx = torch.as_tensor(np.nonzero(active)[0])
            xa = x[idx]
            v = torch.as_tensor(unpack_signs(np.asarray(signs)[idx.numpy(), it]))
            g, hv = grad_hv64(sd, xa.reshape(-1, H * (H + 2)), v.reshape(-1, H * (H + 2)))
            g, hv = g.reshape(-1, H, H + 2), hv.reshape(-1, H, H + 2)
            step = it + 1
            ea[idx] = ea[idx] * BETAS[0] + g * (1 - BETAS[0])
            es[idx] = es[idx] * BETAS[1] + hv * hv * (1 - BETAS[1])
            mhat = ea[idx] / (1 - BETAS[0] ** step)
            denom = es[idx].sqrt() / math.sqrt(1 - BETAS[1] ** step) + EPS
            p = xa - lrs[it] * (mhat / denom)
            mg[idx] = torch.maximum(mg[idx], g.abs().amax((1, 2)))
            mh[idx] = torch.maximum(mh[idx], hv.abs().amax((1, 2)))
            dg, dh = (tol_g * mg[idx])[:, None, None], (tol_hv * mh[idx])[:, None, None]
            B = (lrs[it] * (dg + mhat.abs() / denom * dh) / denom)[:, :, 2:].amax(2)
            a = p[:, :, 2:]
            top = a.sort(2).values
            self.margin[idx.numpy(), it] = ((top[:, :, -1] - top[:, :, -2]) / (2 * B + 1e-300)).amin(1).numpy()
            if it == 0:
                self.robust_rows1 = (top[:, :, -1] - top[:, :, -2]) > 2 * B   # [E,16], step 1 (all active)
            oh = torch.zeros_like(a)
            oh.scatter_(2, a.argmax(2, keepdim=True), 1.0)   # the first maximum (ties do not occur in fp64 here)
            xn = torch.cat((xa[:, :, :2], oh), 2)
            same = (xn[:, :, 2:] == xa[:, :, 2:]).all(2).all(1).numpy()
            x[idx] = xn
            if it < keep:
                for lst, val in ((self.g, g), (self.hv, hv), (self.pre, p), (self.after, xn)):
                    full = torch.full((E, H, H + 2), float("nan"), dtype=torch.float64)
                    full[idx] = val
                    lst.append(full.numpy())
            ids = idx.numpy()
            eq[ids] = np.where(same, eq[ids] + 1, 0)
            done = ids[eq[ids] > PATIENCE]
            self.iterations[done] = it
            active[done] = False
        self.result = x.numpy()
        self.qualifies = np.nanmin(self.margin, axis=1) > 1.0


@functools.lru_cache(maxsize=None)
def fixture_trajectory():
    """The fp64 trajectory of the 240 fixture environments on the fixture's signs."""
    f = fixture()
    sd, _ = GO.load(WEIGHTS)
    return Trajectory64(sd, f["inits"], f["signs"])


def non_one_hot_inits(n=96):
    """test_gobi_non_one_hot_init's recipe on the first n fixture inits: every
    other environment's allocation uniform in [0, 1), every fourth's row 3 all zero."""
    inits = fixture()["inits"][:n].copy()
    rng = np.random.Generator(np.random.PCG64(4))
    inits[::2, :, 2:] = rng.uniform(0, 1, size=inits[::2, :, 2:].shape).astype(np.float32)
    inits[1::4, 3, 2:] = 0.0
    return inits


def max_normalised(a, ref):
    """max |a - ref| / max |ref| per environment: [E, ...] -> [E]."""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    ax = tuple(range(1, ref.ndim))
    return np.abs(a - ref).max(ax) / np.abs(ref).max(ax)


# ---- a duck-typed COSCO environment: hostlist / containerlist, as test_gobi_scheduler_decision_list builds ----

class _Host:
    def __init__(self, c):
        self.c = c

    def getCPU(self):
        return self.c


class _Cont:
    def __init__(self, i, ips, h):
        self.id, self.ips, self.h = i, ips, h

    def getApparentIPS(self):
        return self.ips

    def getHostID(self):
        return self.h


class _Env:
    pass


def duck_env(rng, max_ips):
    env = _Env()
    env.hostlist = [_Host(float(c)) for c in rng.uniform(0, 100, 16)]
    env.containerlist = [_Cont(i, float(rng.uniform(0, max_ips)), int(rng.integers(-1, 16)))
                         if rng.uniform() < 0.8 else None for i in range(16)]
    return env
