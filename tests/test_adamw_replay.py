"""CPU checks of the AdamW replay and its bound (tests/adamw_replay.py), on the
synthetic P / m / v / G the GPU test uses: an independent fp32 restatement of
the formula stays inside every bound, against the replay and against
torch.optim.AdamW itself on fp64 tensors; each wrong formula a kernel could
plausibly hold falls outside it."""
import numpy as np
import pytest
import torch

from tests import adamw_replay as AR

N = 20000
F = np.float32


def fp32_step(P, m, v, G, step, lr, wd, b1, b2, eps, flaw=None):
    """torch's single-tensor AdamW in numpy fp32, one rounding per operation,
    scalars as torch passes them (double, rounded once); ``flaw`` swaps in one
    wrong formula."""
    if flaw == "betas_swapped":
        b1, b2 = b2, b1
    decay, w1, b2f, w2 = F(1.0 - lr * wd), F(1.0 - b1), F(b2), F(1.0 - b2)
    step_size, bc2s, epsf = F(lr / (1.0 - b1 ** step)), F(np.sqrt(1.0 - b2 ** step)), F(eps)
    if flaw == "fp32_one_minus_beta":             # 1.0f - b1, 1.0f - b2
        w1, w2 = F(1.0) - F(b1), F(1.0) - F(b2)
    if flaw == "no_bc1":
        step_size = F(lr)
    if flaw == "no_bc2":
        bc2s = F(1.0)
    g = G
    if flaw == "l2":                              # weight decay folded into the gradient
        g, decay = G + F(wd) * P, F(1.0)
    p = P * decay
    m1 = m + w1 * (g - m)
    v1 = b2f * v + w2 * g * g
    if flaw == "eps_in_sqrt":
        den = np.sqrt(v1 / (bc2s * bc2s) + epsf)
    else:
        den = np.sqrt(v1) / bc2s + epsf
    upd = step_size * (m if flaw == "stale_m" else m1) / den
    p1 = p + upd if flaw == "sign" else p - upd
    assert p1.dtype == m1.dtype == v1.dtype == np.float32
    return p1, m1, v1


FLAWS = ("sign", "no_bc1", "no_bc2", "l2", "eps_in_sqrt", "stale_m", "betas_swapped", "fp32_one_minus_beta")


def _case(step, seed=0):
    return AR.synthetic(N, 1000 * seed + step, fresh=step == 1)


@pytest.mark.parametrize("hyper", sorted(AR.HYPERS))
def test_fp32_restatement_inside_bounds(hyper):
    hy = AR.HYPERS[hyper]
    worst = np.zeros(3)
    for step in AR.STEPS:
        P, m, v, G = _case(step)
        with np.errstate(under="ignore"):
            got = fp32_step(P, m, v, G, step, **hy)
        r = AR.ratios(got, P, m, v, G, [(0, N, 1, step)], **hy)
        worst = np.maximum(worst, [x.max() for x in r])
    print(f"AdamW fp32 restatement, {hyper}: worst error/tolerance P {worst[0]:.3f} m {worst[1]:.3f} v {worst[2]:.3f}")
    assert (worst < 1).all(), worst


def _torch_adamw64(P, m, v, G, step, lr, wd, b1, b2, eps):
    p = torch.nn.Parameter(torch.tensor(P, dtype=torch.float64))
    opt = torch.optim.AdamW([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False)
    opt.state[p] = {"step": torch.tensor(float(step - 1)), "exp_avg": torch.tensor(m, dtype=torch.float64),
                    "exp_avg_sq": torch.tensor(v, dtype=torch.float64)}
    p.grad = torch.tensor(G, dtype=torch.float64)
    opt.step()
    s = opt.state[p]
    assert float(s["step"]) == step
    return p.detach().numpy(), s["exp_avg"].numpy(), s["exp_avg_sq"].numpy()


@pytest.mark.parametrize("hyper", sorted(AR.HYPERS))
def test_torch_adamw_fp64_agrees(hyper):
    """torch.optim.AdamW on fp64 tensors (its scalars stay double): the replay
    is torch's formula, and the fp32 restatement is inside the bounds around
    torch's own result too."""
    hy = AR.HYPERS[hyper]
    worst = 0.0
    for step in AR.STEPS:
        P, m, v, G = _case(step)
        ref = _torch_adamw64(P, m, v, G, step, **hy)
        rep = AR.replay(P, m, v, G, [(0, N, 1, step)], **hy)
        tol = AR.bounds(P, m, v, G, [(0, N, 1, step)], **hy)
        with np.errstate(under="ignore"):
            got = fp32_step(P, m, v, G, step, **hy)
        for k, a, b, g, t in zip("Pmv", rep, ref, got, tol):
            # replay vs torch: only the seven scalars' fp32 rounding apart (each <= u relative)
            assert (np.abs(a - b) <= 0.5 * t).all(), (step, k, float((np.abs(a - b) / t).max()))
            r = float((np.abs(g.astype(np.float64) - b) / t).max())
            worst = max(worst, r)
            assert r < 1, (step, k, r)
    print(f"AdamW fp32 restatement vs torch fp64, {hyper}: worst error/tolerance {worst:.3f}")


@pytest.mark.parametrize("flaw", FLAWS)
def test_wrong_formulas_fall_outside(flaw):
    hy = AR.HYPERS["project"]
    out = n = 0
    per_step = {}
    for step in AR.STEPS:
        P, m, v, G = _case(step)
        with np.errstate(all="ignore"):
            got = fp32_step(P, m, v, G, step, flaw=flaw, **hy)
        r = AR.ratios(got, P, m, v, G, [(0, N, 1, step)], **hy)
        bad = (r[0] >= 1) | (r[1] >= 1) | (r[2] >= 1)
        per_step[step] = float(bad.mean())
        out += int(bad.sum())
        n += N
    print(f"{flaw}: fraction of elements outside the bound per step {per_step}")
    assert out >= 0.01 * n, (flaw, per_step)


def test_inactive_and_outside_unchanged():
    P, m, v, G = AR.synthetic(100, 5, fresh=False)
    tensors = [(3, 10, 1, 4), (20, 7, 0, 9), (40, 0, 1, 2), (50, 50, 1, 1, 5e-5)]
    hy = AR.HYPERS["project"]
    P1, m1, v1, d = AR.replay(P, m, v, G, tensors, **hy)
    tp, tm, tv = AR.bounds(P, m, v, G, tensors, **hy)
    act = AR.active_mask(100, tensors)
    assert act.sum() == 60 and not act[20:27].any()
    for a, b, t in ((P1, P, tp), (m1, m, tm), (v1, v, tv)):
        assert np.array_equal(a[~act], b[~act].astype(np.float64)) and (t[~act] == 0).all() and (t[act] > 0).all()
    assert (d[~act] == 0).all()
    # the tensor with its own learning rate: half the step of the shared one (zero decay apart)
    a = AR.replay(P, m, v, G, [(50, 50, 1, 1, 5e-5)], **hy)[3][50:]
    b = AR.replay(P, m, v, G, [(50, 50, 1, 1)], **hy)[3][50:]
    np.testing.assert_allclose(a, b / 2, rtol=1e-7)
