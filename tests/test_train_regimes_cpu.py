"""The tolerance of the training-regime GPU tests has teeth, and the plan query
they assert their regimes with answers without a device (no GPU here).

tests/test_gpu_train_regimes.py compares summed-over-the-batch gradients of up
to ~2,000 windows with ``close(rel=1e-3, abs_scale=1e-4)``.  A launch form that
dropped ONE window's contribution (a tile skipped, a part not summed) must not
fit inside that tolerance.  The summed loss is linear in the windows, so the
gradient without window i is the full gradient minus the gradient of window i
alone: here, in fp64 on the CPU, that difference exceeds the tolerance in
every trainable tensor, at the largest batch of each host count and for the
GAN sections.  Whoever loosens ``close`` for those tests meets this test first.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import pregan_train_oracle as TO
from preganplus_amd import _native
from preganplus_amd import train as TR
from preganplus_amd import weights as W
from tests.test_gpu_train import _autograd, _batched_case, close

GRAD = dict(rel=1e-3, abs_scale=1e-4)   # test_gpu_train_regimes.GRAD


def _grads(tw):
    return {k: v.grad.numpy().reshape(-1).copy() for k, v in tw.items() if v.grad is not None}


@pytest.mark.parametrize("H,B", [(50, 657), (16, 1025), (8, 2049)])
def test_one_dropped_window_exceeds_the_gradient_tolerance(H, B):
    w, x, y, mult, tgt = _batched_case(H, B, seed=3)
    full = _grads(_autograd(w, x, y, mult, tgt)[0])
    assert len(full) >= 30
    for i in (B - 1, B // 2):
        one = _grads(_autograd(w, x[i:i + 1], y[i:i + 1], mult[i:i + 1], tgt[i:i + 1])[0])
        for k, g in full.items():
            close(g, g, what=k, **GRAD)                      # (the check itself passes on the truth)
            with pytest.raises(AssertionError):
                close(g - one[k], g, what=f"{k} without window {i}", **GRAD)


def test_one_dropped_environment_exceeds_the_gan_tolerance():
    """The same for the Disc and Gen gradients of the batched GAN step at
    (50, 577) (7 k-slices): summed BCE toward per-window targets (Disc) and
    toward [0, 1] through the Disc (Gen), PreGANPlus.py:60-74."""
    H, B = 50, 577
    w = W.synth_weights(H, seed=4)
    rng = np.random.Generator(np.random.PCG64(21 + H + B))
    emb = np.where(rng.uniform(size=(B, H, 1)) < 0.3, rng.uniform(size=(B, H, 2)), 0.0)
    sched = np.zeros((B, H, H))
    sched[np.arange(B)[:, None], np.arange(H)[None, :], rng.integers(0, H, size=(B, H))] = 1.0
    lab = rng.uniform(size=B) < 0.5
    target = torch.tensor(np.stack([1.0 - lab, lab], axis=1).astype(np.float64))
    real = torch.tensor([0.0, 1.0], dtype=torch.float64).expand(B, 2)
    bce = torch.nn.functional.binary_cross_entropy

    def grads(sel):
        gw, dw = TO.leaf_params(w["gen"]), TO.leaf_params(w["disc"])
        e, s = torch.tensor(emb[sel]), torch.tensor(sched[sel])
        ns = TO.gen_t(gw, e, s)
        # per-window mean over the two outputs, summed over the windows
        (bce(TO.disc_t(dw, s, ns.detach()), target[sel], reduction="none").mean(-1).sum()).backward()
        d = {"disc " + k: v.grad.numpy().reshape(-1).copy() for k, v in dw.items()}
        for p in dw.values():
            p.grad = None
        (bce(TO.disc_t(dw, s, ns), real[sel], reduction="none").mean(-1).sum()).backward()
        d.update({"gen " + k: v.grad.numpy().reshape(-1).copy() for k, v in gw.items()})
        return d

    full = grads(slice(0, B))
    assert len(full) == 8
    for i in (B - 1, B // 2):
        one = grads(slice(i, i + 1))
        for k, g in full.items():
            with pytest.raises(AssertionError):
                close(g - one[k], g, what=f"{k} without environment {i}", **GRAD)


def test_plan_queries_answer_without_a_device():
    """pgp_tune_plan_info / pgp_gan_plan_info launch nothing: they answer on a
    machine without a GPU (256 CUs assumed), reject bad arguments, and a prefix
    backward reports the backward batch's geometry with the forward batch's
    forward."""
    L = _native.lib()
    info = TR.tune_plan_info(50, 657)
    assert set(info) == set(TR.TUNE_PLAN_FIELDS) and all(v >= 0 for v in info.values())
    assert info["bwd_grid"] >= 1 and info["bwd_units"] >= 1 and info["dw_blocks"] >= 1 and info["dec_dws"] >= 1
    # every unit / row block is carried by some wave / workgroup
    assert 4 * info["bwd_grid"] * info["bwd_units"] >= (657 * 50 + 15) // 16
    assert info["dw_grid"] * info["dw_blocks"] >= (657 * 150 + 31) // 32
    pre, fwd, bwd = TR.tune_plan_info(50, 430, fwd_batch=500), TR.tune_plan_info(50, 500), TR.tune_plan_info(50, 430)
    for k in ("fwd_side", "fwd_grid", "fwd_units", "dec_s"):
        assert pre[k] == fwd[k], k
    for k in ("bwd_side", "bwd_grid", "bwd_units", "lin_grid", "dw_grid", "dw_blocks", "dec_dws"):
        assert pre[k] == bwd[k], k
    out = (ctypes.c_int * 11)(*([-7] * 11))
    assert L.pgp_tune_plan_info(50, 500, 430, out, 3) == 11 and list(out)[3:] == [-7] * 8   # cap respected
    assert L.pgp_tune_plan_info(50, 430, 500, out, 11) == -1      # backward batch > forward batch
    assert L.pgp_tune_plan_info(50, 500, 0, out, 11) == -1
    assert L.pgp_tune_plan_info(50, 500, 430, None, 11) == -1
    assert L.pgp_tune_plan_info(7, 4, 4, out, 11) == -2
    assert TR.gan_plan_info(16, 37) == 1 and TR.gan_plan_info(50, 1) > 1
    assert L.pgp_gan_plan_info(7, 4) == -2 and L.pgp_gan_plan_info(50, 0) == -1
    with pytest.raises(_native.NativeError):
        TR.tune_plan_info(50, 500, fwd_batch=430)
