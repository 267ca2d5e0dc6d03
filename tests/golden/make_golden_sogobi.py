"""Golden fixture for second-order GOBI: the reference's own so_opt, run here.

  scheduler/SOGOBI.py:18-40            run_SOGOBI: the init of run_GOBI, then so_opt
  scheduler/BaGTI/src/opt.py:35-51     so_opt(): Adahessian(lr 0.8) + CosineAnnealingLR(T_max 10) on
                                       the input, one-hot projection per step, stop after 31
                                       unchanged steps or 200 iterations
  scheduler/BaGTI/src/adahessian.py:49-168  the Hutchinson probe v = 2 randint_like(p, 2) - 1,
                                       hv = grad(g . v), the moments and the update

Imports /root/reference/scheduler/BaGTI (read-only; run with python -B so no
bytecode is written there), loads the shipped checkpoint with
torch.load(weights_only=True), and runs so_opt on the 240 inits of
tests/golden/gobi_h16.npz (reused, not stored again) with
torch.manual_seed(environment index) before each run.  Nothing of the reference
is changed: the draws and the first step's values are recorded by wrapping
torch.randint_like, torch.autograd.grad and opt.convertToOneHot for the run.

Writes
  tests/golden/sogobi_h16.npz       sign_offsets [241] (steps before environment e), sign_words
                                    [steps, 9] uint32 (bit k of word k >> 5 set: v = +1 at row-major
                                    entry k = c * 18 + f), results, iterations, fitness
  tests/golden/sogobi_h16_taps.npz  the first step's g, hv and pre-projection x, [240, 16, 18] each
                                    (a file of its own: with the signs it would pass 1 MiB)
"""
import os
import sys

import numpy as np
import torch

REF = "/root/reference/scheduler/BaGTI"
OUT = os.path.dirname(os.path.abspath(__file__))
H = 16


def pack_signs(v):
    """[..., 16, 18] of +-1 -> [..., 9] uint32, bit k of word k >> 5 set for +1."""
    b = (np.asarray(v).reshape(*np.shape(v)[:-2], 9, 32) > 0).astype(np.uint64)
    return (b << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)


def main():
    sys.path.insert(0, REF)
    sys.argv = ["make_golden_sogobi", "-", "-"]  # models.py:25 reads argv[0], argv[2]
    from src.models import energy_latency_16  # noqa: E402
    import src.opt as ref_opt  # noqa: E402

    model = energy_latency_16()
    ck = torch.load(os.path.join(REF, "checkpoints", "energy_latency_16_Trained.ckpt"), weights_only=True,
                    map_location="cpu")
    model.load_state_dict(ck["model_state_dict"])
    inits = np.load(os.path.join(OUT, "gobi_h16.npz"))["inits"]

    real_randint, real_grad, real_onehot = torch.randint_like, torch.autograd.grad, ref_opt.convertToOneHot
    offsets, words, results, iters, fitness, g1, hv1, pre1 = [0], [], [], [], [], [], [], []
    for e, x in enumerate(inits):
        draws, first = [], {}

        def randint_like(p, high=2, **kw):
            r = real_randint(p, high=high, **kw)
            draws.append((2 * r - 1).numpy().copy())
            return r

        def grad(outputs, inputs, *a, **kw):
            hvs = real_grad(outputs, inputs, *a, **kw)
            if "hv" not in first:  # get_trace: outputs = [p.grad], hvs = (H v,)
                first["g"] = outputs[0].detach().numpy().copy()
                first["hv"] = hvs[0].detach().numpy().copy()
            return hvs

        def onehot(dat, cpu_old, hosts):
            if "pre" not in first:
                first["pre"] = dat.detach().numpy().copy()
            return real_onehot(dat, cpu_old, hosts)

        torch.randint_like, torch.autograd.grad, ref_opt.convertToOneHot = randint_like, grad, onehot
        try:
            torch.manual_seed(e)
            init = torch.tensor(x, dtype=torch.float, requires_grad=True)  # SOGOBI.py:33
            res, it, fit = ref_opt.so_opt(init, model, [], "energy_latency_16")
        finally:
            torch.randint_like, torch.autograd.grad, ref_opt.convertToOneHot = real_randint, real_grad, real_onehot
        words.append(pack_signs(np.stack(draws)))
        offsets.append(offsets[-1] + len(draws))
        results.append(res.numpy().copy())
        iters.append(it)
        fitness.append(float(fit))
        g1.append(first["g"])
        hv1.append(first["hv"])
        pre1.append(first["pre"])
    np.savez_compressed(os.path.join(OUT, "sogobi_h16.npz"), sign_offsets=np.array(offsets, np.int32),
                        sign_words=np.concatenate(words), results=np.stack(results).astype(np.float32),
                        iterations=np.array(iters, np.int32), fitness=np.array(fitness, np.float64))
    np.savez_compressed(os.path.join(OUT, "sogobi_h16_taps.npz"), g=np.stack(g1), hv=np.stack(hv1),
                        pre=np.stack(pre1))
    print("steps", offsets[-1], "iterations min/mean/max", min(iters), np.mean(iters), max(iters))


if __name__ == "__main__":
    main()
