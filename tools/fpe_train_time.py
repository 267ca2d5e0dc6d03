#!/usr/bin/env python3
"""Time the offline FPE training kernels (csrc/pgp_fpetrain.hip) on the GPU.

  python tools/fpe_train_time.py [--hosts 16,50] [--steps 200] [--windows 4096] [--reps 7]

Per host count, with HIP events after a warm-up, on the current stream:
  step_us     one pgp_fpe_train_step + pgp_adamw (the pair a training step is):
              the time of `--steps` consecutive pairs over their count
  forward_us  one window of pgp_fpe_forward_many at n = `--windows`
Each figure is taken `--reps` times; the median, the minimum and the maximum
are reported (the spread is what a difference between two builds has to
exceed).  The steps are issued back to back through ctypes, so step_us is the
larger of the device time and the host's issue time of the pair; both builds of
an A/B pay the same host path.  Select the library with PGP_LIB (make variant)
to compare two builds, in alternating processes.  Prints one JSON line per host
count.  There is no CPU path: without a GPU the tool fails.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from preganplus_amd import _native, adamw  # noqa: E402
from preganplus_amd import fpetrain as FT  # noqa: E402
from preganplus_amd import train as TR  # noqa: E402
from preganplus_amd import weights as W  # noqa: E402


def timed(fn, reps):
    """ms of fn() per repetition, HIP events around it."""
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def stats(ms, per):
    us = sorted(1e3 * m / per for m in ms)
    return {"median": round(us[len(us) // 2], 3), "min": round(us[0], 3), "max": round(us[-1], 3)}


def measure(H, steps, windows, reps):
    w = W.synth_fpe_weights(H, seed=0)
    ft = FT.FPETrainer(w["fpe"], H=H)
    L, vp = ft._L, ctypes.c_void_p
    rng = np.random.Generator(np.random.PCG64(H))
    dev = lambda a, dt: torch.as_tensor(a, dtype=dt).cuda().contiguous()
    win = dev(rng.uniform(0, 1, size=(3, 3 * H)), torch.float32)
    h0 = dev(rng.standard_normal(3), torch.float32)
    y = dev(rng.uniform(size=H) < 0.2, torch.int32)
    c = dev(rng.integers(0, 3, size=H), torch.int32)
    state = torch.tensor(TR.TuneState(w["prototypes"], 0.2).vector(), dtype=torch.float64, device="cuda")
    loss = torch.zeros(2, dtype=torch.float64, device="cuda")
    # AdamW descriptors of a mid-training step (the bias corrections are host scalars)
    rows = FT.adam_rows([dict(t, step=99.0) for t in ft.tensors], True, ft.lr, ft.b1, ft.b2)
    desc = adamw.descriptors(ft.tensors, rows)
    stream = ft._stream()
    P, G, m, v = (vp(t.data_ptr()) for t in (ft.P, ft.G, ft.m, ft.v))

    def run_steps():
        for _ in range(steps):
            rc = L.pgp_fpe_train_step(H, 3, win.data_ptr(), h0.data_ptr(), y.data_ptr(), c.data_ptr(), P, G,
                                      state.data_ptr(), TR.PROTO_UPDATE_MIN, 1.0, loss.data_ptr(), stream)
            rc |= L.pgp_adamw_d(P, G, m, v, ft.lr, ft.wd, ft.b1, ft.b2, ft.eps, desc, len(desc), stream)
            if rc:
                _native.check(rc, "step")

    wins = dev(rng.uniform(0, 1, size=(windows, 3, 3 * H)), torch.float32)
    h0s = dev(rng.standard_normal((windows, 3)), torch.float32)
    out = torch.zeros((2, windows, H, 2), dtype=torch.float64, device="cuda")

    def run_forward():
        _native.check(L.pgp_fpe_forward_many(H, windows, wins.data_ptr(), h0s.data_ptr(), ft.P.data_ptr(),
                                             out[0].data_ptr(), out[1].data_ptr(), stream), "forward_many")

    run_steps()          # warm-up: code objects loaded, clocks up
    run_forward()
    torch.cuda.synchronize()
    res = {"hosts": H, "lib": os.path.basename(_native.LIB_PATH), "steps": steps, "windows": windows, "reps": reps,
           "step_us": stats(timed(run_steps, reps), steps),
           "forward_us_per_window": stats(timed(run_forward, reps), windows)}
    assert torch.isfinite(ft.P).all() and torch.isfinite(out).all()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--hosts", default="16,50")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--windows", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fpe_train_time: no GPU (there is no CPU path)")
    for H in (int(h) for h in a.hosts.split(",")):
        print(json.dumps(measure(H, a.steps, a.windows, a.reps)), flush=True)


if __name__ == "__main__":
    main()
