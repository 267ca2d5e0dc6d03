#!/usr/bin/env python3
"""Time the training kernels of GOBI's surrogate (csrc/pgp_gobitrain.hip).

  python tools/gobi_train_time.py [--steps 159] [--eval 40] [--reps 9] [--cpu-steps 159]

With HIP events after a warm-up, on the current stream, over a synthetic
dataset of the reference's shape (199 samples of [16,18], one-hot allocations):
  step_us        one step of pgp_gobi_train_steps: a launch of `--steps`
                 sequential steps (159: one reference epoch's train part) over
                 their count
  eval_us        one sample of pgp_gobi_train_eval at n = `--eval` (40: one
                 epoch's validation part) and at n = 199
and, on this machine's CPU (torch's threads as the environment sets them), the
same quantities for the tests' restatement of the reference's loop
(tests/gobitrain_ref.py, fp32): cpu_step_us, cpu_eval_us.  Each GPU figure is
taken `--reps` times; median, minimum and maximum are reported.  Run it in
several processes to see the process-to-process spread.  Prints one JSON line.
There is no CPU path for the kernels: without a GPU the tool fails.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from preganplus_amd import _native  # noqa: E402
from preganplus_amd import gobitrain as GT  # noqa: E402
from tests import gobitrain_ref as R  # noqa: E402


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


def dataset(n=199, seed=0):
    rng = np.random.Generator(np.random.PCG64(seed))
    feats = np.zeros((n, 16, 18))
    feats[:, :, 0] = rng.uniform(0, 1, (n, 16))
    feats[:, :, 1] = rng.uniform(0, 1, (n, 16)) * (rng.uniform(size=(n, 16)) < 0.7)
    host = rng.integers(-1, 16, (n, 16))
    i, c = np.nonzero(host >= 0)
    feats[i, c, 2 + host[i, c]] = 1
    return feats, rng.uniform(0, 1, (n, 2)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=159)
    ap.add_argument("--eval", type=int, default=40)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--cpu-steps", type=int, default=159)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gobi_train_time: no GPU (there is no CPU path)")
    feats, targets = dataset()
    w0 = GT.fresh_weights(0)
    t = GT.GOBITrainer(weights=w0)
    t.set_data(feats, targets)
    rng = np.random.Generator(np.random.PCG64(1))
    order = rng.integers(0, len(feats), a.steps)
    dev = lambda o: torch.as_tensor(np.asarray(o, dtype=np.int32)).cuda()
    o_steps, o_eval, o_all = dev(order), dev(order[:a.eval] % len(feats)), dev(np.arange(len(feats)))
    loss = torch.empty(max(a.steps, len(feats)), device="cuda")
    stream = t._stream()

    def run_steps():
        _native.check(t._L.pgp_gobi_train_steps(16, t.n_samples, a.steps, t.feats.data_ptr(), t.targets.data_ptr(),
                                                o_steps.data_ptr(), t.P.data_ptr(), t.m.data_ptr(), t.v.data_ptr(),
                                                t.step, t.lr, t.wd, t.b1, t.b2, t.eps, loss.data_ptr(), stream), "steps")
        t.step += a.steps

    def run_eval(o):
        _native.check(t._L.pgp_gobi_train_eval(16, t.n_samples, int(o.numel()), t.feats.data_ptr(),
                                               t.targets.data_ptr(), o.data_ptr(), t.P.data_ptr(), loss.data_ptr(),
                                               stream), "eval")

    run_steps()   # warm-up: code object loaded, clocks up
    run_eval(o_all)
    torch.cuda.synchronize()
    res = {"lib": os.path.basename(_native.LIB_PATH), "steps": a.steps, "reps": a.reps,
           "step_us": stats(timed(run_steps, a.reps), a.steps),
           f"eval_us_n{a.eval}": stats(timed(lambda: run_eval(o_eval), a.reps), a.eval),
           f"eval_us_n{len(feats)}": stats(timed(lambda: run_eval(o_all), a.reps), len(feats))}
    assert torch.isfinite(t.P).all() and torch.isfinite(loss).all()
    # the restatement of the reference's CPU loop, fp32, here
    R.run(w0, feats, targets, order[:8])
    t0 = time.perf_counter()
    R.run(w0, feats, targets, order[:a.cpu_steps])
    res["cpu_step_us"] = round(1e6 * (time.perf_counter() - t0) / a.cpu_steps, 1)
    t0 = time.perf_counter()
    R.losses(w0, feats, targets, np.arange(len(feats)), dtype=torch.float32)
    res["cpu_eval_us"] = round(1e6 * (time.perf_counter() - t0) / len(feats), 1)
    res["cpu_threads"] = torch.get_num_threads()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
