#!/usr/bin/env python3
"""Time the fused batch-1 tuning step (csrc/pgp_tune1.hip) with and without
train-mode dropout on the GPU.

  python tools/tune1_dropout_time.py [--hosts 16] [--steps 50] [--replays 4] [--reps 7] [--p 0.1]

A captured graph of `--steps` x (step + AdamW from a device table), the form
backprop() replays, timed with HIP events over `--replays` replays after a
warm-up; `--reps` figures each, median / min / max in microseconds per step:
  step_us          pgp_tune_step1 + pgp_adamw_table (the existing entry)
  step_dropout_us  pgp_tune_step1_dropout at p + pgp_adamw_table (when the
                   library has the entry: an older library reports only step_us)
  masks_us         pgp_tune_dropout_masks alone (the mask generation by itself,
                   an upper bound on its share: in the step it runs beside the
                   weight copy's loads, before the first barrier)
Select the library with PGP_LIB to compare two builds, in alternating
processes.  Prints one JSON line per host count.  There is no CPU path.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from preganplus_amd import _native  # noqa: E402
from preganplus_amd import train as TR  # noqa: E402
from preganplus_amd import weights as W  # noqa: E402


def timed(fn, reps):
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


def measure(H, steps, replays, reps, p):
    tr = TR.Trainer(H, W.synth_weights(H, seed=3), max_batch=1)
    L, dev = tr._L, tr.device
    rng = np.random.Generator(np.random.PCG64(H))
    x = rng.uniform(0, 0.8, size=(3, 3 * H))
    x = np.where(rng.uniform(size=x.shape) < 0.03, rng.uniform(0.9, 1.3, size=x.shape), x)
    win = torch.tensor(x, dtype=torch.float32, device=dev)
    y = torch.tensor(rng.uniform(size=H) < 0.3, dtype=torch.int32, device=dev)
    c = torch.tensor(rng.integers(0, 3, size=H), dtype=torch.int32, device=dev)
    state0 = TR.TuneState(rng.uniform(0.1, 0.9, (H, 2)), 0.2).to_device(dev)
    state = state0.clone()
    K = (state.numel() - 3) // 2
    loss = torch.zeros(2, dtype=torch.float64, device=dev)
    sel = [t for t in tr.tensors if t["section"] == "transformer" and t["trainable"]]
    tab = torch.tensor(tr.adam_schedule_np("transformer", np.ones(steps, dtype=bool), ()), device=dev)
    words = torch.tensor(np.array([12345, 100], dtype=np.int64), device=dev)   # {seed, base step}
    has_drop = hasattr(L, "pgp_tune_step1_dropout")   # absent from a build before the dropout step (PGP_LIB)

    def step(i, drop):
        args = (H, K, win.data_ptr(), y.data_ptr(), c.data_ptr(), tr.P.data_ptr(), tr.G.data_ptr(), state.data_ptr(),
                TR.PROTO_UPDATE_MIN, TR.PROTO_FACTOR_DECAY, tr.logits.data_ptr(), tr.protos.data_ptr(),
                loss.data_ptr())
        if drop:
            _native.check(L.pgp_tune_step1_dropout(*args, p, words.data_ptr(), i, tr._stream()), "step_dropout")
        else:
            _native.check(L.pgp_tune_step1(*args, tr._stream()), "step")
        tr.adam_step_table("transformer", sel, tab[i])

    def capture(drop):
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(g):
            for i in range(steps):
                step(i, drop)
        return g

    P0 = tr.P.clone()
    res = {"hosts": H, "lib": os.path.basename(_native.LIB_PATH), "steps": steps, "replays": replays, "reps": reps}
    forms = [("step_us", False)] + ([("step_dropout_us", True)] if has_drop else [])
    for name, drop in forms:
        g = capture(drop)

        def run():
            for _ in range(replays):
                g.replay()

        run()      # warm-up
        torch.cuda.synchronize()
        res[name] = stats(timed(run, reps), steps * replays)
        assert torch.isfinite(tr.P).all()
        tr.P.copy_(P0)
        tr.m.zero_()
        tr.v.zero_()
        state.copy_(state0)
    if has_drop:
        res["p"] = p
        keep = torch.empty(int(L.pgp_tune_dropout_mask_len(H)), dtype=torch.uint8, device=dev)
        n = steps * replays

        def run_masks():
            for i in range(n):
                L.pgp_tune_dropout_masks(H, p, words.data_ptr(), i, keep.data_ptr(), tr._stream())

        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(g):
            run_masks()
        g.replay()
        torch.cuda.synchronize()
        res["masks_us"] = stats(timed(g.replay, reps), n)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--hosts", default="16")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--replays", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--p", type=float, default=0.1)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tune1_dropout_time: no GPU (there is no CPU path)")
    for H in (int(h) for h in a.hosts.split(",")):
        print(json.dumps(measure(H, a.steps, a.replays, a.reps, a.p)), flush=True)


if __name__ == "__main__":
    main()
