#!/usr/bin/env python3
"""Times the FPE's epoch-per-launch and fleet entries against the
lone two-launch loop.

One process = one fleet size of one host count = one record (a JSON line, also
written to --out), as tools/gobi_fleet_time.py:

    for M in 1 16 64 256 512; do python tools/fpe_fleet_time.py --hosts 16 --models $M --out f16_$M.json; done

  many.us_per_step       pgp_fpe_train_steps_many, `--steps` steps of all M models in one
                         launch (every model on the same windows, its own slot and GRU
                         states), launch time over the step count
  many.forward_us        pgp_fpe_forward_many_cells, M x steps windows in one launch
With --models 1 the record also holds, for ONE model:
  lone.event_us_per_step / lone.host_us_per_step
                         FPETrainer.backprop (pgp_fpe_train_step + pgp_adamw_d per window,
                         uploads and the read-back included): between device events, and
                         on the host clock (what a caller pays)
  one.us_per_step        pgp_fpe_train_steps, the same steps in one launch
  one.no_adam_us_per_step  the same launch with an empty tensor table (the step alone):
                         the difference to one.us_per_step is the in-kernel AdamW
  one.backprop_host_us_per_step  FPETrainer.backprop(one_launch=True) on the host clock
Times are device events around the launch unless named host; the median of
--reps after --warmup, with min and max.  Select the library with PGP_LIB.
There is no CPU path: without a GPU the tool fails.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(ms, per):
    us = [1e3 * m / per for m in ms]
    return {"median": round(statistics.median(us), 3), "min": round(min(us), 3), "max": round(max(us), 3)}


def timed(fn, warmup, reps, per, host=False):
    """(device-event stats, host-clock stats) of fn() in us per `per`."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev, hs = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        b.synchronize()
        hs.append(1e3 * (time.perf_counter() - t0))
        ev.append(a.elapsed_time(b))
    return (stats(ev, per), stats(hs, per)) if host else stats(ev, per)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--hosts", type=int, default=16)
    ap.add_argument("--models", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fpe_fleet_time: no GPU (there is no CPU path)")

    from preganplus_amd import _native
    from preganplus_amd import fpetrain as FT
    from preganplus_amd import train as TR
    from preganplus_amd import weights as W

    H, M, n = a.hosts, a.models, a.steps
    L, vp = _native.lib(), ctypes.c_void_p
    rec = {"hosts": H, "models": M, "steps": n, "warmup": a.warmup, "reps": a.reps,
           "lib": os.path.basename(_native.LIB_PATH), "device": torch.cuda.get_device_name(0)}
    w = W.synth_fpe_weights(H, seed=0)
    rng = np.random.Generator(np.random.PCG64(H))
    wins = rng.uniform(0, 1, size=(n, 3, 3 * H))
    anom = (rng.uniform(size=(n, H)) < 0.2).astype(np.int32)
    cls = rng.integers(0, 3, size=(n, H)).astype(np.int32)
    protos = np.asarray(w["prototypes"], dtype=np.float64)[:3]
    stream = lambda: vp(torch.cuda.current_stream().cuda_stream)
    dev = lambda x, dt: torch.as_tensor(np.asarray(x), dtype=dt).cuda().contiguous()

    # ---- M models in one launch: the same windows, each model its own slot, state and GRU states ----
    ft = FT.FPETrainer(w["fpe"], H=H)
    nt, ln = len(ft.tensors), ft.P.numel()
    wd, yd, cd = dev(wins, torch.float32), dev(anom, torch.int32), dev(cls, torch.int32)
    h0 = dev(rng.standard_normal((M * n, 3)), torch.float32)
    table = FT.adam_table([dict(t, step=100.0) for t in ft.tensors], anom.any(axis=1), ft.lr, ft.b1, ft.b2)
    sched = dev(np.tile(table, (M, 1, 1)), torch.float32)
    loss = torch.zeros((M * n, 2), dtype=torch.float64, device="cuda")
    P = ft.P.repeat(M, 1).contiguous()
    G, m, v = torch.zeros_like(P), torch.zeros_like(P), torch.zeros_like(P)
    state = dev(np.tile(TR.TuneState(protos, 0.2).vector(), (M, 1)), torch.float64)
    jobs = np.zeros(M, dtype=FT.JOB_DTYPE)
    jobs["step_off"], jobs["n"] = np.arange(M) * n, n
    jobs_dev = torch.empty(M * FT.JOB_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    desc = ft._desc()

    def many(ntensors=nt):
        _native.check(L.pgp_fpe_train_steps_many(
            H, 3, M, jobs.ctypes.data, n, wd.data_ptr(), yd.data_ptr(), cd.data_ptr(), M * n, h0.data_ptr(),
            sched.data_ptr(), loss.data_ptr(), P.data_ptr(), G.data_ptr(), m.data_ptr(), v.data_ptr(),
            state.data_ptr(), TR.PROTO_UPDATE_MIN, 1.0, ft.lr, ft.wd, ft.b1, ft.b2, ft.eps, desc, ntensors,
            jobs_dev.data_ptr(), stream()), "pgp_fpe_train_steps_many")

    out = torch.zeros((2, M * n, H, 2), dtype=torch.float64, device="cuda")

    def forward():
        _native.check(L.pgp_fpe_forward_many_cells(H, M, jobs.ctypes.data, n, wd.data_ptr(), M * n, h0.data_ptr(),
                                                   P.data_ptr(), out[0].data_ptr(), out[1].data_ptr(),
                                                   jobs_dev.data_ptr(), stream()), "pgp_fpe_forward_many_cells")

    rec["many"] = {"us_per_step": timed(many, a.warmup, a.reps, n),
                   "forward_us": timed(forward, a.warmup, a.reps, 1)}
    assert torch.isfinite(P).all() and torch.isfinite(out).all()

    # ---- one model: the lone loop, one launch, and the step without its AdamW ----
    if M == 1:
        h1 = rng.standard_normal((n, 3))
        lone = FT.FPETrainer(w["fpe"], H=H)
        st = TR.TuneState(protos, 0.2)
        ev, hs = timed(lambda: lone.backprop(st, wins, h1, anom, cls), a.warmup, a.reps, n, host=True)
        rec["lone"] = {"event_us_per_step": ev, "host_us_per_step": hs}
        one = FT.FPETrainer(w["fpe"], H=H)
        _, hs = timed(lambda: one.backprop(st, wins, h1, anom, cls, one_launch=True), a.warmup, a.reps, n, host=True)

        def single(ntensors=nt):   # slot 0 of the fleet's buffers
            _native.check(L.pgp_fpe_train_steps(
                H, 3, n, wd.data_ptr(), h0.data_ptr(), yd.data_ptr(), cd.data_ptr(), P.data_ptr(), G.data_ptr(),
                m.data_ptr(), v.data_ptr(), state.data_ptr(), TR.PROTO_UPDATE_MIN, 1.0, ft.lr, ft.wd, ft.b1, ft.b2,
                ft.eps, desc, ntensors, sched.data_ptr(), loss.data_ptr(), stream()), "pgp_fpe_train_steps")
        rec["one"] = {"us_per_step": timed(single, a.warmup, a.reps, n),
                      "no_adam_us_per_step": timed(lambda: single(0), a.warmup, a.reps, n),
                      "backprop_host_us_per_step": hs}
        assert torch.isfinite(lone.P).all() and torch.isfinite(one.P).all()
    line = json.dumps(rec, sort_keys=True)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
