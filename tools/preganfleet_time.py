#!/usr/bin/env python3
"""Times one interval of the PreGAN fleet plugin against lone plugins.

One process = one fleet size = one record (a JSON line, also written to --out), as
tools/fpe_fleet_time.py:

    for M in 1 16 64 256; do python tools/preganfleet_time.py --cells $M --out pf_$M.json; done

16 hosts, K = 3, seeded weights (synth_fpe_weights(16, 11): every window is anomalous, so
every cell takes the whole interval), training on, fake environments whose runSimulation
returns at once (the simulator's own time is the caller's, not the plugin's).

  fleet.detect_us            pgp_fpe_forward1_many alone, all M cells in one launch, between
                             device events (inputs already on the device)
  fleet.run_model_host_us    PreGANFleetRecovery.run_model on the host clock: window building,
                             upload, detect, download, FleetTuner.train_gan (two launches, 2M
                             simulator calls), one K5 call, the decisions
  lone.default_host_us       M PreGANRecovery.run_model calls back to back, host clock, default
                             path (packed K4 + K3 at batch 1, lone train_gan graphs, host repack,
                             batched gan_forward, K5)
  lone.master_host_us        the same with master_forward=True (pgp_fpe_forward1, no repack)
The M lone calls cycle over min(M, --lone-plugins) plugin objects (every call is a whole
run_model on its own weights; building hundreds of lone plugins with their graphs is not
what is measured).  Median of --reps after --warmup, with min and max.  Select the library
with PGP_LIB.  There is no CPU path: without a GPU the tool fails.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H = 16


def stats(ms):
    us = [1e3 * m for m in ms]
    return {"median": round(statistics.median(us), 1), "min": round(min(us), 1), "max": round(max(us), 1)}


def timed(fn, warmup, reps, host=False):
    """Device-event (or host-clock) stats of fn() in us."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(1e3 * (time.perf_counter() - t0) if host else a.elapsed_time(b))
    return stats(out)


class _Obj:
    pass


class _Container:
    def __init__(self, cid, host):
        self.id, self._host = cid, host

    def getHostID(self):
        return self._host


def fake_env(rng):
    """The fields run_model reads, with a runSimulation that returns at once."""
    env = _Obj()
    env.hostlist = list(range(H))
    env.containerlist = [_Container(c, int(rng.integers(0, H))) for c in range(H)]
    env.scheduler = _Obj()
    env.scheduler.result_cache = rng.uniform(0, 1, size=(H, H))
    env.stats = _Obj()
    env.stats.time_series = rng.uniform(0, 1.2, size=(5, 3 * H))
    env.stats.schedule_series = None
    env.stats.runSimulation = lambda sched: (1.0, 0.5)
    return env


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cells", type=int, default=1)
    ap.add_argument("--lone-plugins", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("preganfleet_time: no GPU (there is no CPU path)")

    from preganplus_amd import _native
    from preganplus_amd import weights as W
    from preganplus_amd.recovery import PreGANFleetRecovery, PreGANRecovery

    M = a.cells
    rec = {"hosts": H, "cells": M, "warmup": a.warmup, "reps": a.reps, "lib": os.path.basename(_native.LIB_PATH),
           "device": torch.cuda.get_device_name(0)}
    w = W.synth_fpe_weights(H, seed=11)
    extra = {"train_time_data": np.ones((2, 3 * H))}
    rng = np.random.Generator(np.random.PCG64(M))
    envs = [fake_env(rng) for _ in range(M)]
    decisions = [[(c, (c + 1) % H) for c in range(0, H, 4)] for _ in range(M)]
    h0 = rng.standard_normal((M, 3))

    # ---- the fleet ----
    fleet = PreGANFleetRecovery(H, [w] * M, [extra] * M, training=True)
    fleet.setEnvironments(envs)
    wins = np.stack([fleet._input_window(m) for m in range(M)])
    scheds = np.stack([e.scheduler.result_cache for e in envs])
    out = fleet.forward(wins, h0, scheds)
    if not out["any"].all():
        sys.exit(f"preganfleet_time: {int((out['any'] == 0).sum())} of {M} cells see no anomaly")
    io = fleet._io
    rec["fleet"] = {
        "detect_us": timed(lambda: io.launch(fleet.fpe_P, fleet.tuner.P, fleet.prototypes, upload=False),
                           a.warmup, a.reps),
        "run_model_host_us": timed(lambda: fleet.run_model(decisions, h0=h0), a.warmup, a.reps, host=True)}
    # GAN steps taken against calls made: equal when every call of every cell took the whole interval
    rec["fleet"]["gan_steps"] = [int(sum(fleet.epoch)), M * (a.warmup + a.reps)]
    assert torch.isfinite(fleet.tuner.P).all()

    # ---- M lone run_model calls, in this process ----
    n = min(M, a.lone_plugins)
    rec["lone"] = {"plugins": n}
    for key, mf in (("default_host_us", False), ("master_host_us", True)):
        lones = [PreGANRecovery(H, "", training=True, weights=w, extra=extra, master_forward=mf) for _ in range(n)]

        def calls():
            for m in range(M):
                p = lones[m % n]
                p.setEnvironment(envs[m])
                p.run_model(None, decisions[m])
        rec["lone"][key] = timed(calls, a.warmup, a.reps, host=True)
        rec["lone"][key]["gan_steps"] = [int(sum(p.epoch for p in lones)), M * (a.warmup + a.reps)]
        for p in lones:
            p.close()
        del lones
    line = json.dumps(rec, sort_keys=True)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
