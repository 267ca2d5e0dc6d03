#!/usr/bin/env python3
"""Time one interval's tuning of a fleet of cells on the GPU: ``FleetTuner.tune``
(one graph of 2n + 1 launches for all cells) next to what it replaces, M lone
``backprop`` graphs replayed one after another.

  python tools/fleettune_time.py [--hosts 16] [--n 10] [--cells 1,16,64,256,512] [--p 0,0.1] [--reps 7]
                                 [--out profiles/r12/fleettune]

Per (p, M), HIP events around the graph replays alone (inputs already on the
device), `--reps` figures each after a warm-up, median / min / max:
  fleet_ms       one replay of the fleet graph (every cell active, score=True)
  lone_ms        M replays of a lone backprop(score=True) graph, back to back
                 on one stream (the same Trainer each time: the launches and
                 their cost do not depend on the weights)
  fleet_call_ms  the whole FleetTuner.tune() call on the host clock: staging,
                 upload, replay, download, per-cell scores
Writes fleettune.jsonl (one line per (p, M)) and summary.md into --out and
prints the lines.  There is no CPU path.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from preganplus_amd import train as TR  # noqa: E402
from preganplus_amd import weights as W  # noqa: E402


def stats(ms):
    s = sorted(ms)
    return {"median": round(s[len(s) // 2], 4), "min": round(s[0], 4), "max": round(s[-1], 4)}


def events(fn, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def data(H, M, n, seed):
    r = np.random.default_rng(seed)
    wins = r.uniform(0, 1, (M, n, 3, 3 * H)).astype(np.float32)
    anom = (r.uniform(size=(M, n, H)) < 0.25).astype(np.int32)
    anom[:, 0, 1] = 1
    return wins, anom, r.integers(0, 3, (M, n, H)).astype(np.int32)


def measure(H, n, M, p, reps):
    base = [W.synth_weights(H, seed=s) for s in range(min(M, 8))]
    ft = TR.FleetTuner(H, [base[m % len(base)] for m in range(M)], dropout=p, dropout_seeds=list(range(1, M + 1)))
    wins, anom, cls = data(H, M, n, seed=M)
    ft.tune(wins, anom, cls)                                  # captures the graph, warms up
    g = ft.graph(n, True)
    fleet = events(g.graph.replay, reps)
    host = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ft.tune(wins, anom, cls)
        host.append(1e3 * (time.perf_counter() - t0))
    tr = TR.Trainer(H, base[0], max_batch=1, dropout=p, dropout_seed=1)
    st = TR.TuneState(base[0]["prototypes"])
    TR.backprop(tr, st, wins[0], anom[0], cls[0], score=True)
    lg = next(iter(tr._graphs.values()))

    def lone_all():
        for _ in range(M):
            lg.graph.replay()

    lone = events(lone_all, reps)
    f, l = stats(fleet), stats(lone)
    return {"hosts": H, "n": n, "cells": M, "p": p, "fleet_ms": f, "lone_ms": l, "fleet_call_ms": stats(host),
            "fleet_us_per_cell": round(1e3 * f["median"] / M, 2), "lone_us_per_cell": round(1e3 * l["median"] / M, 2),
            "speedup": round(l["median"] / f["median"], 2), "device": torch.cuda.get_device_name(0),
            "cus": torch.cuda.get_device_properties(0).multi_processor_count}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hosts", type=int, default=16)
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--cells", default="1,16,64,256,512")
    ap.add_argument("--p", default="0,0.1")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="profiles/r12/fleettune")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    rows = []
    with open(os.path.join(a.out, "fleettune.jsonl"), "w") as f:
        for p in (float(x) for x in a.p.split(",")):
            for M in (int(x) for x in a.cells.split(",")):
                r = measure(a.hosts, a.n, M, p, a.reps)
                rows.append(r)
                line = json.dumps(r)
                print(line, flush=True)
                f.write(line + "\n")
    with open(os.path.join(a.out, "summary.md"), "w") as f:
        f.write(f"# FleetTuner.tune, H = {a.hosts}, n = {a.n}, score=True ({rows[0]['device']}, {rows[0]['cus']} CUs)\n\n")
        f.write("Graph replay between HIP events, median (min-max) of %d, ms.\n\n" % a.reps)
        f.write("| p | cells | fleet graph | per cell (us) | M lone graphs | per cell (us) | lone / fleet | tune() host |\n")
        f.write("|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            fm, lm, hm = r["fleet_ms"], r["lone_ms"], r["fleet_call_ms"]
            f.write(f"| {r['p']} | {r['cells']} | {fm['median']} ({fm['min']}-{fm['max']}) | {r['fleet_us_per_cell']} | "
                    f"{lm['median']} ({lm['min']}-{lm['max']}) | {r['lone_us_per_cell']} | {r['speedup']} | "
                    f"{hm['median']} |\n")


if __name__ == "__main__":
    main()
