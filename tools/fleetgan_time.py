#!/usr/bin/env python3
"""Time one interval's GAN step of a fleet of cells on the GPU:
``FleetTuner.train_gan`` (one workgroup per cell in ``pgp_gan_forward1_many`` /
``pgp_gan_step1_many``) next to what it replaces, M lone ``train_gan`` graph
pairs (``_GanGraph`` A + B) replayed one after another.

  for M in 1 16 64 256 512; do
    timeout -k 10 180 python tools/fleetgan_time.py --cells $M --append || break
  done
  python tools/fleetgan_time.py --summary            # summary.md from the lines

(one process and one time limit per fleet size; nothing is sized by the
machine's CPU count).  Per M, HIP events around the graph replays alone (inputs
already on the device), `--reps` figures each after a warm-up, median / min /
max:
  envs_ms        one replay of the envs= graph: forward -> pgp_simulate -> step
  ab_ms          graphs A + B of the simulate= mode back to back, no host
                 simulator between them
  lone_ms        M replays of a lone _GanGraph's A + B, back to back on one
                 stream (the same Trainer each time: the launches and their
                 cost do not depend on the weights)
  call_ms        a whole train_gan(simulate=...) call on the host clock with a
                 trivial simulator: staging, two uploads, two replays, two
                 downloads, the per-cell bookkeeping
Writes fleetgan.jsonl (one line per M) and summary.md into --out and prints the
lines.  There is no CPU path.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from preganplus_amd import simulate as SIM  # noqa: E402
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


def measure(H, M, reps):
    base = [W.synth_weights(H, seed=s) for s in range(min(M, 8))]
    ft = TR.FleetTuner(H, [base[m % len(base)] for m in range(M)])
    r = np.random.default_rng(M)
    emb = r.uniform(0.1, 0.9, (M, H, 2)).astype(np.float32)
    scheds = r.uniform(0, 1, (M, H, H))
    envs = SIM.synth_envs(min(M, 16), H, seed=1)[np.arange(M) % min(M, 16)]
    sims = [lambda s: 1.0] * M
    ft.train_gan(emb, scheds, envs=envs)                       # captures the graphs, warms up
    ft.train_gan(emb, scheds, simulate=sims)
    ge, gs = ft.gan_graph(True), ft.gan_graph(False)
    envs_ms = events(ge.graphs["E"].replay, reps)

    def ab():
        gs.graphs["A"].replay()
        gs.graphs["B"].replay()

    ab_ms = events(ab, reps)
    host = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ft.train_gan(emb, scheds, simulate=sims)
        host.append(1e3 * (time.perf_counter() - t0))
    tr = TR.Trainer(H, base[0], max_batch=1)
    TR.train_gan(tr, emb[0], scheds[0], sims[0], fused=True)
    lg = tr._gan_graph

    def lone_all():
        for _ in range(M):
            lg.gA.replay()
            lg.gB.replay()

    lone = events(lone_all, reps)
    e, a, lo = stats(envs_ms), stats(ab_ms), stats(lone)
    return {"hosts": H, "cells": M, "envs_ms": e, "ab_ms": a, "lone_ms": lo, "call_ms": stats(host),
            "ab_us_per_cell": round(1e3 * a["median"] / M, 2), "lone_us_per_cell": round(1e3 * lo["median"] / M, 2),
            "lone_over_ab": round(lo["median"] / a["median"], 2), "lone_over_envs": round(lo["median"] / e["median"], 2),
            "device": torch.cuda.get_device_name(0), "cus": torch.cuda.get_device_properties(0).multi_processor_count}


def summary(out, reps):
    with open(os.path.join(out, "fleetgan.jsonl")) as f:
        rows = [json.loads(x) for x in f if x.strip()]
    with open(os.path.join(out, "summary.md"), "w") as f:
        f.write(f"# FleetTuner.train_gan, H = {rows[0]['hosts']} ({rows[0]['device']}, {rows[0]['cus']} CUs)\n\n")
        f.write("Graph replays between HIP events, median (min-max) of %d, ms; the last column is the host clock.\n\n"
                % reps)
        f.write("| cells | envs= graph | graphs A + B | per cell (us) | M lone A + B | per cell (us) | lone / (A + B) | "
                "lone / envs= | train_gan(simulate=) host |\n")
        f.write("|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            e, a, lo, h = r["envs_ms"], r["ab_ms"], r["lone_ms"], r["call_ms"]
            f.write(f"| {r['cells']} | {e['median']} ({e['min']}-{e['max']}) | {a['median']} ({a['min']}-{a['max']}) | "
                    f"{r['ab_us_per_cell']} | {lo['median']} ({lo['min']}-{lo['max']}) | {r['lone_us_per_cell']} | "
                    f"{r['lone_over_ab']} | {r['lone_over_envs']} | {h['median']} ({h['min']}-{h['max']}) |\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hosts", type=int, default=16)
    ap.add_argument("--cells", default="1,16,64,256,512")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="profiles/r14/fleetgan")
    ap.add_argument("--append", action="store_true", help="add to fleetgan.jsonl instead of starting it anew")
    ap.add_argument("--summary", action="store_true", help="only write summary.md from fleetgan.jsonl")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if not a.summary:
        with open(os.path.join(a.out, "fleetgan.jsonl"), "a" if a.append else "w") as f:
            for M in (int(x) for x in a.cells.split(",")):
                line = json.dumps(measure(a.hosts, M, a.reps))
                print(line, flush=True)
                f.write(line + "\n")
    summary(a.out, a.reps)


if __name__ == "__main__":
    main()
