#!/usr/bin/env python3
"""Time the end of a fleet's interval on the GPU: the tuning
call with the scores computed per cell on the host (``tune(score=True)``) and
inside the graph (``score="device"``, ``pgp_tune_scores_many``), and the
plugin's decision stage as a per-cell ``_recover`` loop and as one batched K5
call (``PreGANPlusFleetRecovery(device_finish=True)``).

  python tools/fleetfinish_time.py [--hosts 16] [--n 10] [--cells 1,16,64,256,512] [--reps 7]
                                   [--out profiles/r15/fleetfinish]

One child process per fleet size.  Per size, `--reps` figures each after a
warm-up, median / min / max, in ms:
  graph_ms[mode]    one replay of the tuning graph between HIP events (inputs
                    already on the device)
  span_ms[mode]     upload + replay + download between HIP events, as
                    tune_launch enqueues them
  call_ms[mode]     the whole FleetTuner.tune() call on the host clock
  download_bytes[mode]
  decide_loop_ms    the decision stage as run_model's default runs it: per
                    deciding cell one _recover (upload, K5 at batch 1,
                    download, synchronisation), on the host clock
  decide_batch_ms   the same decisions through _recover_many: one upload, one
                    K5 launch at batch M, one download, one synchronisation
The decision stage runs on a stand-in holding the fields it reads (random
placements, every cell deciding: the costliest case for both forms).
Writes fleetfinish.jsonl (one line per size) and summary.md into --out and
prints the lines.  There is no CPU path.
"""
import argparse
import json
import os
import subprocess
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MODES = (("host", True), ("device", "device"))


def stats(ms):
    s = sorted(ms)
    return {"median": round(s[len(s) // 2], 4), "min": round(s[0], 4), "max": round(s[-1], 4)}


class _Container:
    def __init__(self, cid, host):
        self.id, self._h = cid, host

    def getHostID(self):
        return self._h


def measure(H, n, M, reps):
    import numpy as np
    import torch

    from preganplus_amd import recovery as R
    from preganplus_amd import train as TR
    from preganplus_amd import weights as W

    def events(fn):
        out = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            out.append(a.elapsed_time(b))
        return out

    def clock(fn):
        out = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            out.append(1e3 * (time.perf_counter() - t0))
        return out

    r = np.random.default_rng(M)
    base = [W.synth_weights(H, seed=s) for s in range(min(M, 8))]
    wins = r.uniform(0, 1, (M, n, 3, 3 * H)).astype(np.float32)
    anom = (r.uniform(size=(M, n, H)) < 0.25).astype(np.int32)
    anom[:, 0, 1] = 1
    cls = r.integers(0, 3, (M, n, H)).astype(np.int32)
    row = {"hosts": H, "n": n, "cells": M, "graph_ms": {}, "span_ms": {}, "call_ms": {}, "download_bytes": {}}
    for name, mode in MODES:
        ft = TR.FleetTuner(H, [base[m % len(base)] for m in range(M)])
        ft.tune(wins, anom, cls, score=mode)                   # captures the graph, warms up
        g = ft.graph(n, mode)

        def span():
            g.din.copy_(g.hin, non_blocking=True)
            g.graph.replay()
            g.hout.copy_(g.down, non_blocking=True)

        span()
        row["graph_ms"][name] = stats(events(g.graph.replay))
        row["span_ms"][name] = stats(events(span))
        row["call_ms"][name] = stats(clock(lambda: ft.tune(wins, anom, cls, score=mode)))
        row["download_bytes"][name] = g.hout.numel() * g.hout.element_size()
        del ft, g
    # the decision stage
    device = torch.device("cuda", torch.cuda.current_device())
    envs = [types.SimpleNamespace(containerlist=[
        None if u < 0.1 else _Container(c, -1 if u < 0.25 else int(r.integers(0, H)))
        for c, u in enumerate(r.uniform(size=H))]) for _ in range(M)]
    originals = [[(int(c), int(r.integers(0, H))) for c in r.permutation(H)[:3]] for _ in range(M)]
    final_target = r.integers(0, H, (M, H)).astype(np.int32)
    probs = np.tile(np.array([0.2, 0.8], dtype=np.float32), (M, 1))
    cells = list(range(M))
    rio = R._RecoverIO(H, device)

    def loop():
        res = list(originals)
        for m in cells:                                        # run_model's default decision stage
            p = probs[m]
            res[m], _ = R._recover(envs[m], H, None, originals[m], bool(p[0] > p[1]), device,
                                   final_target[m].tolist(), io=rio)
        return res

    fleet = types.SimpleNamespace(M=M, hosts=H, device=device, _rio_many=None, envs=envs,
                                  tuner=types.SimpleNamespace(gan_probs_after=probs), hosts_from=[None] * M)

    def batch():
        res = list(originals)
        R.PreGANPlusFleetRecovery._recover_many(fleet, cells, res, originals, final_target)
        return res

    assert loop() == batch()
    row["decide_loop_ms"] = stats(clock(loop))
    row["decide_batch_ms"] = stats(clock(batch))
    row["decide_loop_us_per_cell"] = round(1e3 * row["decide_loop_ms"]["median"] / M, 2)
    row["device"] = torch.cuda.get_device_name(0)
    row["cus"] = torch.cuda.get_device_properties(0).multi_processor_count
    return row


def fmt(s):
    return f"{s['median']} ({s['min']}-{s['max']})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hosts", type=int, default=16)
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--cells", default="1,16,64,256,512")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="profiles/r15/fleetfinish")
    ap.add_argument("--one", type=int, default=0, help="measure this fleet size in this process, print its line")
    a = ap.parse_args()
    if a.one:
        print("ROW " + json.dumps(measure(a.hosts, a.n, a.one, a.reps)), flush=True)
        return
    os.makedirs(a.out, exist_ok=True)
    rows = []
    with open(os.path.join(a.out, "fleetfinish.jsonl"), "w") as f:
        for M in (int(x) for x in a.cells.split(",")):       # one fresh process per size, one at a time
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--hosts", str(a.hosts), "--n", str(a.n),
                                  "--reps", str(a.reps), "--one", str(M)], check=True, stdout=subprocess.PIPE, text=True,
                                 cwd=ROOT).stdout
            line = next(ln for ln in out.splitlines() if ln.startswith("ROW "))[4:]
            rows.append(json.loads(line))
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
    with open(os.path.join(a.out, "summary.md"), "w") as f:
        f.write(f"# The end of a fleet's interval, H = {a.hosts}, n = {a.n} ({rows[0]['device']}, {rows[0]['cus']} CUs)\n\n")
        f.write(f"Median (min-max) of {a.reps}, ms; one process per size.  host = tune(score=True), "
                "device = tune(score=\"device\").\n\n")
        f.write("| cells | graph host | graph device | up+graph+down host | up+graph+down device | download bytes host / device "
                "| tune() host | tune() device | decisions: per-cell loop | per cell (us) | decisions: one call |\n")
        f.write("|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write(f"| {r['cells']} | {fmt(r['graph_ms']['host'])} | {fmt(r['graph_ms']['device'])} | "
                    f"{fmt(r['span_ms']['host'])} | {fmt(r['span_ms']['device'])} | "
                    f"{r['download_bytes']['host']} / {r['download_bytes']['device']} | "
                    f"{fmt(r['call_ms']['host'])} | {fmt(r['call_ms']['device'])} | {fmt(r['decide_loop_ms'])} | "
                    f"{r['decide_loop_us_per_cell']} | {fmt(r['decide_batch_ms'])} |\n")


if __name__ == "__main__":
    main()
