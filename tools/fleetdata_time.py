#!/usr/bin/env python3
"""Time a fleet's tuning datasets on the GPU: built per cell on
the host (``_input_window`` + ``on_the_fly_dataset`` + stacking, as
``PreGANPlusFleetRecovery.run_model`` does by default) against staged and built
by one ``FleetTuner.dataset`` call (``pgp_tune_dataset_cells``,
``device_dataset=True``).

  python tools/fleetdata_time.py [--hosts 16] [--n 10] [--cells 1,16,64,256,512] [--reps 7]
                                 [--series-rows 200] [--out profiles/r16/fleetdata]

One child process per fleet size.  Per size, `--reps` figures each after a
warm-up, median / min / max, in ms:
  data_host_ms      the dataset stage of the default run_model on the host
                    clock: per cell _input_window (normalises the cell's whole
                    series of --series-rows rows) and on_the_fly_dataset, then
                    the copy of every cell's windows and labels into [M,n,...]
                    arrays
  data_device_ms    the same stage with device_dataset: per cell the copy of its
                    last n rows into the pinned staging, one dataset() call
                    (upload, launch and the labels' download enqueued, nothing
                    waited for)
  data_device_sync_ms  ... and a stream synchronisation behind it (in run_model
                    that wait is the detect download's)
  kernel_ms         pgp_tune_dataset_cells alone between HIP events
  upload_bytes      what one tune_launch uploads with inputs="host" and
                    inputs="device", and dataset()'s own upload (series | active)
  run_model_ms      the whole plugin call on stand-in environments (every cell
                    anomalous, constant simulator scores), both flags off and
                    both on
Writes fleetdata.jsonl (one line per size) and summary.md into --out and prints
the lines.  There is no CPU path.
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


def stats(ms):
    s = sorted(ms)
    return {"median": round(s[len(s) // 2], 4), "min": round(s[0], 4), "max": round(s[-1], 4)}


class _Container:
    def __init__(self, cid, host):
        self.id, self._h = cid, host

    def getHostID(self):
        return self._h


def measure(H, n, M, reps, rows):
    import numpy as np
    import torch

    from preganplus_amd import _native
    from preganplus_amd import train as TR
    from preganplus_amd import weights as W
    from preganplus_amd.recovery import PreGANPlusFleetRecovery

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
    scale = r.uniform(10, 100, size=3 * H)
    trains = [r.uniform(0.1, 1.0, size=(40, 3 * H)) * scale * (1 + m % 7) for m in range(M)]
    series = [r.uniform(0.05, 1.2, size=(rows, 3 * H)) * scale * (1 + m % 7) for m in range(M)]

    def forced(w):          # every host anomalous whatever the window: every cell tunes, the costliest interval
        t = dict(w["transformer"])
        t["anomaly_decoder.0.weight"] = np.zeros_like(np.asarray(t["anomaly_decoder.0.weight"]))
        bias = np.zeros(2 * H)
        bias[1::2] = 2.0
        t["anomaly_decoder.0.bias"] = bias
        return dict(w, transformer=t)

    base = [forced(W.synth_weights(H, seed=s)) for s in range(min(M, 8))]
    weights = [base[m % len(base)] for m in range(M)]
    extras = [{"train_time_data": t} for t in trains]
    sched = r.uniform(0, 1, (rows, H, H))

    def envs():
        out = []
        for m in range(M):
            stats_ = types.SimpleNamespace(time_series=series[m], schedule_series=sched,
                                           runSimulation=lambda s: (1.0, 1.0))
            out.append(types.SimpleNamespace(
                stats=stats_, scheduler=types.SimpleNamespace(result_cache=sched[-1]),
                containerlist=[_Container(c, int(r.integers(0, H))) for c in range(H)]))
        return out

    row = {"hosts": H, "n": n, "cells": M, "series_rows": rows}
    host = PreGANPlusFleetRecovery(H, weights, extras, training=True)
    devp = PreGANPlusFleetRecovery(H, weights, extras, training=True, device_finish=True, device_dataset=True)
    host.setEnvironments(envs())
    devp.setEnvironments(envs())
    decisions = [[] for _ in range(M)]

    # the dataset stage alone, as each run_model runs it
    def data_host():
        wins = np.stack([host._input_window(m) for m in range(M)])
        data = {m: TR.on_the_fly_dataset(host.envs[m].stats.time_series, host.envs[m].stats.schedule_series,
                                         host.train_time_data[m]) for m in range(M)}
        k = np.asarray(data[0][0]).shape[0]
        w = np.zeros((M, k, 3, 3 * H), dtype=np.float32)
        y = np.zeros((M, k, H), dtype=np.int32)
        c = np.zeros((M, k, H), dtype=np.int32)
        for m in range(M):
            w[m], y[m], c[m] = data[m][0], np.asarray(data[m][2]).reshape(k, H), np.asarray(data[m][3]).reshape(k, H)
        return wins, w, y, c

    def data_device():
        return devp._device_datasets("device")

    def data_device_sync():
        devp._device_datasets("device")
        torch.cuda.current_stream().synchronize()

    wins_h, w_h, y_h, c_h = data_host()
    d = data_device()[n]
    torch.cuda.synchronize()
    g = devp.tuner.graph(n, "device")
    assert g.W.cpu().numpy().tobytes() == w_h.tobytes() and d.y.tobytes() == y_h.tobytes()   # the same dataset
    assert devp.tuner.infer_windows.cpu().numpy().tobytes() == wins_h.astype(np.float32).tobytes()
    row["data_host_ms"] = stats(clock(data_host))
    row["data_device_ms"] = stats(clock(data_device))
    row["data_device_sync_ms"] = stats(clock(data_device_sync))
    row["data_host_us_per_cell"] = round(1e3 * row["data_host_ms"]["median"] / M, 2)
    row["data_device_us_per_cell"] = round(1e3 * row["data_device_ms"]["median"] / M, 2)

    ft, L = devp.tuner, _native.lib()

    def kernel():
        _native.check(L.pgp_tune_dataset_cells(
            H, M, n, d.d_active.data_ptr(), d.d_series.data_ptr(), ft._train_max.data_ptr(), g.W.data_ptr(),
            g.Y.data_ptr(), g.C.data_ptr(), d.d_positive.data_ptr(), ft.infer_windows.data_ptr(), ft._stream()),
            "pgp_tune_dataset_cells")

    kernel()
    row["kernel_ms"] = stats(events(kernel))
    total = g.din.numel()
    row["upload_bytes"] = {"tune_host": total, "tune_device": total - g.span["sched"][0], "dataset": d.upload_bytes}

    # the whole plugin call
    for p in (host, devp):
        p.run_model(decisions)
        p.run_model(decisions)
    row["run_model_ms"] = {"default": stats(clock(lambda: host.run_model(decisions))),
                           "device": stats(clock(lambda: devp.run_model(decisions)))}
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
    ap.add_argument("--series-rows", type=int, default=200, help="rows of each cell's stats.time_series (>= n)")
    ap.add_argument("--out", default="profiles/r16/fleetdata")
    ap.add_argument("--one", type=int, default=0, help="measure this fleet size in this process, print its line")
    a = ap.parse_args()
    if a.series_rows < a.n or not 1 <= a.n <= 10:
        ap.error("1 <= n <= 10 (LATEST_WINDOW_SIZE) and --series-rows >= n")
    if a.one:
        print("ROW " + json.dumps(measure(a.hosts, a.n, a.one, a.reps, a.series_rows)), flush=True)
        return
    os.makedirs(a.out, exist_ok=True)
    rows = []
    with open(os.path.join(a.out, "fleetdata.jsonl"), "w") as f:
        for M in (int(x) for x in a.cells.split(",")):       # one fresh process per size, one at a time
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--hosts", str(a.hosts), "--n", str(a.n),
                                  "--reps", str(a.reps), "--series-rows", str(a.series_rows), "--one", str(M)],
                                 check=True, stdout=subprocess.PIPE, text=True, cwd=ROOT).stdout
            line = next(ln for ln in out.splitlines() if ln.startswith("ROW "))[4:]
            rows.append(json.loads(line))
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
    with open(os.path.join(a.out, "summary.md"), "w") as f:
        f.write(f"# A fleet's tuning datasets, H = {a.hosts}, n = {a.n}, series of {a.series_rows} rows "
                f"({rows[0]['device']}, {rows[0]['cus']} CUs)\n\n")
        f.write(f"Median (min-max) of {a.reps}, ms; one process per size.  host = per-cell numpy, "
                "device = staging + one dataset() call.\n\n")
        f.write("| cells | dataset host | per cell (us) | dataset device (enqueue) | per cell (us) | ... + sync | kernel "
                "| upload bytes: tune host / tune device / dataset | run_model default | run_model both flags |\n")
        f.write("|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            u = r["upload_bytes"]
            f.write(f"| {r['cells']} | {fmt(r['data_host_ms'])} | {r['data_host_us_per_cell']} | "
                    f"{fmt(r['data_device_ms'])} | {r['data_device_us_per_cell']} | {fmt(r['data_device_sync_ms'])} | "
                    f"{fmt(r['kernel_ms'])} | {u['tune_host']} / {u['tune_device']} / {u['dataset']} | "
                    f"{fmt(r['run_model_ms']['default'])} | {fmt(r['run_model_ms']['device'])} |\n")


if __name__ == "__main__":
    main()
