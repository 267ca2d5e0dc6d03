#!/usr/bin/env python3
"""Times second-order GOBI (pgp_gobi_so_optimize) next to the first-order entry
on the same inits, in the same process.  One process = one batch size = one
JSON record (printed, and written to --out):

    for E in 4 64 1024; do python tools/sogobi_time.py --envs $E --out so_$E.json; done

  so.ms / fo.ms           time per call: device events around the launch, inputs
                          already on the device, the median of --reps after --warmup
  *.iters_max             iterations of the batch's slowest environment (the
                          launch lasts as long as its slowest workgroup's chain)
  *.us_per_iter           ms / (iters_max + 1 final forward ~ iters_max): the time
                          per executed iteration of a workgroup (2 environments
                          second-order, 4 first-order); GOBI's run time depends on
                          how many iterations its inputs take, so the two are
                          compared per iteration
  *.iters_mean            mean iterations per environment
  cpu.s_per_schedule      --cpu N: tests/sogobi_ref.restate (the fp32 restatement,
                          bit-equal to the reference's so_opt) on N of the inits on
                          this machine's CPU, one thread
Inits: the 240 of tests/golden/gobi_h16.npz, repeated to --envs; probes generated
from seeds 0 .. E - 1.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return {"ms": statistics.median(out), "min_ms": min(out), "max_ms": max(out)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cpu", type=int, default=0, help="also time the fp32 CPU restatement on this many inits")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from preganplus_amd import _native
    from preganplus_amd.gobi import GOBIOptimizer

    E = args.envs
    inits = np.load(os.path.join(ROOT, "tests", "golden", "gobi_h16.npz"))["inits"]
    x = torch.tensor(np.resize(inits, (E, 16, 18)), device="cuda")
    seeds = torch.arange(E, dtype=torch.int64, device="cuda")
    g = GOBIOptimizer()
    out = (torch.empty_like(x), torch.empty(E, dtype=torch.int32, device="cuda"),
           torch.empty(E, dtype=torch.float32, device="cuda"))
    L, h, vp = g._L, g._h, lambda t: t.data_ptr()
    st = torch.cuda.current_stream().cuda_stream
    rec = {"lib": os.path.basename(_native.LIB_PATH), "device": torch.cuda.get_device_name(0), "envs": E,
           "warmup": args.warmup, "reps": args.reps}

    def so():
        assert L.pgp_gobi_so_optimize(h, E, vp(x), vp(out[0]), vp(out[1]), vp(out[2]), 0, None, 0, vp(seeds), None,
                                      st) == 0

    def fo():
        assert L.pgp_gobi_optimize(h, E, vp(x), vp(out[0]), vp(out[1]), vp(out[2]), 0, None, st) == 0

    for name, fn, per_wg in (("so", so, 2), ("fo", fo, 4)):
        r = timed(fn, args.warmup, args.reps)
        its = out[1].cpu().numpy()
        r.update(iters_max=int(its.max()), iters_mean=float(its.mean()), envs_per_workgroup=per_wg,
                 us_per_iter=1e3 * r["ms"] / max(int(its.max()), 1), fitness_mean=float(out[2].mean()))
        rec[name] = r
    if args.cpu:
        import sogobi_ref as S
        from oracle import gobi_oracle as GO
        torch.set_num_threads(1)
        f = S.fixture()
        sd, _ = GO.load(S.WEIGHTS)
        t0, steps = time.perf_counter(), 0
        for e in range(args.cpu):
            taps = []
            S.restate(sd, f["inits"][e], S.unpack_signs(f["signs"][e]), torch.float32, taps=taps)
            steps += len(taps)
        dt = time.perf_counter() - t0
        rec["cpu"] = {"schedules": args.cpu, "s_per_schedule": dt / args.cpu, "us_per_iter": 1e6 * dt / steps}
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
