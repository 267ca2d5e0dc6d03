#!/usr/bin/env python3
"""Times the fleet entries of GOBI's surrogate against the single-model ones,
and fingerprints the single-model entries so that two builds can be compared.

One process = one record (a JSON line, also written to --out).  Select the
library with PGP_LIB; a library without the fleet entries (an older build)
gives the single-model part alone, so alternating processes on two libraries
give an A/B of the entries both have:

    PGP_LIB=old.so python tools/gobi_fleet_time.py --out a1.json
    python tools/gobi_fleet_time.py --out b1.json
    PGP_LIB=old.so python tools/gobi_fleet_time.py --out a2.json ...

  single.train_us_per_step   pgp_gobi_train_steps, 159 steps in one launch
  single.optimize_ms         pgp_gobi_optimize, 1,024 environments
  single.*_sha256            the bits of one 159-step sequence (P, m, v, losses)
                             and of one GOBI batch (result, iterations, fitness)
  many.train_us_per_step[M]  pgp_gobi_train_steps_many, 159 steps, M = 1 .. 512
                             (every model on the same dataset, its own seed)
  many.optimize_groups_ms[M] pgp_gobi_optimize_groups, 1,024 environments spread
                             round-robin over M = 1, 4, 64 surrogates
Times are device events around the launch, the median of --reps after --warmup.
"""
import argparse
import hashlib
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden")
STEPS, ENVS = 159, 1024


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
    return {"median_ms": statistics.median(out), "min_ms": min(out), "max_ms": max(out)}


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--models", type=int, nargs="*", default=[1, 16, 64, 256, 512])
    ap.add_argument("--opt-models", type=int, nargs="*", default=[1, 4, 64])
    args = ap.parse_args()

    import ctypes

    from preganplus_amd import _native
    from preganplus_amd import gobitrain as GT
    from preganplus_amd.gobi import GOBIOptimizer, load_weights

    L = _native.lib()
    rec = {"lib": os.path.basename(_native.LIB_PATH), "device": torch.cuda.get_device_name(0), "steps": STEPS,
           "envs": ENVS, "warmup": args.warmup, "reps": args.reps}
    feats, targets, _ = GT.load_energy_latency_data(os.path.join(GOLD, "energy_latency_16_scheduling.csv"))
    order = np.random.RandomState(7).permutation(feats.shape[0])[:STEPS].tolist()
    inits = np.load(os.path.join(GOLD, "gobi_h16.npz"))["inits"].astype(np.float32)
    x = torch.tensor(np.concatenate([inits] * (ENVS // inits.shape[0] + 1))[:ENVS], device="cuda")

    # ---- the single-model entries: the bits, then the times ----
    t = GT.GOBITrainer(seed=16)
    t.set_data(feats, targets)
    loss = t.backprop(order)
    single = {"train_sha256": sha(t.P.cpu().numpy(), t.m.cpu().numpy(), t.v.cpu().numpy(), loss)}
    o = t._order(order)
    lossbuf = torch.empty(STEPS, dtype=torch.float32, device="cuda")

    def one_launch():   # the entry alone: no upload, no read-back (the state keeps moving; the time does not)
        _native.check(L.pgp_gobi_train_steps(16, t.n_samples, STEPS, t.feats.data_ptr(), t.targets.data_ptr(),
                                             o.data_ptr(), t.P.data_ptr(), t.m.data_ptr(), t.v.data_ptr(), t.step,
                                             t.lr, t.wd, t.b1, t.b2, t.eps, lossbuf.data_ptr(), t._stream()), "steps")
    r = timed(one_launch, args.warmup, args.reps)
    single["train_us_per_step"] = {k.replace("_ms", ""): v * 1e3 / STEPS for k, v in r.items()}
    opt = GOBIOptimizer(weights=load_weights()[0])
    res, its, fit = opt.optimize(x)
    single["optimize_sha256"] = sha(res.cpu().numpy(), its.cpu().numpy(), fit.cpu().numpy())
    out = (torch.empty_like(x), torch.empty(ENVS, dtype=torch.int32, device="cuda"),
           torch.empty(ENVS, dtype=torch.float32, device="cuda"))
    single["optimize_ms"] = timed(lambda: opt.optimize(x, out=out), args.warmup, args.reps)
    rec["single"] = single

    # ---- the fleet entries, where the library has them ----
    if hasattr(L, "pgp_gobi_train_steps_many"):
        many = {"train_us_per_step": {}, "optimize_groups_ms": {}}
        vp = ctypes.c_void_p
        for M in args.models:
            f = GT.GOBIFleetTrainer(seeds=list(range(16, 16 + min(M, 8))) * (M // min(M, 8)))
            assert f.n_models == M, (M, f.n_models)
            f.set_data([(feats, targets)])
            jobs, pool = GT.fleet_jobs([order] * M, [0] * M, [feats.shape[0]] * M, f.steps, f.hypers)
            od = torch.as_tensor(pool).cuda()
            ls = torch.empty(pool.size, dtype=torch.float32, device="cuda")

            def launch():
                _native.check(f._L.pgp_gobi_train_steps_many(
                    16, M, jobs.ctypes.data_as(vp), int(f.feats.shape[0]), f.feats.data_ptr(), f.targets.data_ptr(),
                    int(pool.size), od.data_ptr(), f.P.data_ptr(), f.m.data_ptr(), f.v.data_ptr(), ls.data_ptr(),
                    f._jobs_dev.data_ptr(), vp(torch.cuda.current_stream().cuda_stream)), "steps_many")
            r = timed(launch, args.warmup, args.reps)
            many["train_us_per_step"][str(M)] = {k.replace("_ms", ""): v * 1e3 / STEPS for k, v in r.items()}
            assert not torch.isnan(ls).any()
            del f, od, ls
        w0 = load_weights()[0]
        for M in args.opt_models:
            ws = [w0] + [GT.fresh_weights(100 + m) for m in range(1, M)]
            og = GOBIOptimizer(weights=ws)
            model_of = np.arange(ENVS) % M
            og.optimize(x, out=out, model_of=model_of)   # plans the table once
            many["optimize_groups_ms"][str(M)] = timed(lambda: og.optimize(x, out=out, model_of=model_of),
                                                       args.warmup, args.reps)
            if M == 1:
                many["optimize_groups_m1_sha256"] = sha(*(a.cpu().numpy() for a in out))
            og.close()
        rec["many"] = many
    line = json.dumps(rec, sort_keys=True)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
