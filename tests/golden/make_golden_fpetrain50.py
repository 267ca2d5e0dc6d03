"""Golden fixture for PreGAN's offline FPE training at 50 hosts (build container only).

Run from a scratch directory:  python <repo>/tests/golden/make_golden_fpetrain50.py

The 50-host counterpart of make_golden_fpetrain.py.  The reference's FPE_50
class cannot run (dlutils.py:306), so the model is the one C4 already uses:
the reference's host-count-generic FPE_16 class with its constants set for 50
hosts (make_golden_fpe50.build_fpe, an extrapolation of FPE_16 and NOT the
reference's FPE_50).  Everything else is the reference's own code: AdamW as
load_model builds it (utils.py:65: lr = model.lr, weight decay 1e-5),
normalize_time_data / convert_to_windows / form_test_dataset (utils.py:7-24,
91-92, i.e. load_dataset without its npy read), train.backprop and
train.accuracy (train.py:42-57, 94-109).

Model: build_fpe(50).double() loaded with
preganplus_amd.weights.synth_fpe_weights(50, seed=0) and its prototypes.  They
are fp32-representable, so the fixture stores the seed and a checksum
(weights.fpe_weights_checksum) in place of the initial weights.

Data: a synthetic 50-host [cpu, ram, disk] series of 24 rows in the style of
make_golden_train50.synth_series, with three idle rows (IDLE_ROWS, 0 - 0.04 of
the column scale): an idle row is never above a column's 98th percentile, so
its window has no positive label and its step leaves the prototype decoder
without a gradient.

Recorded: two epochs of backprop + accuracy with every GRU state the forwards
draw (torch.randn inside encode, models.py:70, recorded by wrapping
torch.randn), under the keys of the 16-host fixture; and three single steps
from the initial weights at num_zero, num_ones = 7, 3 and factor 0.2 (a window
with many positives, an idle window, one other window): the gradient of every
parameter, (aloss, tloss) and the state after the step.  encoder.0.weight
(79,500 values) is stored through tests/golden/digest.py wherever it occurs.

Three files, each below 1 MiB:
  tests/golden/fpe_train_h50.npz        data, GRU states, per-epoch scalars,
                                        prototypes, parameters and step counts
  tests/golden/fpe_train_h50_opt.npz    AdamW moments after each epoch
                                        (exp_avg_sq of encoder.0.weight is left
                                        out: nothing reads it and its digest
                                        would take the file past the limit)
  tests/golden/fpe_train_h50_steps.npz  the three single steps

Before writing, the script replays the two epochs with the oracle's restatement
in fp32 (oracle.pregan_train_oracle, CPU) against the fp64 record and asserts
that fp32 arithmetic alone keeps every tensor within the device test's cap
(fewer than 1 % of a tensor's entries out of 1e-4 |want| + 1e-5 max|want|).
It prints the reference's mean time per backprop step on this machine.
"""
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)

import make_golden_fpe50 as MF  # noqa: E402  (imports the reference through refshim)
from digest import FULL, digest  # noqa: E402
from preganplus_amd import weights as W  # noqa: E402

models, utils, train = MF.models, MF.utils, MF.train

H = 50
N_WIN = 24
EPOCHS = 2
SEED = 0
DATA_SEED = 5024
IDLE_ROWS = (5, 6, 17)
STEP_COUNTERS = (7, 3)      # num_zero, num_ones of the single steps
STEP_FACTOR = 0.2


def synth_series(rng, T):
    """make_golden_train50.synth_series at T rows, with IDLE_ROWS idle."""
    scale = rng.uniform(20, 100, size=3 * H)
    x = rng.uniform(0.05, 0.6, size=(T, 3 * H)) * scale
    spike = rng.uniform(size=x.shape) < 0.03
    x = np.where(spike, rng.uniform(0.8, 1.0, size=x.shape) * scale, x)
    for r in IDLE_ROWS:
        x[r] = rng.uniform(0.0, 0.04, size=3 * H) * scale
    return x


def new_model(w):
    f = MF.build_fpe(H).double()
    f.load_state_dict(MF.to_sd(w["fpe"]))
    f.prototype = [torch.tensor(p) for p in np.asarray(w["prototypes"], dtype=np.float64)]
    return f, torch.optim.AdamW(f.parameters(), lr=f.lr, weight_decay=1e-5)      # utils.py:65


def put(rec, name, a, key):
    """A tensor under its plain key, or through digest.py when it is large."""
    a = np.asarray(a, dtype=np.float64)
    if a.size <= FULL:
        rec[name] = a.copy()
    else:
        rec.update(digest(name, a, key=key))


def fp32_alone_within_cap(w, rec, wins, anom, cls):
    """The oracle's loop in fp32 against the fp64 record: the share of entries
    per tensor outside the device test's tolerance, from fp32 rounding alone."""
    from digest import sample_index
    from oracle import pregan_train_oracle as TO
    fw = TO.leaf_params(w["fpe"], skip=(), dtype=torch.float32)
    opt = TO.AdamW(fw, 1e-4)
    st = TO.TuneState(w["prototypes"], 0.2)
    worst = 0.0
    for ep in range(EPOCHS):
        TO.fpe_backprop(fw, opt, st, wins.astype(np.float32), rec[f"ep{ep}/h0_backprop"].astype(np.float32), anom, cls)
        for k, q in fw.items():
            got = q.detach().numpy().astype(np.float64).reshape(-1)
            if f"ep{ep}/p/{k}" in rec:
                want = rec[f"ep{ep}/p/{k}"].reshape(-1)
            else:
                want = rec[f"ep{ep}/p/{k}/sample"]
                got = got[sample_index(k, got.size)]
            noise = np.zeros(want.size, dtype=bool)
            if k == "mha.in_proj_bias":
                E = want.size // 3
                noise[E:2 * E] = True
            tol = 1e-4 * np.abs(want) + 1e-5 * np.abs(want).max()
            bad = ((np.abs(got - want) > tol) & ~noise).mean()
            worst = max(worst, bad)
            assert bad < 0.01, (ep, k, bad)
    print(f"fp32 oracle vs fp64 record: worst share of entries out of tolerance {worst:.4%} (cap 1 %)")


def main():
    w = W.synth_fpe_weights(H, seed=SEED)
    f, opt = new_model(w)
    assert sum(p.numel() for p in f.parameters()) == 93137
    rng = np.random.Generator(np.random.PCG64(DATA_SEED))
    series = synth_series(rng, N_WIN)
    time_data = utils.normalize_time_data(series)                              # utils.py:34
    wins = utils.convert_to_windows(time_data, f)                              # utils.py:36
    anom, cls = utils.form_test_dataset(time_data)                             # utils.py:37
    sched = torch.zeros((N_WIN, H, H), dtype=torch.double)                     # the FPE's forward does not read it
    npos = anom.sum(1)
    assert (npos == 0).sum() >= 2 and (npos > 0).sum() >= 15, npos
    assert set(np.unique(cls[anom > 0])) == {0, 1, 2}
    assert all(npos[r] == 0 for r in IDLE_ROWS)
    rec = {"series": series, "wins": wins.numpy(), "anom": np.asarray(anom, dtype=np.int64),
           "cls": np.asarray(cls, dtype=np.int64), "weights_seed": np.int32(SEED), "n_hosts": np.int32(H),
           "weights_checksum": np.float64(W.fpe_weights_checksum(w)),
           "model_note": np.array("reference FPE_16 class instantiated at n_hosts=50 "
                                  "(extrapolation; the reference FPE_50 raises at dlutils.py:306)")}
    ropt = {}
    draws = []
    randn = torch.randn

    def recording_randn(*a, **k):
        t = randn(*a, **k)
        draws.append(t.detach().numpy().reshape(-1).copy())
        return t

    torch.randn = recording_randn
    torch.manual_seed(11)
    train.PROTO_UPDATE_FACTOR = 0.2   # the module global starts at PROTO_UPDATE_FACTOR (train.py:1)
    spent = 0.0
    try:
        for ep in range(EPOCHS):
            n0 = len(draws)
            t0 = time.perf_counter()
            loss, factor = train.backprop(ep, f, wins, sched, anom, cls, opt)
            spent += time.perf_counter() - t0
            n1 = len(draws)
            asc, csc = train.accuracy(f, wins, sched, anom, cls, None)
            n2 = len(draws)
            assert n1 - n0 == N_WIN and n2 - n1 == N_WIN, (n0, n1, n2)
            rec[f"ep{ep}/h0_backprop"] = np.stack(draws[n0:n1])
            rec[f"ep{ep}/h0_accuracy"] = np.stack(draws[n1:n2])
            rec[f"ep{ep}/loss"] = np.float64(loss)
            rec[f"ep{ep}/factor"] = np.float64(factor)
            rec[f"ep{ep}/ascore"] = np.float64(asc)
            rec[f"ep{ep}/cscore"] = np.float64(csc)
            rec[f"ep{ep}/num_zero"] = np.float64(train.num_zero)
            rec[f"ep{ep}/num_ones"] = np.float64(train.num_ones)
            rec[f"ep{ep}/proto_factor"] = np.float64(train.PROTO_UPDATE_FACTOR)
            rec[f"ep{ep}/prototypes"] = np.stack([p.detach().numpy() for p in f.prototype])
            for k, v in f.state_dict().items():
                put(rec, f"ep{ep}/p/{k}", v.detach().numpy(), k)
            for k, q in f.named_parameters():
                st = opt.state[q]
                put(ropt, f"ep{ep}/m/{k}", st["exp_avg"].numpy(), k)
                if q.numel() <= FULL:
                    ropt[f"ep{ep}/v/{k}"] = st["exp_avg_sq"].numpy().copy()
                rec[f"ep{ep}/step/{k}"] = np.float64(float(st["step"]))
            print(f"epoch {ep}: loss {loss:.6f} factor {factor:.6f} AScore {asc:.4f} CScore {csc:.4f}")
        print(f"reference backprop: {spent / (EPOCHS * N_WIN) * 1e6:.0f} us per step "
              f"(mean of {EPOCHS * N_WIN} steps, {torch.get_num_threads()} threads)")

        # three single steps from the initial weights
        many = int(np.argmax(npos))
        idle = IDLE_ROWS[0]
        other = int(np.argmin(np.where(npos > 0, npos, 10 ** 6)))
        assert len({many, idle, other}) == 3
        rsteps = {"index": np.array([many, idle, other], dtype=np.int64),
                  "num_zero": np.float64(STEP_COUNTERS[0]), "num_ones": np.float64(STEP_COUNTERS[1]),
                  "factor": np.float64(STEP_FACTOR)}
        torch.manual_seed(21)
        for j, i in enumerate((many, idle, other)):
            g, _ = new_model(w)
            train.PROTO_UPDATE_FACTOR = STEP_FACTOR
            train.num_zero, train.num_ones = STEP_COUNTERS
            n0 = len(draws)
            out = g(wins[i], sched[i])
            assert len(draws) == n0 + 1
            aloss, tloss = train.custom_loss(g, out, anom[i], cls[i])
            (aloss + tloss).backward()
            rsteps[f"s{j}/h0"] = draws[n0]
            rsteps[f"s{j}/loss"] = np.array([float(aloss), float(tloss)])
            rsteps[f"s{j}/prototypes"] = np.stack([p.detach().numpy() for p in g.prototype])
            rsteps[f"s{j}/state"] = np.array([train.PROTO_UPDATE_FACTOR, train.num_zero, train.num_ones],
                                             dtype=np.float64)
            for k, q in g.named_parameters():
                rsteps[f"s{j}/has_grad/{k}"] = np.bool_(q.grad is not None)
                put(rsteps, f"s{j}/g/{k}", q.grad.numpy() if q.grad is not None else np.zeros(q.shape), k)
            print(f"step {j}: window {i}, {int(npos[i])} positive hosts, aloss {float(aloss):.6f} "
                  f"tloss {float(tloss):.6f}")
    finally:
        torch.randn = randn
    fp32_alone_within_cap(w, rec, wins.numpy(), np.asarray(anom), np.asarray(cls))
    for name, d in (("fpe_train_h50.npz", rec), ("fpe_train_h50_opt.npz", ropt), ("fpe_train_h50_steps.npz", rsteps)):
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **d)
        size = os.path.getsize(path)
        print(name, size, "bytes")
        assert size < 1 << 20, (name, size)


if __name__ == "__main__":
    main()
