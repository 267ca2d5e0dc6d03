"""Golden fixtures for the training of GOBI's surrogate (energy_latency_16):
the reference's own loader, model, loss and training loop, run here.

  scheduler/BaGTI/src/utils.py:57-78   load_energy_latency_data (pd.read_csv takes the first data
                                       line as the header: 199 samples of the 200-line file)
  scheduler/BaGTI/src/models.py:8-27   energy_latency_16 (returns the 2-vector when training)
  scheduler/BaGTI/train.py:13-42       custom_loss, backprop, accuracy
  scheduler/BaGTI/train.py:53, 81-91   Adam(lr 1e-4, weight_decay 1e-5); the epoch loop

Imports /root/reference/scheduler/BaGTI read-only (run with python -B from any
directory); only names the installed libraries no longer have are shimmed
(np.float, matplotlib's 'science' / 'ieee' styles), no reference code is changed.
Writes, each below the committed-file limit,
  tests/golden/gobitrain_h16.npz            dataset, initial weights, orders, losses, bounds, two epochs
  tests/golden/gobitrain_h16_f32_n{1,8,64}.npz   the reference's fp32 backprop after n steps: p, m, v blobs
  tests/golden/gobitrain_h16_f64_n{1,8,64}.npz   the same steps in fp64
The fp64 run takes the fp32 run's inputs (features and targets rounded to fp32,
train.py:22) so that the two differ by arithmetic alone.  To fit the size limit
its state is stored in fp32: the parameters as the move p_n - p_0 (at most n lr,
so the rounding is under 4e-10), the moments directly (2^-25 relative: at most
half of the fp32 run's own deviation, which after one step is rounding
alone); the script checks both.
bounds[kind][n][tensor] = max |fp32 run - stored fp64 run|: what 8x of is the
GPU tests' per-tensor bound (tests/test_gpu_gobitrain.py).
"""
import os
import random
import sys

import numpy as np
import torch

REF = "/root/reference"
BAGTI = os.path.join(REF, "scheduler", "BaGTI")
OUT = os.path.dirname(os.path.abspath(__file__))
H = 16
ORDER = ("find.0.weight", "find.0.bias", "find.2.weight", "find.2.bias", "find.4.weight", "find.4.bias",
         "find.6.weight", "find.6.bias")
INIT_SEED, ORDER_SEED, EPOCH_SEED = 16, 7, 1
STEPS = (1, 8, 64)


def import_reference():
    sys.dont_write_bytecode = True
    os.environ.setdefault("MPLBACKEND", "Agg")
    import matplotlib
    import matplotlib.style
    for name in ("science", "ieee"):  # utils.py:12 (scienceplots is not installed; plotting is out of scope)
        matplotlib.style.library.setdefault(name, matplotlib.RcParams())
    if not hasattr(np, "float"):
        np.float = float  # utils.py:60 (removed from numpy 1.24)
    sys.path.insert(0, BAGTI)
    sys.argv[:] = ["make_golden_gobitrain", "-", "-"]  # utils.py:16 makes a checkpoint folder for 'train' in argv[0]
    os.chdir(REF)  # utils.py:59 reads scheduler/BaGTI/datasets/... relative to the working directory
    import src.models as models
    import src.utils as utils
    import train
    sys.argv[:] = ["train.py", "energy_latency_16", "train"]  # models.py:25: the training output is the 2-vector
    return models, utils, train


def blob(tensors):
    return np.concatenate([np.asarray(t, dtype=np.float64).reshape(-1) for t in tensors])


def state(model, opt):
    ps = list(model.parameters())
    return (blob(p.detach().numpy() for p in ps), blob(opt.state[p]["exp_avg"].numpy() for p in ps),
            blob(opt.state[p]["exp_avg_sq"].numpy() for p in ps))


def fresh(models):
    torch.manual_seed(INIT_SEED)
    return models.energy_latency_16()


def adam(model):
    return torch.optim.Adam(model.parameters(), lr=0.0001, weight_decay=1e-5)  # train.py:53


def main():
    models, utils, train = import_reference()
    dataset, size, max_ips = utils.load_energy_latency_data(H)
    assert size == 199, size
    feats = np.stack([d[0] for d in dataset]).astype(np.float64)
    targets = np.stack([d[1].numpy() for d in dataset]).astype(np.float32)
    out = {"feats": feats, "targets": targets, "max_ips": np.float64(max_ips), "init_seed": INIT_SEED,
           "epoch_seed": EPOCH_SEED}

    model = fresh(models)
    w0 = {k: v.detach().numpy().copy() for k, v in model.state_dict().items()}
    assert tuple(w0) == ORDER
    p0 = blob(w0[k] for k in ORDER)
    for k in ORDER:
        out["w0/" + k] = w0[k]

    order = random.Random(ORDER_SEED).sample(range(size), max(STEPS))
    unplaced = [i for i in range(size) if (feats[i][:, 2:].sum(1) == 0).any()]
    full = [i for i in range(size) if (feats[i][:, 2:].sum(1) == 1).all()]
    out["order"] = np.array(order, dtype=np.int32)
    out["sample_unplaced"], out["sample_full"] = np.int32(unplaced[0]), np.int32(full[0])

    # the reference's own fp32 backprop, one sample at a time to record the per-sample loss
    opt = adam(model)
    loss32, snap32 = [], {}
    for i, s in enumerate(order):
        loss32.append(float(train.backprop([dataset[s]], model, opt).data))
        if i + 1 in STEPS:
            snap32[i + 1] = state(model, opt)
    out["loss_f32"] = np.array(loss32, dtype=np.float32)

    # the same steps in fp64 (train.py:18-31 with the dtype changed; the fp32 run's inputs)
    m64 = fresh(models).double()
    opt64 = adam(m64)
    loss64, snap64 = [], {}
    for i, s in enumerate(order):
        x = torch.tensor(dataset[s][0], dtype=torch.float).double()
        y = dataset[s][1].double()
        opt64.zero_grad()
        loss = train.custom_loss(m64(x), y, m64.name)
        loss.backward()
        opt64.step()
        loss64.append(float(loss.data))
        if i + 1 in STEPS:
            snap64[i + 1] = state(m64, opt64)
    out["loss_f64"] = np.array(loss64, dtype=np.float64)

    sizes = [int(np.prod(w0[k].shape)) for k in ORDER]
    offs = np.concatenate([[0], np.cumsum(sizes)])
    for n in STEPS:
        p32, m32, v32 = snap32[n]
        p64, m64b, v64 = snap64[n]
        dp = (p64 - p0).astype(np.float32)
        st = {"p": p0 + dp.astype(np.float64), "m": m64b.astype(np.float32).astype(np.float64),
              "v": v64.astype(np.float32).astype(np.float64)}
        np.savez_compressed(os.path.join(OUT, f"gobitrain_h16_f64_n{n}.npz"), dp=dp, m=m64b.astype(np.float32),
                            v=v64.astype(np.float32))
        np.savez_compressed(os.path.join(OUT, f"gobitrain_h16_f32_n{n}.npz"), p=p32.astype(np.float32),
                            m=m32.astype(np.float32), v=v32.astype(np.float32))
        for kind, a32, a64 in (("p", p32, p64), ("m", m32, m64b), ("v", v32, v64)):
            dev = np.array([np.abs(a32 - st[kind])[offs[j]:offs[j + 1]].max() for j in range(len(ORDER))])
            rnd = np.array([np.abs(a64 - st[kind])[offs[j]:offs[j + 1]].max() for j in range(len(ORDER))])
            # the storage rounding against the deviation the bound is 8x of (the bound is measured
            # against the STORED values, so the two are consistent in any case)
            assert np.all(rnd <= dev / (16 if kind == "p" else 2)), (kind, n, rnd, dev)
            out[f"bound/{kind}/n{n}"] = dev
            move = np.array([np.abs(a64 - (p0 if kind == "p" else 0))[offs[j]:offs[j + 1]].max()
                             for j in range(len(ORDER))])
            out[f"move/{kind}/n{n}"] = move
            print(f"n={n:2d} {kind}: fp32-vs-fp64 max dev per tensor", " ".join(f"{d:.2e}" for d in dev))
            print(f"          8x bound / max move              ", " ".join(f"{8 * d / mv:.1e}" for d, mv in zip(dev, move)))

    # two whole epochs (train.py:81-91) from the same initial model
    model = fresh(models)
    opt = adam(model)
    random.seed(EPOCH_SEED)
    idx = list(range(size))  # random.shuffle depends on the length alone: the dataset's own permutation
    split = int(0.8 * size)
    orders, acc = [], []
    for _ in range(2):
        random.shuffle(idx)
        ds = [dataset[i] for i in idx]
        loss = train.backprop(ds[:split], model, opt)
        acc.append((float(train.accuracy(ds[split:], model).data), float(loss.data)))
        orders.append(list(idx))
    out["epoch_orders"] = np.array(orders, dtype=np.int32)
    out["accuracy_list"] = np.array(acc, dtype=np.float64)
    print("split", split, size - split, "accuracy_list", acc)
    np.savez_compressed(os.path.join(OUT, "gobitrain_h16.npz"), **out)
    for f in sorted(os.listdir(OUT)):
        if f.startswith("gobitrain_h16"):
            sz = os.path.getsize(os.path.join(OUT, f))
            assert sz < 1 << 20, (f, sz)
            print(f, sz)


if __name__ == "__main__":
    main()
