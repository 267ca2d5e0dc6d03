"""Training of GOBI's surrogate on MI355X: the reference's
``python train.py energy_latency_16 train`` (scheduler/BaGTI/train.py:69-94) for
the energy_latency_16 model (scheduler/BaGTI/src/models.py:8-27), whose output
``GOBIOptimizer(weights=...)`` / ``GOBIScheduler(weights=..., max_ips=...)``
consume directly.

The reference treats the surrogate as per-environment (it ships one dataset and
one checkpoint per environment) and trains it by 300 epochs of sequential
batch-1 steps: forward, ``sum((y_pred - y_true)**2)`` (train.py:13-16),
``torch.optim.Adam(lr=1e-4, weight_decay=1e-5)`` (train.py:53: L2 folded into
the gradient, not the decoupled AdamW of ``pgp_adamw``).  Here a whole
``backprop`` pass (train.py:18-31) is ONE launch of ``pgp_gobi_train_steps``
(csrc/pgp_gobitrain.hip) over the dataset uploaded once, and ``accuracy``
(train.py:33-42) one launch of ``pgp_gobi_train_eval``.  All of it is fp32, as
the reference's model and features are.

``GOBIFleetTrainer`` trains M surrogates at once, one workgroup each in one
``pgp_gobi_train_steps_many`` launch (a fleet's cells, or a seed / learning-rate
sweep over one dataset), every model with the bits of a lone ``GOBITrainer``.
"""
from __future__ import annotations

import ctypes
import random

import numpy as np
import torch

from . import _native
from .gobi import _ORDER, H

bind_many = _native.bind   # the earlier helper's name: the previous release's tests reach the library through it
LR, WEIGHT_DECAY, BETAS, EPS = 1e-4, 1e-5, (0.9, 0.999), 1e-8   # train.py:53 (torch.optim.Adam's defaults)
SHAPES = {"find.0.weight": (128, H * (H + 2)), "find.0.bias": (128,), "find.2.weight": (128, 128),
          "find.2.bias": (128,), "find.4.weight": (64, 128), "find.4.bias": (64,), "find.6.weight": (2, 64),
          "find.6.bias": (2,)}


def _read_csv_float(s: str) -> float:
    """A decimal string as ``pd.read_csv``'s default float parser reads it
    (utils.py:59; pandas' documented 'high' precision converter): the first 17
    digits, leading zeros included, accumulated in a double, the rest dropped,
    then one multiplication or division by a power of ten.  It is NOT the
    correctly rounded value for 17-digit strings ("0.20000000000000004" reads as
    0.2), and the reference's dataset is full of those, so float() here would
    give other features than the reference trains on."""
    s = s.strip()
    neg = s.startswith("-")
    if s[:1] in "+-":
        s = s[1:]
    mant, _, exp = s.lower().partition("e")
    whole, _, frac = mant.partition(".")
    if not (whole + frac).isdigit() or (exp and not exp.lstrip("+-").isdigit()):
        return float(("-" if neg else "") + s)   # nan, inf, or not a number: Python's own verdict
    number, digits, exponent = 0.0, 0, 0
    for ch in whole:
        if digits < 17:
            number = number * 10.0 + (ord(ch) - 48)
            digits += 1
        else:
            exponent += 1
    for ch in frac:
        if digits >= 17:
            break
        number = number * 10.0 + (ord(ch) - 48)
        digits += 1
        exponent -= 1
    if exp:
        exponent += int(exp)
    if neg:
        number = -number
    if exponent > 308:
        return float("-inf") if neg else float("inf")
    if exponent > 0:
        return number * float(f"1e{exponent}")
    if exponent < -308:
        return 0.0 if exponent < -616 else number / float(f"1e{-308 - exponent}") / 1e308
    return number / float(f"1e{-exponent}")


def load_energy_latency_data(path, hosts=16):
    """load_energy_latency_data (scheduler/BaGTI/src/utils.py:57-78) of a
    scheduling trace (rows of H host cpu %, H container ips, H container hosts
    (-1: unplaced), energy, latency): (feats [N,H,H+2] float64, targets [N,2]
    float32, max_ips).

    The FIRST LINE IS DROPPED, as the reference drops it: its ``pd.read_csv``
    takes the first data line of the headerless file as the header, so the
    200-line energy_latency_16_scheduling.csv gives 199 samples, and max_ips
    and the targets' min / max are taken over those 199 rows."""
    with open(path) as f:
        lines = [ln for ln in f.read().splitlines() if ln.strip()][1:]
    data = np.array([[_read_csv_float(c) for c in ln.split(",")] for ln in lines], dtype=np.float64)
    if data.ndim != 2 or data.shape[1] != 3 * hosts + 2:
        raise ValueError(f"{path}: {data.shape[1]} columns, expected {3 * hosts + 2} for {hosts} hosts")
    n = data.shape[0]
    max_ips = float(data[:, hosts:2 * hosts].max())
    feats = np.zeros((n, hosts, hosts + 2), dtype=np.float64)
    feats[:, :, 0] = data[:, :hosts] / 100
    feats[:, :, 1] = data[:, hosts:2 * hosts] / max_ips
    host = data[:, 2 * hosts:3 * hosts].astype(np.int64)   # int(): truncation (utils.py:70)
    i, c = np.nonzero(host >= 0)
    feats[i, c, 2 + host[i, c]] = 1
    e, lat = data[:, -2], data[:, -1]
    targets = np.stack([(e - e.min()) / (e.max() - e.min()), np.maximum(0, lat) / lat.max()], axis=1)
    return feats, targets.astype(np.float32), max_ips   # torch.Tensor([...]): fp32 (utils.py:74)


def fresh_weights(seed=None):
    """A new energy_latency_16's parameters: the four nn.Linear of
    models.py:12-20 constructed on the CPU in that order, under
    torch.manual_seed(seed) when a seed is given (the reference's init)."""
    if seed is not None:
        torch.manual_seed(seed)
    out = {}
    for i, (fin, fout) in zip((0, 2, 4, 6), ((H * (H + 2), 128), (128, 128), (128, 64), (64, 2))):
        lin = torch.nn.Linear(fin, fout)
        out[f"find.{i}.weight"] = lin.weight.detach().numpy().copy()
        out[f"find.{i}.bias"] = lin.bias.detach().numpy().copy()
    return out


def checkpoint_dict(P, m, v, step, epoch, accuracy_list, lr=LR, weight_decay=WEIGHT_DECAY, betas=BETAS, eps=EPS):
    """save_model's dict (train.py:44-50) from the parameter / moment blobs
    (state-dict order) after `step` optimizer steps: what the reference's
    load_model (train.py:52-67) and torch.optim.Adam.load_state_dict accept."""
    state, sd, off = {}, {}, 0
    for idx, k in enumerate(_ORDER):
        cnt = int(np.prod(SHAPES[k]))
        sl = slice(off, off + cnt)
        off += cnt
        sd[k] = torch.tensor(np.asarray(P[sl], dtype=np.float32).reshape(SHAPES[k]).copy())
        if step > 0:   # torch keeps no state for a parameter before its first step
            state[idx] = {"step": torch.tensor(float(step)),
                          "exp_avg": torch.tensor(np.asarray(m[sl], dtype=np.float32).reshape(SHAPES[k]).copy()),
                          "exp_avg_sq": torch.tensor(np.asarray(v[sl], dtype=np.float32).reshape(SHAPES[k]).copy())}
    group = {"lr": lr, "betas": tuple(betas), "eps": eps, "weight_decay": weight_decay, "amsgrad": False,
             "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
             "params": list(range(len(_ORDER)))}
    return {"epoch": epoch, "model_state_dict": sd,
            "optimizer_state_dict": {"state": state, "param_groups": [group]},
            "accuracy_list": list(accuracy_list)}


class GOBITrainer:
    """fp32 parameters and Adam moments of the surrogate on the device, as one
    blob in state-dict order (``gobi._ORDER``, pgp_gobi_weight_len(16) floats).

    weights: the ``_ORDER`` dict (None: a fresh model, ``fresh_weights(seed)``);
    state: a checkpoint's ``optimizer_state_dict``."""

    def __init__(self, weights: dict | None = None, state: dict | None = None, device="cuda", seed=None):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("GOBITrainer runs on the GPU only (no CPU fallback)")
        self._L = L = _native.lib()
        if weights is None:
            weights = fresh_weights(seed)
        for k in _ORDER:
            if tuple(np.shape(weights[k])) != SHAPES[k]:
                raise ValueError(f"{k}: shape {tuple(np.shape(weights[k]))}, expected {SHAPES[k]}")
        self.tensors, off = [], 0
        for k in _ORDER:
            cnt = int(np.prod(SHAPES[k]))
            self.tensors.append((k, off, cnt))
            off += cnt
        assert off == L.pgp_gobi_weight_len(H), (off, L.pgp_gobi_weight_len(H))
        blob = np.concatenate([np.asarray(weights[k], dtype=np.float32).reshape(-1) for k in _ORDER])
        m, v = np.zeros_like(blob), np.zeros_like(blob)
        self.step = 0          # one step count: every tensor gets a gradient in every step
        self.lr, self.wd, (self.b1, self.b2), self.eps = LR, WEIGHT_DECAY, BETAS, EPS   # a checkpoint's own below
        if state and state.get("state"):
            steps = set()
            for idx, (k, o, cnt) in enumerate(self.tensors):   # torch's keys: the parameter index
                s = state["state"][idx]
                m[o:o + cnt] = np.asarray(s["exp_avg"], dtype=np.float32).reshape(-1)
                v[o:o + cnt] = np.asarray(s["exp_avg_sq"], dtype=np.float32).reshape(-1)
                steps.add(int(s["step"]))
            if len(steps) != 1:
                raise ValueError(f"optimizer state with different step counts per tensor: {sorted(steps)}")
            self.step = steps.pop()
            g = state["param_groups"][0]
            self.lr, self.wd, self.eps = g["lr"], g["weight_decay"], g["eps"]
            self.b1, self.b2 = g["betas"]
        with torch.cuda.device(self.device):
            self.P = torch.tensor(blob, device=self.device)
            self.m = torch.tensor(m, device=self.device)
            self.v = torch.tensor(v, device=self.device)
        self.feats = self.targets = None
        self.n_samples = 0

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def set_data(self, feats, targets):
        """Upload the dataset once: feats [N,16,18] (rounded to fp32 as
        train.py:22 rounds each sample), targets [N,2]."""
        f = torch.as_tensor(np.asarray(feats), dtype=torch.float32)
        t = torch.as_tensor(np.asarray(targets), dtype=torch.float32)
        if f.dim() != 3 or tuple(f.shape[1:]) != (H, H + 2) or tuple(t.shape) != (f.shape[0], 2):
            raise ValueError(f"feats must be [N,{H},{H + 2}] and targets [N,2], got {tuple(f.shape)}, {tuple(t.shape)}")
        self.feats, self.targets = f.to(self.device).contiguous(), t.to(self.device).contiguous()
        self.n_samples = int(f.shape[0])

    def _order(self, order):
        if self.feats is None:
            raise RuntimeError("no dataset: call set_data(feats, targets) first")
        o = np.asarray(order, dtype=np.int64).reshape(-1)
        if o.size and (o.min() < 0 or o.max() >= self.n_samples):
            raise IndexError(f"sample index outside [0, {self.n_samples})")
        return torch.as_tensor(o.astype(np.int32)).to(self.device)

    def backprop(self, order):
        """train.py:18-31 over the samples order[0..n), in that order: n
        sequential steps in one launch.  Returns the per-sample fp32 losses
        (each before its step's update)."""
        o = self._order(order)
        n = int(o.numel())
        loss = torch.empty(n, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _native.check(self._L.pgp_gobi_train_steps(
                H, self.n_samples, n, self.feats.data_ptr(), self.targets.data_ptr(), o.data_ptr(), self.P.data_ptr(),
                self.m.data_ptr(), self.v.data_ptr(), self.step, self.lr, self.wd, self.b1, self.b2, self.eps,
                loss.data_ptr(), self._stream()), "pgp_gobi_train_steps")
        self.step += n
        return loss.cpu().numpy()

    def accuracy(self, order):
        """train.py:33-42: the per-sample fp32 losses of the samples in order."""
        o = self._order(order)
        n = int(o.numel())
        loss = torch.empty(n, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _native.check(self._L.pgp_gobi_train_eval(
                H, self.n_samples, n, self.feats.data_ptr(), self.targets.data_ptr(), o.data_ptr(), self.P.data_ptr(),
                loss.data_ptr(), self._stream()), "pgp_gobi_train_eval")
        return loss.cpu().numpy()

    @staticmethod
    def _mean(losses):
        """total / len(dataset) of train.py:19-31: the fp32 losses added one by one in fp32."""
        return float(np.cumsum(losses, dtype=np.float32)[-1] / np.float32(len(losses))) if len(losses) else 0.0

    def train(self, feats, targets, epochs, rng=random):
        """The epoch loop of train.py:78-91: every epoch shuffles the dataset
        (``rng.shuffle``; Python's ``random`` as the reference, seed it with
        ``random.seed``), trains on the first 80% and evaluates the rest;
        returns accuracy_list, [(test, train), ...].  The list being shuffled
        persists over the epochs, as the reference's does; the orders it took
        are kept in ``self.orders``."""
        self.set_data(feats, targets)
        idx = list(range(self.n_samples))   # random.shuffle depends on the length alone
        split = int(0.8 * self.n_samples)
        acc = []
        self.orders = []
        for _ in range(epochs):
            rng.shuffle(idx)
            self.orders.append(list(idx))
            train_loss = self._mean(self.backprop(idx[:split]))
            acc.append((self._mean(self.accuracy(idx[split:])), train_loss))
        return acc

    def weights_numpy(self) -> dict:
        p = self.P.detach().cpu().numpy()
        return {k: p[o:o + cnt].reshape(SHAPES[k]).copy() for k, o, cnt in self.tensors}

    def checkpoint(self, epoch, accuracy_list):
        """save_model's dict (train.py:44-50): epoch, model_state_dict,
        optimizer_state_dict (torch.optim.Adam's own layout), accuracy_list."""
        return checkpoint_dict(self.P.cpu().numpy(), self.m.cpu().numpy(), self.v.cpu().numpy(), self.step, epoch,
                               accuracy_list, self.lr, self.wd, (self.b1, self.b2), self.eps)

    def save(self, path, epoch=0, accuracy_list=()):
        """torch.save of checkpoint() (train.py:44-50; the reference names the
        file checkpoints/energy_latency_16_<epoch>.ckpt)."""
        torch.save(self.checkpoint(epoch, accuracy_list), path)


# ---- a fleet of surrogates: M models trained in one launch ----

# pgp_gobi_job of include/preganplus.h (72 bytes, no padding)
JOB_DTYPE = np.dtype([("sample_off", "<i8"), ("order_off", "<i8"), ("step0", "<i8"), ("n_samples", "<i4"),
                      ("n", "<i4"), ("lr", "<f8"), ("weight_decay", "<f8"), ("beta1", "<f8"), ("beta2", "<f8"),
                      ("eps", "<f8")])
_HYPER_KEYS = ("lr", "weight_decay", "beta1", "beta2", "eps")


def _blob_of(weights):
    for k in _ORDER:
        if tuple(np.shape(weights[k])) != SHAPES[k]:
            raise ValueError(f"{k}: shape {tuple(np.shape(weights[k]))}, expected {SHAPES[k]}")
    return np.concatenate([np.asarray(weights[k], dtype=np.float32).reshape(-1) for k in _ORDER])


def fleet_state(weights=None, seeds=None, states=None, hyper=None):
    """The host side of GOBIFleetTrainer's construction (no device needed):
    (P, m, v [M, 61890] float32, steps [M], hypers: M dicts of lr /
    weight_decay / beta1 / beta2 / eps).  Exactly one of weights (a list of
    ``_ORDER`` dicts) and seeds (``fresh_weights(seed)`` each); states: None or
    one ``optimizer_state_dict`` (or None) per model; hyper: None, one dict for
    all, or one per model (over a checkpoint's own values)."""
    if (weights is None) == (seeds is None):
        raise ValueError("pass weights=[...] or seeds=[...], one of them")
    ws = [fresh_weights(s) for s in seeds] if weights is None else list(weights)
    M = len(ws)
    if M == 0:
        raise ValueError("an empty fleet")
    if states is None:
        states = [None] * M
    if len(states) != M:
        raise ValueError(f"{len(states)} optimizer states for {M} models")
    if hyper is None or isinstance(hyper, dict):
        hyper = [hyper] * M
    if len(hyper) != M:
        raise ValueError(f"{len(hyper)} hyper-parameter sets for {M} models")
    P = np.stack([_blob_of(w) for w in ws])
    m, v = np.zeros_like(P), np.zeros_like(P)
    steps, hypers = [0] * M, []
    for i in range(M):
        hy = {"lr": LR, "weight_decay": WEIGHT_DECAY, "beta1": BETAS[0], "beta2": BETAS[1], "eps": EPS}
        st = states[i]
        if st and st.get("state"):
            seen, off = set(), 0
            for idx, k in enumerate(_ORDER):
                cnt = int(np.prod(SHAPES[k]))
                s = st["state"][idx]
                m[i, off:off + cnt] = np.asarray(s["exp_avg"], dtype=np.float32).reshape(-1)
                v[i, off:off + cnt] = np.asarray(s["exp_avg_sq"], dtype=np.float32).reshape(-1)
                seen.add(int(s["step"]))
                off += cnt
            if len(seen) != 1:
                raise ValueError(f"model {i}: optimizer state with different step counts per tensor: {sorted(seen)}")
            steps[i] = seen.pop()
            g = st["param_groups"][0]
            hy.update(lr=g["lr"], weight_decay=g["weight_decay"], eps=g["eps"], beta1=g["betas"][0],
                      beta2=g["betas"][1])
        if hyper[i]:
            unknown = set(hyper[i]) - set(_HYPER_KEYS)
            if unknown:
                raise ValueError(f"unknown hyper-parameters {sorted(unknown)}; known: {_HYPER_KEYS}")
            hy.update(hyper[i])
        hypers.append(hy)
    return P, m, v, steps, hypers


def pool_datasets(datasets, dataset_of, n_models):
    """One sample pool from a list of (feats [N,16,18], targets [N,2]):
    (feats fp32 [Ntot,16,18], targets fp32 [Ntot,2], offsets, sizes,
    dataset_of [n_models]).  dataset_of None: model m trains on dataset m, or
    every model on the only one."""
    datasets = list(datasets)
    if not datasets:
        raise ValueError("no dataset")
    fs, ts = [], []
    for i, (f, t) in enumerate(datasets):
        f, t = np.asarray(f, dtype=np.float32), np.asarray(t, dtype=np.float32)
        if f.ndim != 3 or f.shape[1:] != (H, H + 2) or t.shape != (f.shape[0], 2):
            raise ValueError(f"dataset {i}: feats must be [N,{H},{H + 2}] and targets [N,2], got {f.shape}, {t.shape}")
        fs.append(f)
        ts.append(t)
    if dataset_of is None:
        if len(datasets) == 1:
            dataset_of = [0] * n_models
        elif len(datasets) == n_models:
            dataset_of = list(range(n_models))
        else:
            raise ValueError(f"{len(datasets)} datasets for {n_models} models: say which with dataset_of")
    dataset_of = [int(d) for d in dataset_of]
    if len(dataset_of) != n_models:
        raise ValueError(f"dataset_of has {len(dataset_of)} entries for {n_models} models")
    if any(d < 0 or d >= len(datasets) for d in dataset_of):
        raise ValueError(f"dataset_of has an index outside [0, {len(datasets)})")
    sizes = [int(f.shape[0]) for f in fs]
    offsets = [int(x) for x in np.concatenate([[0], np.cumsum(sizes)[:-1]])]
    return np.concatenate(fs), np.concatenate(ts), offsets, sizes, dataset_of


def fleet_jobs(orders, sample_off, n_samples, steps, hypers):
    """The job table (JOB_DTYPE [M]) and the order pool (int32) of one call:
    model m's order list, relative to its own dataset, goes to the pool at
    order_off = the lengths before it.  IndexError for an index outside the
    model's dataset (as GOBITrainer), ValueError for another number of lists."""
    M = len(steps)
    if len(orders) != M:
        raise ValueError(f"{len(orders)} order lists for {M} models")
    jobs = np.zeros(M, dtype=JOB_DTYPE)
    pool, off = [], 0
    for i in range(M):
        o = np.asarray(orders[i], dtype=np.int64).reshape(-1)
        if o.size and (o.min() < 0 or o.max() >= n_samples[i]):
            raise IndexError(f"model {i}: sample index outside [0, {n_samples[i]})")
        jobs[i] = (sample_off[i], off, steps[i], n_samples[i], o.size) + tuple(hypers[i][k] for k in _HYPER_KEYS)
        pool.append(o.astype(np.int32))
        off += o.size
    return jobs, (np.concatenate(pool) if pool else np.zeros(0, np.int32))


class GOBIFleetTrainer:
    """M surrogates on the device, one slot each of P / m / v [M, 61890], trained
    by ``pgp_gobi_train_steps_many``: one workgroup per model, every model's
    bits those of a lone ``GOBITrainer`` with its settings.  The reference keeps
    a surrogate per environment (one dataset and checkpoint per data_type,
    scheduler/BaGTI/); the same entry serves a seed / learning-rate sweep over
    one dataset.  See ``fleet_state`` for the arguments."""

    def __init__(self, weights=None, seeds=None, states=None, hyper=None, device="cuda"):
        P, m, v, self.steps, self.hypers = fleet_state(weights, seeds, states, hyper)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("GOBIFleetTrainer runs on the GPU only (no CPU fallback)")
        self._L = _native.lib()
        self.n_models = int(P.shape[0])
        assert P.shape[1] == self._L.pgp_gobi_weight_len(H)
        with torch.cuda.device(self.device):
            self.P = torch.tensor(P, device=self.device)
            self.m = torch.tensor(m, device=self.device)
            self.v = torch.tensor(v, device=self.device)
            self._jobs_dev = torch.empty(self.n_models * JOB_DTYPE.itemsize, dtype=torch.uint8, device=self.device)
        self.feats = self.targets = None

    def set_data(self, datasets, dataset_of=None):
        """Upload the datasets once as one pool; models may share entries."""
        f, t, self._off, self._size, self.dataset_of = pool_datasets(datasets, dataset_of, self.n_models)
        self.feats = torch.as_tensor(f).to(self.device).contiguous()
        self.targets = torch.as_tensor(t).to(self.device).contiguous()

    def n_samples(self, m):
        return self._size[self.dataset_of[m]]

    def _launch(self, orders, train):
        if self.feats is None:
            raise RuntimeError("no dataset: call set_data(datasets) first")
        M = self.n_models
        jobs, pool = fleet_jobs(orders, [self._off[self.dataset_of[i]] for i in range(M)],
                                [self.n_samples(i) for i in range(M)], self.steps, self.hypers)
        order = torch.as_tensor(pool).to(self.device)
        loss = torch.empty(int(pool.size), dtype=torch.float32, device=self.device)
        vp = ctypes.c_void_p
        st = vp(torch.cuda.current_stream(self.device).cuda_stream)
        with torch.cuda.device(self.device):
            if train:
                _native.check(self._L.pgp_gobi_train_steps_many(
                    H, M, jobs.ctypes.data_as(vp), int(self.feats.shape[0]), self.feats.data_ptr(),
                    self.targets.data_ptr(), int(pool.size), order.data_ptr(), self.P.data_ptr(), self.m.data_ptr(),
                    self.v.data_ptr(), loss.data_ptr(), self._jobs_dev.data_ptr(), st), "pgp_gobi_train_steps_many")
            else:
                _native.check(self._L.pgp_gobi_train_eval_many(
                    H, M, jobs.ctypes.data_as(vp), int(self.feats.shape[0]), self.feats.data_ptr(),
                    self.targets.data_ptr(), int(pool.size), order.data_ptr(), self.P.data_ptr(), loss.data_ptr(),
                    self._jobs_dev.data_ptr(), st), "pgp_gobi_train_eval_many")
        out = loss.cpu().numpy()   # also the point up to which `jobs` (read by the stream's copy) must live
        return [out[int(j["order_off"]):int(j["order_off"]) + int(j["n"])].copy() for j in jobs], jobs

    def backprop(self, orders):
        """train.py:18-31 for every model over its own order list (relative to
        its own dataset; an empty list leaves the model untouched), all in one
        launch.  Returns the per-sample fp32 losses, one array per model."""
        losses, jobs = self._launch(orders, True)
        for i in range(self.n_models):
            self.steps[i] += int(jobs[i]["n"])
        return losses

    def accuracy(self, orders):
        """train.py:33-42 for every model: the per-sample losses of its list."""
        return self._launch(orders, False)[0]

    def train(self, epochs, rngs):
        """The epoch loop of train.py:78-91 per model (set_data first): model m
        has its own ``random.Random`` rngs[m], its own persistent shuffled list
        and its own 80/20 split; each epoch is one training launch and one
        evaluation launch for the whole fleet.  Returns the accuracy lists,
        [[(test, train), ...] per model]; the orders taken are in
        ``self.orders[m]``."""
        M = self.n_models
        if len(rngs) != M:
            raise ValueError(f"{len(rngs)} random generators for {M} models")
        if self.feats is None:
            raise RuntimeError("no dataset: call set_data(datasets) first")
        idx = [list(range(self.n_samples(i))) for i in range(M)]
        split = [int(0.8 * self.n_samples(i)) for i in range(M)]
        acc = [[] for _ in range(M)]
        self.orders = [[] for _ in range(M)]
        for _ in range(epochs):
            for i in range(M):
                rngs[i].shuffle(idx[i])
                self.orders[i].append(list(idx[i]))
            tr = self.backprop([idx[i][:split[i]] for i in range(M)])
            te = self.accuracy([idx[i][split[i]:] for i in range(M)])
            for i in range(M):
                acc[i].append((GOBITrainer._mean(te[i]), GOBITrainer._mean(tr[i])))
        return acc

    def _tensors(self):
        out, off = [], 0
        for k in _ORDER:
            cnt = int(np.prod(SHAPES[k]))
            out.append((k, off, cnt))
            off += cnt
        return out

    def weights_numpy(self, m) -> dict:
        p = self.P[m].detach().cpu().numpy()
        return {k: p[o:o + cnt].reshape(SHAPES[k]).copy() for k, o, cnt in self._tensors()}

    def checkpoint(self, m, epoch, accuracy_list):
        """save_model's dict (train.py:44-50) of model m."""
        hy = self.hypers[m]
        return checkpoint_dict(self.P[m].cpu().numpy(), self.m[m].cpu().numpy(), self.v[m].cpu().numpy(),
                               self.steps[m], epoch, accuracy_list, hy["lr"], hy["weight_decay"],
                               (hy["beta1"], hy["beta2"]), hy["eps"])

    def save(self, m, path, epoch=0, accuracy_list=()):
        torch.save(self.checkpoint(m, epoch, accuracy_list), path)

    def trainer(self, m) -> GOBITrainer:
        """An ordinary GOBITrainer holding copies of model m's parameters,
        moments, step count, hyper-parameters and (if set) dataset: it goes on
        as a checkpoint of model m would."""
        t = GOBITrainer(weights=self.weights_numpy(m), device=self.device)
        t.m, t.v, t.step = self.m[m].clone(), self.v[m].clone(), self.steps[m]
        hy = self.hypers[m]
        t.lr, t.wd, t.b1, t.b2, t.eps = hy["lr"], hy["weight_decay"], hy["beta1"], hy["beta2"], hy["eps"]
        if self.feats is not None:
            o, n = self._off[self.dataset_of[m]], self.n_samples(m)
            t.feats, t.targets, t.n_samples = self.feats[o:o + n].clone(), self.targets[o:o + n].clone(), n
        return t
