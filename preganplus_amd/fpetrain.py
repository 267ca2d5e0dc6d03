"""Offline training of PreGAN's FPE encoder on MI355X, at 16 or 50 hosts
(FPE_16, and FPE_16's architecture with its constants set for 50 hosts: the
reference's own FPE_50 class cannot run) (PreGAN.py:26-27,
39-49): with no FPE checkpoint the reference creates a new FPE_16 and trains it
for num_epochs (train.py:42-57 backprop + :94-109 accuracy over utils.py:36-42
load_dataset's series, AdamW lr 1e-4 weight decay 1e-5, models.py:14), saving
the checkpoint after every epoch; the encoder is then frozen.  The reference's
framework environment ships no FPE checkpoint, so this is the path it takes
there.

Every step runs on the device: ``pgp_fpe_train_step`` (forward, custom_loss /
triplet_loss bookkeeping on the device state in fp64, full backward, one
workgroup; csrc/pgp_fpetrain.hip) then ``pgp_adamw`` with torch's semantics.
The GRU state the reference draws inside every forward (torch.randn,
models.py:70) is drawn here by the same call in the same order (backprop's N,
then accuracy's N per epoch), so a seeded run reproduces the reference's.

``FPETrainer.backprop(one_launch=True)`` runs a whole pass in one launch
(``pgp_fpe_train_steps``: the AdamW inside the kernel, driven by
``adam_table``'s rows), and ``FPEFleetTrainer`` / ``train_fleet`` train M FPEs
at once, one workgroup per model (``pgp_fpe_train_steps_many``,
``pgp_fpe_forward_many_cells``; csrc/pgp_fpetrain_cells.hip): the
reference keeps one FPE per PreGANRecovery, so a fleet of cells trains one per
cell.  Every model keeps the bits of a lone run."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _native, adamw
from . import weights as W
from .train import PROTO_FACTOR_DECAY, PROTO_UPDATE_MIN, TuneState, accuracy_scores

FPE_LR = 1e-4          # FPE_16.lr (models.py:14)
SUPPORTED_H = (16, 50)  # the host counts pgp_fpetrain.hip is compiled for
COND = adamw.COND_TENSORS   # no gradient without a positive label


def adam_table(tensors, positive, lr, b1, b2):
    """The AdamW rows of consecutive steps, float32 [len(positive), len(tensors),
    3] = (active, step_size, bc2_sqrt) (``adamw.schedule``), and the tensors'
    step counts advanced: a tensor of COND takes no step on a window without a
    positive label (torch skips a parameter without a gradient)."""
    table, steps = adamw.schedule([t["step"] for t in tensors], adamw.stepping([t["name"] for t in tensors], positive),
                                  lr, b1, b2)
    for t, st in zip(tensors, steps.tolist()):
        t["step"] = st
    return table


def adam_rows(tensors, positive: bool, lr, b1, b2):
    """One torch.optim.AdamW.step's per-tensor scalars [(active, step_size,
    bc2_sqrt)] in the tensors' order — ``adam_table``'s row of that one step,
    as ``FPETrainer.adam_step`` puts it in its descriptors."""
    return [(int(a), float(s), float(b)) for a, s, b in adam_table(tensors, [positive], lr, b1, b2)[0]]


def fpe_blob(fpe: dict, H: int = 16) -> torch.Tensor:
    """The natural fp32 parameter blob of an FPE weight dict, in state_dict order
    (weights.fpe_shapes(H); pgp_fpe_param_len(H) floats), on the host: what
    ``FPETrainer.P`` holds and ``pgp_fpe_forward1`` reads."""
    blob = np.concatenate([np.asarray(fpe[k], dtype=np.float64).reshape(-1) for k in W.fpe_shapes(H)])
    return torch.tensor(blob, dtype=torch.float32)


class FPETrainer:
    """fp32 master weights, gradients and AdamW moments of the H-host FPE on the
    device, in state_dict order (weights.fpe_shapes(H)); H in SUPPORTED_H."""

    def __init__(self, fpe: dict, device="cuda", state: dict | None = None, weight_decay=1e-5,
                 betas=(0.9, 0.999), eps=1e-8, H=16):
        self.H = H
        self.device = torch.device(device)
        self._L = L = _native.lib()
        n = int(L.pgp_fpe_param_len(H))
        if n == 0:
            raise ValueError(f"FPE training: H={H} not supported (supported host counts: "
                             f"{', '.join(map(str, SUPPORTED_H))})")
        shapes = W.fpe_shapes(H)
        self.tensors, off = [], 0
        for name, shp in shapes.items():
            cnt = int(np.prod(shp))
            self.tensors.append({"name": name, "shape": shp, "offset": off, "n": cnt, "step": 0.0})
            off += cnt
        assert off == n, (off, n)
        f32 = torch.float32
        self.P = fpe_blob(fpe, H).to(self.device)
        self.G = torch.zeros_like(self.P)
        self.m = torch.zeros_like(self.P)
        self.v = torch.zeros_like(self.P)
        if state:   # AdamW state per parameter INDEX: a checkpoint's optimizer_state_dict["state"]
            m, v = self.m.cpu().numpy(), self.v.cpu().numpy()   # (torch's keys, as checkpoint() writes them)
            for idx, t in enumerate(self.tensors):
                s = state.get(idx)
                if s:
                    m[t["offset"]:t["offset"] + t["n"]] = np.asarray(s["exp_avg"]).reshape(-1)
                    v[t["offset"]:t["offset"] + t["n"]] = np.asarray(s["exp_avg_sq"]).reshape(-1)
                    t["step"] = float(s["step"])
            self.m.copy_(torch.tensor(m))
            self.v.copy_(torch.tensor(v))
        self.lr, self.wd, self.b1, self.b2, self.eps = FPE_LR, weight_decay, betas[0], betas[1], eps
        self.loss = torch.zeros(2, dtype=torch.float64, device=self.device)

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def adam_step(self, positive: bool):
        """torch.optim.AdamW.step (utils.py:65); the prototype decoder had no
        gradient when the window has no positive label (torch skips it)."""
        desc = adamw.descriptors(self.tensors, adam_rows(self.tensors, positive, self.lr, self.b1, self.b2))
        _native.check(self._L.pgp_adamw_d(
            ctypes.c_void_p(self.P.data_ptr()), ctypes.c_void_p(self.G.data_ptr()),
            ctypes.c_void_p(self.m.data_ptr()), ctypes.c_void_p(self.v.data_ptr()),
            self.lr, self.wd, self.b1, self.b2, self.eps, desc, len(desc), self._stream()), "pgp_adamw_d")

    def adam_table(self, positive):
        """The rows n consecutive ``adam_step(positive[i])`` calls put in their
        descriptors, float32 [n,16,3] = (active, step_size, bc2_sqrt): the same
        Python doubles rounded to fp32 once (pgp_fpe_train_steps's ``sched``).
        Advances the tensors' step counts as those calls do."""
        return adam_table(self.tensors, positive, self.lr, self.b1, self.b2)

    def _desc(self):
        """The tensors' places in the blob (offset, n): what a table-driven update reads of a descriptor."""
        return adamw.descriptors(self.tensors)

    def backprop(self, st: TuneState, wins, h0s, anom, cls, one_launch=False):
        """train.py:42-57 over the windows: one device step per window (forward,
        bookkeeping, backward) and its AdamW; the state (prototypes, factor,
        counters) lives on the device for the whole pass and is read back once.
        Returns the per-window (aloss, tloss).  ``one_launch``: the whole pass
        in one launch of ``pgp_fpe_train_steps`` (the AdamW rows uploaded once
        as a table) instead of two launches per window; the same bits."""
        st.num_zero, st.num_ones = 1, 1
        n, H, dev = len(wins), self.H, self.device
        anom = np.asarray(anom).reshape(n, H)
        cls = np.asarray(cls).reshape(n, H)
        w = torch.as_tensor(np.asarray(wins), dtype=torch.float32).to(dev).contiguous()
        h = torch.as_tensor(np.asarray(h0s), dtype=torch.float32).reshape(n, 3).to(dev).contiguous()
        y = torch.as_tensor(anom, dtype=torch.int32).to(dev).contiguous()
        c = torch.as_tensor(np.clip(cls, 0, 2), dtype=torch.int32).to(dev).contiguous()
        state = torch.tensor(st.vector(), dtype=torch.float64, device=dev)
        K = st.protos.shape[0]
        losses = torch.zeros((n, 2), dtype=torch.float64, device=dev)
        positive = np.any(anom > 0, axis=1)
        if one_launch:
            sched = torch.from_numpy(self.adam_table(positive)).to(dev)
            _native.check(self._L.pgp_fpe_train_steps(
                H, K, n, w.data_ptr(), h.data_ptr(), y.data_ptr(), c.data_ptr(), self.P.data_ptr(),
                self.G.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), state.data_ptr(), PROTO_UPDATE_MIN,
                PROTO_FACTOR_DECAY, self.lr, self.wd, self.b1, self.b2, self.eps, self._desc(), len(self.tensors),
                sched.data_ptr(), losses.data_ptr(), self._stream()), "pgp_fpe_train_steps")
        for i in range(0 if one_launch else n):
            _native.check(self._L.pgp_fpe_train_step(
                H, K, w[i].data_ptr(), h[i].data_ptr(), y[i].data_ptr(), c[i].data_ptr(), self.P.data_ptr(),
                self.G.data_ptr(), state.data_ptr(), PROTO_UPDATE_MIN, PROTO_FACTOR_DECAY, losses[i].data_ptr(),
                self._stream()), "pgp_fpe_train_step")
            self.adam_step(bool(positive[i]))
        st.from_vector(state.cpu().numpy())
        return [tuple(r) for r in losses.cpu().numpy().tolist()]

    def forward_many(self, wins, h0s):
        """n independent forwards (accuracy(), train.py:94-109): probs, protos [n,H,2] fp64."""
        n, H, dev = len(wins), self.H, self.device
        w = torch.as_tensor(np.asarray(wins), dtype=torch.float32).to(dev).contiguous()
        h = torch.as_tensor(np.asarray(h0s), dtype=torch.float32).reshape(n, 3).to(dev).contiguous()
        out = torch.zeros((2, n, H, 2), dtype=torch.float64, device=dev)
        _native.check(self._L.pgp_fpe_forward_many(H, n, w.data_ptr(), h.data_ptr(), self.P.data_ptr(),
                                                    out[0].data_ptr(), out[1].data_ptr(), self._stream()),
                      "pgp_fpe_forward_many")
        o = out.cpu().numpy()
        return o[0], o[1]

    def accuracy(self, st: TuneState, wins, h0s, anom, cls):
        """train.py:94-109 on the FPE (its probabilities are what the reference
        takes the argmax of): (AScore, CScore)."""
        probs, protos = self.forward_many(wins, h0s)
        return accuracy_scores(probs, protos, anom, cls, st.protos)

    def weights_numpy(self) -> dict:
        p = self.P.detach().cpu().numpy().astype(np.float64)
        return {t["name"]: p[t["offset"]:t["offset"] + t["n"]].reshape(t["shape"]) for t in self.tensors}

    def checkpoint(self, epoch, accuracy_list, prototypes):
        """save_model's dict (utils.py:49-58) for the FPE: weights, prototypes,
        AdamW state per parameter index, epoch, accuracy_list."""
        w = self.weights_numpy()
        m, v = self.m.cpu().numpy(), self.v.cpu().numpy()
        state = {}
        for idx, t in enumerate(self.tensors):
            sl = slice(t["offset"], t["offset"] + t["n"])
            if t["step"] > 0:
                state[idx] = {"step": torch.tensor(float(t["step"])),
                              "exp_avg": torch.tensor(m[sl].astype(np.float64).reshape(t["shape"])),
                              "exp_avg_sq": torch.tensor(v[sl].astype(np.float64).reshape(t["shape"]))}
        return {"epoch": epoch,
                "model_state_dict": {k: torch.tensor(a) for k, a in w.items()},
                "model_prototypes": [torch.tensor(np.asarray(p, dtype=np.float64)) for p in prototypes],
                "optimizer_state_dict": {"state": state, "param_groups": [{
                    "lr": self.lr, "betas": (self.b1, self.b2), "eps": self.eps, "weight_decay": self.wd,
                    "amsgrad": False, "params": list(range(len(self.tensors)))}]},
                "accuracy_list": list(accuracy_list)}


def draw_h0(n, generator=None):
    """The GRU states n consecutive FPE forwards draw (models.py:70:
    torch.randn(1, 1, 3, dtype=torch.double) on the CPU generator), [n,3]."""
    return np.stack([torch.randn(1, 1, 3, dtype=torch.double, generator=generator).numpy().reshape(3)
                     for _ in range(n)])


# ---- a fleet of FPEs: M models trained in one launch ----

# pgp_fpe_job of include/preganplus.h (24 bytes, no padding)
JOB_DTYPE = np.dtype([("window_off", "<i8"), ("step_off", "<i8"), ("n", "<i4"), ("reserved", "<i4")])


class FPEFleetTrainer:
    """M FPEs of one host count, each a slot of P / G / m / v [M, len] on the
    device with its own AdamW step counts: the reference keeps one FPE per
    PreGANRecovery (PreGAN.py:26-27), so a fleet of cells, a seed sweep over one
    series or a set of newly deployed sites trains M of them.  ``backprop`` runs
    every model's pass in ONE launch (pgp_fpe_train_steps_many: one workgroup per
    model), ``forward_many`` every model's forwards in one
    (pgp_fpe_forward_many_cells); model m has the bits a lone ``FPETrainer`` has."""

    def __init__(self, fpes, H=16, device="cuda", states=None, weight_decay=1e-5, betas=(0.9, 0.999), eps=1e-8):
        self.H, self.M = H, len(fpes)
        self.device = torch.device(device)
        self._L = L = _native.lib()
        self.len = int(L.pgp_fpe_param_len(H))
        if self.len == 0:
            raise ValueError(f"FPE training: H={H} not supported (supported host counts: "
                             f"{', '.join(map(str, SUPPORTED_H))})")
        self._kw = dict(weight_decay=weight_decay, betas=betas, eps=eps, H=H)
        self.lr, self.wd, self.b1, self.b2, self.eps = FPE_LR, weight_decay, betas[0], betas[1], eps
        f32 = torch.float32
        self.P = torch.zeros((self.M, self.len), dtype=f32, device=self.device)
        self.G, self.m, self.v = torch.zeros_like(self.P), torch.zeros_like(self.P), torch.zeros_like(self.P)
        self.tensors = []      # per model: the lone trainer's tensor list (name, shape, offset, n, step)
        for k, fpe in enumerate(fpes):   # a lone trainer per model builds the slot: one code path for blob and state
            ft = FPETrainer(fpe, device=self.device, state=states[k] if states else None, **self._kw)
            self.load(k, ft)
        self._jobs_dev = torch.empty(max(self.M, 1) * JOB_DTYPE.itemsize, dtype=torch.uint8, device=self.device)

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _desc(self):
        ts = self.tensors[0]
        return adamw.descriptors(ts), len(ts)

    # ---------------- one model as a lone FPETrainer, and back ----------------
    def trainer(self, m: int) -> FPETrainer:
        """Slot m as a lone ``FPETrainer`` (weights, gradient, moments, step
        counts): ``checkpoint()`` on it writes what a lone run writes."""
        ft = FPETrainer(self.weights_numpy(m), device=self.device, **self._kw)
        ft.P.copy_(self.P[m])
        ft.G.copy_(self.G[m])
        ft.m.copy_(self.m[m])
        ft.v.copy_(self.v[m])
        for t, s in zip(ft.tensors, self.tensors[m]):
            t["step"] = s["step"]
        return ft

    def load(self, m: int, ft: FPETrainer):
        """The reverse of ``trainer(m)``: slot m continues from that trainer."""
        if ft.H != self.H:
            raise ValueError("load: the trainer's host count differs from the fleet's")
        self.P[m].copy_(ft.P)
        self.G[m].copy_(ft.G)
        self.m[m].copy_(ft.m)
        self.v[m].copy_(ft.v)
        ts = [dict(t) for t in ft.tensors]
        if m < len(self.tensors):
            self.tensors[m] = ts
        else:
            assert m == len(self.tensors)
            self.tensors.append(ts)

    def weights_numpy(self, m: int) -> dict:
        p = self.P[m].detach().cpu().numpy().astype(np.float64)
        return {t["name"]: p[t["offset"]:t["offset"] + t["n"]].reshape(t["shape"]) for t in self.tensors[m]}

    # ---------------- the pools of one call ----------------
    def _pools(self, wins, h0s, labels=None):
        """Job table and pools of a call over per-model lists (None or empty: the
        model sits the call out).  Models given the SAME window (and label)
        objects share one range of the window pool; the step-indexed rows are
        each job's own."""
        H = self.H
        jobs = np.zeros(self.M, dtype=JOB_DTYPE)
        wparts, lparts, hparts, seen, nw, ns = [], [], [], {}, 0, 0
        for k in range(self.M):
            n = 0 if wins[k] is None else len(wins[k])
            if n == 0:
                continue
            key = (id(wins[k]),) + (tuple(id(a[k]) for a in labels) if labels else ())
            if key not in seen:
                seen[key] = nw
                wparts.append(np.asarray(wins[k], dtype=np.float32).reshape(n, 3, 3 * H))
                if labels:
                    lparts.append([np.asarray(a[k]).reshape(n, H) for a in labels])
                nw += n
            hparts.append(np.asarray(h0s[k], dtype=np.float32).reshape(n, 3))
            jobs[k] = (seen[key], ns, n, 0)
            ns += n
        dev = self.device
        up = lambda parts, dt, shape: torch.as_tensor(
            np.concatenate(parts) if parts else np.zeros(shape, dtype=dt), dtype=getattr(torch, np.dtype(dt).name)
        ).to(dev).contiguous()
        w = up(wparts, np.float32, (0, 3, 3 * H))
        h = up(hparts, np.float32, (0, 3))
        lab = [up([p[i] for p in lparts], np.int32, (0, H)) for i in range(len(labels))] if labels else []
        return jobs, nw, ns, w, h, lab

    def backprop(self, sts, wins, h0s, anom, cls):
        """``FPETrainer.backprop`` of every model, in one launch.  Per-model
        lists (ragged; None or empty: the model sits this call out): sts
        [M] TuneState, wins[m] [n_m,3,3H], h0s[m] [n_m,3], anom / cls [m]
        [n_m,H].  Returns the per-model lists of (aloss, tloss) and updates each
        TuneState."""
        M, H, dev = self.M, self.H, self.device
        live = [k for k in range(M) if wins[k] is not None and len(wins[k]) > 0]
        for k in live:
            sts[k].num_zero, sts[k].num_ones = 1, 1
        K = sts[0].protos.shape[0]
        if any(s.protos.shape[0] != K for s in sts):
            raise ValueError("backprop: the models' prototype counts differ")
        jobs, nw, ns, w, h, (y, c) = self._pools(wins, h0s, labels=(anom, cls))
        c = torch.clamp(c, 0, 2)
        state = torch.tensor(np.stack([s.vector() for s in sts]), dtype=torch.float64, device=dev)
        losses = torch.zeros((ns, 2), dtype=torch.float64, device=dev)
        nt = len(self.tensors[0])
        table = np.zeros((ns, nt, 3), dtype=np.float32)
        for k in live:
            a = np.asarray(anom[k]).reshape(int(jobs[k]["n"]), H)
            o = int(jobs[k]["step_off"])
            table[o:o + len(a)] = adam_table(self.tensors[k], np.any(a > 0, axis=1), self.lr, self.b1, self.b2)
        sched = torch.from_numpy(table).to(dev)
        desc, nd = self._desc()
        _native.check(self._L.pgp_fpe_train_steps_many(
            H, K, M, jobs.ctypes.data, nw, w.data_ptr(), y.data_ptr(), c.data_ptr(), ns, h.data_ptr(),
            sched.data_ptr(), losses.data_ptr(), self.P.data_ptr(), self.G.data_ptr(), self.m.data_ptr(),
            self.v.data_ptr(), state.data_ptr(), PROTO_UPDATE_MIN, PROTO_FACTOR_DECAY, self.lr, self.wd, self.b1,
            self.b2, self.eps, desc, nd, self._jobs_dev.data_ptr(), self._stream()), "pgp_fpe_train_steps_many")
        sv, ls = state.cpu().numpy(), losses.cpu().numpy()    # the copies wait for the stream: `jobs` may go now
        out = [[] for _ in range(M)]
        for k in live:
            sts[k].from_vector(sv[k])
            o, n = int(jobs[k]["step_off"]), int(jobs[k]["n"])
            out[k] = [tuple(r) for r in ls[o:o + n].tolist()]
        return out

    def forward_many(self, wins, h0s):
        """Every model's independent forwards in one launch: per model (probs,
        protos) [n_m,H,2] fp64, None for a model that sits the call out."""
        M, H, dev = self.M, self.H, self.device
        jobs, nw, ns, w, h, _ = self._pools(wins, h0s)
        out = torch.zeros((2, ns, H, 2), dtype=torch.float64, device=dev)
        _native.check(self._L.pgp_fpe_forward_many_cells(
            H, M, jobs.ctypes.data, nw, w.data_ptr(), ns, h.data_ptr(), self.P.data_ptr(), out[0].data_ptr(),
            out[1].data_ptr(), self._jobs_dev.data_ptr(), self._stream()), "pgp_fpe_forward_many_cells")
        o = out.cpu().numpy()
        res = []
        for k in range(M):
            s, n = int(jobs[k]["step_off"]), int(jobs[k]["n"])
            res.append((o[0, s:s + n], o[1, s:s + n]) if n else None)
        return res

    def accuracy(self, sts, wins, h0s, anom, cls):
        """``FPETrainer.accuracy`` of every model from one launch: per model
        (AScore, CScore), None for a model that sits the call out."""
        fw = self.forward_many(wins, h0s)
        return [None if f is None else accuracy_scores(f[0], f[1], anom[k], cls[k], sts[k].protos)
                for k, f in enumerate(fw)]


def train_fleet(fpes, prototypes, time_data, num_epochs, generators=None, H=16, device="cuda"):
    """``PreGANRecovery.train_model``'s epoch loop (PreGAN.py:39-49) for M
    models at once: fpes / prototypes / time_data / generators are per-model
    lists (models given the same time_data object share its windows: a seed
    sweep over one series).  Model m draws its GRU states from generators[m] in
    the lone order (per epoch backprop's N, then accuracy's N).  Returns per
    model (weights, prototypes, accuracy_list) as the lone run's."""
    from .train import load_dataset
    M = len(fpes)
    generators = generators or [None] * M
    sets = {}
    for td in time_data:
        if id(td) not in sets:
            sets[id(td)] = load_dataset(td)
    wins, anom, cls = ([sets[id(td)][i] for td in time_data] for i in range(3))
    fleet = FPEFleetTrainer(fpes, H=H, device=device)
    sts = [TuneState(p) for p in prototypes]
    acc = [[] for _ in range(M)]
    for _ in range(num_epochs):
        losses = fleet.backprop(sts, wins, [draw_h0(len(w), g) for w, g in zip(wins, generators)], anom, cls)
        factors = [st.factor + PROTO_UPDATE_MIN for st in sts]
        scores = fleet.accuracy(sts, wins, [draw_h0(len(w), g) for w, g in zip(wins, generators)], anom, cls)
        for k in range(M):
            loss = float(np.mean([a for a, _ in losses[k]]) + np.mean([t for _, t in losses[k]]))   # train.py:56-57
            acc[k].append((loss, factors[k]) + tuple(scores[k]))
    return [(fleet.weights_numpy(k), sts[k].protos.copy(), acc[k]) for k in range(M)]
