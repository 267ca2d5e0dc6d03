"""PreGAN's FPE trained an epoch per launch and a fleet of FPEs at once:
pgp_fpe_train_steps, pgp_fpe_train_steps_many and pgp_fpe_forward_many_cells against the lone
two-launch loop (pgp_fpe_train_step + its AdamW) and pgp_fpe_forward_many, whose parity to
the reference tests/test_gpu_fpetrain.py and tests/test_gpu_fpetrain50.py pin.  Every
comparison is on bytes; the fused update is also replayed in fp64 from its own gradient."""
import ctypes

import numpy as np
import pytest
import torch

from preganplus_amd import _native
from preganplus_amd import fpetrain as FT
from preganplus_amd import train as TR
from preganplus_amd import weights as W
from preganplus_amd.fpetrain import COND

pytestmark = pytest.mark.gpu

SENT = -7.25
eq = np.testing.assert_array_equal


def fixture(H):
    z = np.load(f"tests/golden/fpe_train_h{H}.npz")
    return z["wins"], z["anom"], z["cls"], z["ep0/h0_backprop"]


def protos0():
    return np.random.default_rng(1).uniform(0.1, 0.9, (3, 2))


def fresh(H, seed=3):
    return FT.FPETrainer(W.synth_fpe_weights(H, seed=seed)["fpe"], H=H)


def bufs(ft):
    torch.cuda.synchronize()
    return {k: getattr(ft, k).cpu().numpy().copy() for k in "PGmv"}


def same_trainers(a, b):
    for k, x in bufs(a).items():
        eq(x.view(np.uint32), bufs(b)[k].view(np.uint32), err_msg=k)
    assert [t["step"] for t in a.tensors] == [t["step"] for t in b.tensors]


def dev(a, dt):
    return torch.as_tensor(np.asarray(a), dtype=dt).cuda().contiguous()


class Rows:
    """One dataset on the device: windows, GRU states, labels."""

    def __init__(self, H, wins, h0, anom, cls):
        self.H, self.n = H, len(wins)
        self.w, self.h = dev(wins, torch.float32), dev(h0, torch.float32).reshape(-1, 3)
        self.y, self.c = dev(anom, torch.int32), dev(np.clip(cls, 0, 2), torch.int32)
        self.positive = np.any(np.asarray(anom) > 0, axis=1)


def train_steps(ft, rows, lo, hi, state, sched, loss):
    """pgp_fpe_train_steps on rows [lo, hi) of a dataset, its table and its loss rows."""
    _native.check(ft._L.pgp_fpe_train_steps(
        ft.H, 3, hi - lo, rows.w[lo:].data_ptr(), rows.h[lo:].data_ptr(), rows.y[lo:].data_ptr(),
        rows.c[lo:].data_ptr(), ft.P.data_ptr(), ft.G.data_ptr(), ft.m.data_ptr(), ft.v.data_ptr(), state.data_ptr(),
        TR.PROTO_UPDATE_MIN, TR.PROTO_FACTOR_DECAY, ft.lr, ft.wd, ft.b1, ft.b2, ft.eps, ft._desc(), len(ft.tensors),
        sched[lo:].data_ptr(), loss[lo:].data_ptr(), ft._stream()), "pgp_fpe_train_steps")


# ---------------------------------------------------------------------------
# one launch against the lone loop
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("H, lo, n", [(16, 0, 1), (16, 0, 2), (16, 0, 6), (50, 5, 3)])
def test_one_launch_equals_the_lone_loop(H, lo, n):
    """n = 2 is the smallest run in which a stale parameter read shows; the n = 6 run (and H = 50's 3)
    holds a window without a positive label that is not the last one."""
    wins, anom, cls, h0 = (a[lo:lo + n] for a in fixture(H))
    positive = np.any(anom > 0, axis=1)
    if n >= 3:
        assert not positive[:-1].all() and positive.any()
    a, b = fresh(H), fresh(H)
    sa, sb = TR.TuneState(protos0(), 0.2), TR.TuneState(protos0(), 0.2)
    la = a.backprop(sa, wins, h0, anom, cls, one_launch=True)
    lb = b.backprop(sb, wins, h0, anom, cls)
    same_trainers(a, b)
    eq(sa.vector().view(np.uint64), sb.vector().view(np.uint64))
    eq(np.asarray(la).view(np.uint64), np.asarray(lb).view(np.uint64))
    assert len(la) == n and a.tensors[0]["step"] == n
    if not positive.all():
        assert {t["name"] for t in a.tensors if t["step"] < n} == set(COND)


def test_six_steps_equal_one_two_three():
    H = 16
    rows = Rows(H, *[fixture(H)[i][:6] for i in (0, 3, 1, 2)])
    out = []
    for parts in ((6,), (1, 2, 3)):
        ft = fresh(H)
        sched = torch.from_numpy(ft.adam_table(rows.positive)).cuda()
        state = torch.tensor(TR.TuneState(protos0(), 0.2).vector(), dtype=torch.float64, device="cuda")
        loss = torch.zeros((6, 2), dtype=torch.float64, device="cuda")
        lo = 0
        for p in parts:
            train_steps(ft, rows, lo, lo + p, state, sched, loss)
            lo += p
        out.append((bufs(ft), state.cpu().numpy(), loss.cpu().numpy()))
    for k in "PGmv":
        eq(out[0][0][k].view(np.uint32), out[1][0][k].view(np.uint32), err_msg=k)
    eq(out[0][1].view(np.uint64), out[1][1].view(np.uint64))
    eq(out[0][2].view(np.uint64), out[1][2].view(np.uint64))


@pytest.mark.parametrize("H", [16, 50])
def test_fused_update_replays_in_fp64(H):
    """tests/test_gpu_adamw_fused.py::test_fpe_step_replays through pgp_fpe_train_steps: one step replayed
    from its own G inside tests/adamw_replay's bounds, the second call without a positive label."""
    from tests.test_gpu_adamw_fused import replay_step, snap, steps_of, tune_inputs
    fpe = dict(W.synth_fpe_weights(H, seed=3)["fpe"])
    for k in ("mha.in_proj_bias", "mha.out_proj.bias"):
        fpe[k] = np.zeros_like(fpe[k])
    ft = FT.FPETrainer(fpe, H=H)
    st = TR.TuneState(protos0(), 0.2)
    rng = np.random.default_rng(H)
    for call in range(2):
        wins, anom, cls = tune_inputs(H, 1, 30 * H + call, positive=call == 0)
        h0 = rng.standard_normal((1, 3)).astype(np.float32)
        before, steps0 = snap(ft), steps_of(ft)
        ft.backprop(st, wins, h0, anom, cls, one_launch=True)
        _, stepped = replay_step(f"pgp_fpe_train_steps H={H} call {call}", ft, before, steps0, steps_of(ft),
                                 lambda t: ft.lr)
        want = {t["name"] for t in ft.tensors} - (set(COND) if call == 1 else set())
        assert stepped == want, stepped ^ want


# ---------------------------------------------------------------------------
# fleet: pgp_fpe_train_steps_many against pgp_fpe_train_steps per model
# ---------------------------------------------------------------------------
class Fleet:
    """M slots and the pools of one _many call, built from per-model (weights blob, window range, h0)."""

    def __init__(self, H, blobs, ranges, h0s, rows, spare=0):
        self.H, self.M, self.rows = H, len(blobs), rows
        self.ft = fresh(H)                                      # the tensor table and the scalars
        self.len = self.ft.P.numel()
        self.jobs = np.zeros(self.M, dtype=FT.JOB_DTYPE)
        hs, tabs, ns = [], [], 0
        for m, ((lo, n), h0) in enumerate(zip(ranges, h0s)):
            self.jobs[m] = (lo, ns, n, 0)
            if n:
                hs.append(np.asarray(h0, dtype=np.float32).reshape(n, 3))
                tabs.append(FT.adam_table([dict(t, step=0.0) for t in self.ft.tensors], rows.positive[lo:lo + n],
                                          self.ft.lr, self.ft.b1, self.ft.b2))
            else:                                               # rows nobody may touch
                hs.append(np.full((spare, 3), SENT, dtype=np.float32))
                tabs.append(np.full((spare, len(self.ft.tensors), 3), SENT, dtype=np.float32))
            ns += n if n else spare
        self.ns = ns
        self.h, self.sched = dev(np.concatenate(hs), torch.float32), dev(np.concatenate(tabs), torch.float32)
        self.P = dev(np.stack(blobs), torch.float32)
        self.G, self.m, self.v = (torch.zeros_like(self.P) for _ in range(3))
        self.state = dev(np.tile(TR.TuneState(protos0(), 0.2).vector(), (self.M, 1)), torch.float64)
        self.loss = torch.full((ns, 2), SENT, dtype=torch.float64, device="cuda")
        self.jobs_dev = torch.empty(self.M * FT.JOB_DTYPE.itemsize, dtype=torch.uint8, device="cuda")

    def snapshot(self):
        torch.cuda.synchronize()
        return {k: getattr(self, k).cpu().numpy().copy() for k in ("P", "G", "m", "v", "state", "loss")}

    def run_many(self):
        ft, r = self.ft, self.rows
        _native.check(ft._L.pgp_fpe_train_steps_many(
            self.H, 3, self.M, self.jobs.ctypes.data, r.n, r.w.data_ptr(), r.y.data_ptr(), r.c.data_ptr(), self.ns,
            self.h.data_ptr(), self.sched.data_ptr(), self.loss.data_ptr(), self.P.data_ptr(), self.G.data_ptr(),
            self.m.data_ptr(), self.v.data_ptr(), self.state.data_ptr(), TR.PROTO_UPDATE_MIN, TR.PROTO_FACTOR_DECAY,
            ft.lr, ft.wd, ft.b1, ft.b2, ft.eps, ft._desc(), len(ft.tensors), self.jobs_dev.data_ptr(), ft._stream()),
            "pgp_fpe_train_steps_many")
        return self.snapshot()

    def run_lone(self, models=None):
        """pgp_fpe_train_steps on each slot alone, with that job's ranges."""
        ft, r = self.ft, self.rows
        for m in range(self.M) if models is None else models:
            lo, so, n = (int(self.jobs[m][k]) for k in ("window_off", "step_off", "n"))
            if n == 0:
                continue
            _native.check(ft._L.pgp_fpe_train_steps(
                self.H, 3, n, r.w[lo:].data_ptr(), self.h[so:].data_ptr(), r.y[lo:].data_ptr(), r.c[lo:].data_ptr(),
                self.P[m].data_ptr(), self.G[m].data_ptr(), self.m[m].data_ptr(), self.v[m].data_ptr(),
                self.state[m].data_ptr(), TR.PROTO_UPDATE_MIN, TR.PROTO_FACTOR_DECAY, ft.lr, ft.wd, ft.b1, ft.b2,
                ft.eps, ft._desc(), len(ft.tensors), self.sched[so:].data_ptr(), self.loss[so:].data_ptr(),
                ft._stream()), "pgp_fpe_train_steps")
        return self.snapshot()


def blobs_of(H, M, seed=0):
    """M weight blobs: a synthetic FPE and seeded relative perturbations of it (fp32)."""
    base = fresh(H).P.cpu().numpy()
    rng = np.random.default_rng(seed)
    return [base] + [(base * (1 + 0.05 * rng.standard_normal(base.size))).astype(np.float32) for _ in range(M - 1)]


def h0_of(n, seed):
    return np.random.default_rng(seed).standard_normal((n, 3)).astype(np.float32)


def same_snapshots(a, b, what=""):
    for k in a:
        eq(a[k].view(np.uint64 if a[k].dtype == np.float64 else np.uint32),
           b[k].view(np.uint64 if b[k].dtype == np.float64 else np.uint32), err_msg=f"{what} {k}")


def test_fleet_ragged_jobs_equal_their_lone_runs():
    """Jobs of n = (6, 0, 4, 1): jobs 0 and 2 share a window range with different h0 rows; the n = 0 job's
    slot, state row and pool rows hold a sentinel and come back untouched."""
    H = 16
    rows = Rows(H, *[fixture(H)[i][:8] for i in (0, 3, 1, 2)])
    assert not rows.positive[:6].all() and rows.positive[:6].any()
    ranges = [(0, 6), (0, 0), (0, 4), (6, 1)]

    def build():
        f = Fleet(H, blobs_of(H, 4), ranges, [h0_of(n, 10 + m) for m, (_, n) in enumerate(ranges)], rows, spare=2)
        for a in (f.P, f.G, f.m, f.v, f.state):
            a[1].fill_(SENT)
        return f

    many, lone = build().run_many(), build().run_lone()
    same_snapshots(many, lone)
    for k in ("P", "G", "m", "v", "state"):
        assert (many[k][1] == SENT).all(), k
    assert (many["loss"][6:8] == SENT).all() and not (many["loss"][:6] == SENT).any()
    assert not np.array_equal(many["loss"][:4], many["loss"][8:12])        # the shared windows, other GRU states
    assert not np.array_equal(many["P"][0], many["P"][2])


def test_a_model_has_the_same_bits_wherever_it_sits():
    """One model at slot 0 of 1, slot 2 of 3 and the last of 300 (more workgroups than CUs), n = 2 everywhere;
    the other 299 equal their own lone runs."""
    H, n = 16, 2
    rows = Rows(H, *[fixture(H)[i][:4] for i in (0, 3, 1, 2)])
    pool = blobs_of(H, 300)
    x_blob, x_h0 = pool[7], h0_of(n, 99)
    got = []
    for M, slot in ((1, 0), (3, 2), (300, 299)):
        blobs = [pool[(k + 1) % 300] for k in range(M)]
        h0s = [h0_of(n, 200 + k) for k in range(M)]
        blobs[slot], h0s[slot] = x_blob, x_h0
        mk = lambda: Fleet(H, blobs, [(1, n)] * M, h0s, rows)
        many = mk().run_many()
        got.append({k: many[k][slot] if k != "loss" else many[k][slot * n:(slot + 1) * n] for k in many})
        if M == 300:
            same_snapshots(many, mk().run_lone(), "300 models")
    same_snapshots(got[0], got[1], "slot 2 of 3")
    same_snapshots(got[0], got[2], "slot 299 of 300")
    assert not np.array_equal(got[0]["P"], x_blob)


def test_fleet_h50_and_run_to_run():
    H = 50
    rows = Rows(H, *[fixture(H)[i][4:8] for i in (0, 3, 1, 2)])
    assert not rows.positive.all()
    mk = lambda: Fleet(H, blobs_of(H, 2), [(1, 3), (0, 3)], [h0_of(3, 5), h0_of(3, 6)], rows)
    first, second, lone = mk().run_many(), mk().run_many(), mk().run_lone()
    same_snapshots(first, second, "run to run")
    same_snapshots(first, lone)


# ---------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("H, ns", [(16, (5, 1, 3)), (50, (2, 2))])
def test_forward_cells_equals_forward_many_per_model(H, ns):
    M = len(ns)
    wins = fixture(H)[0][:6]
    w = dev(wins, torch.float32)
    P = dev(np.stack(blobs_of(H, M)), torch.float32)
    jobs = np.zeros(M, dtype=FT.JOB_DTYPE)
    off = 0
    for m, n in enumerate(ns):
        jobs[m] = (m, off, n, 0)                                 # overlapping window ranges, own step rows
        off += n
    h = dev(h0_of(off, 3), torch.float32)
    L = _native.lib()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    got = torch.full((2, off, H, 2), SENT, dtype=torch.float64, device="cuda")
    jobs_dev = torch.empty(M * FT.JOB_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    _native.check(L.pgp_fpe_forward_many_cells(H, M, jobs.ctypes.data, len(wins), w.data_ptr(), off, h.data_ptr(),
                                               P.data_ptr(), got[0].data_ptr(), got[1].data_ptr(),
                                               jobs_dev.data_ptr(), st), "pgp_fpe_forward_many_cells")
    want = torch.full_like(got, SENT)
    for m, n in enumerate(ns):
        so = int(jobs[m]["step_off"])
        _native.check(L.pgp_fpe_forward_many(H, n, w[m:].data_ptr(), h[so:].data_ptr(), P[m].data_ptr(),
                                             want[0, so:].data_ptr(), want[1, so:].data_ptr(), st),
                      "pgp_fpe_forward_many")
    torch.cuda.synchronize()
    g, x = got.cpu().numpy(), want.cpu().numpy()
    assert not (x == SENT).any()
    eq(g.view(np.uint64), x.view(np.uint64))


# ---------------------------------------------------------------------------
# Python: FPEFleetTrainer, train_fleet, train_model(one_launch=True)
# ---------------------------------------------------------------------------
def ckpt_equal(a, b):
    assert a["epoch"] == b["epoch"] and a["accuracy_list"] == b["accuracy_list"]
    for k in a["model_state_dict"]:
        eq(a["model_state_dict"][k].numpy(), b["model_state_dict"][k].numpy(), err_msg=k)
    for p, q in zip(a["model_prototypes"], b["model_prototypes"]):
        eq(p.numpy(), q.numpy())
    sa, sb = a["optimizer_state_dict"]["state"], b["optimizer_state_dict"]["state"]
    assert sorted(sa) == sorted(sb)
    for i in sa:
        for k in ("step", "exp_avg", "exp_avg_sq"):
            eq(sa[i][k].numpy(), sb[i][k].numpy(), err_msg=f"{i} {k}")
    assert a["optimizer_state_dict"]["param_groups"] == b["optimizer_state_dict"]["param_groups"]


def test_fleet_trainer_equals_three_lone_trainers():
    """3 models, 2 epochs: two seeds over one 8-window series, a third model on a 5-window series; the
    reference is train_model's loop on three lone trainers with equally seeded generators."""
    H, epochs = 16, 2
    rng = np.random.default_rng(4)
    s8, s5 = rng.uniform(0, 100, size=(8, 3 * H)), rng.uniform(0, 100, size=(5, 3 * H))
    series, seeds = [s8, s8, s5], [11, 12, 13]
    fpes = [W.synth_fpe_weights(H, seed=s)["fpe"] for s in (3, 3, 4)]
    gen = lambda: [torch.Generator().manual_seed(s) for s in seeds]
    # the lone runs
    want = []
    for fpe, td, g in zip(fpes, series, gen()):
        wins, anom, cls = TR.load_dataset(td)
        ft, st, acc = FT.FPETrainer(fpe, H=H), TR.TuneState(protos0()), []
        for ep in range(epochs):
            losses = ft.backprop(st, wins, FT.draw_h0(len(wins), g), anom, cls)
            loss = float(np.mean([a for a, _ in losses]) + np.mean([t for _, t in losses]))
            factor = st.factor + TR.PROTO_UPDATE_MIN
            acc.append((loss, factor) + tuple(ft.accuracy(st, wins, FT.draw_h0(len(wins), g), anom, cls)))
        want.append((ft, st, acc))
    # the fleet, by hand
    sets = {id(td): TR.load_dataset(td) for td in series}
    wins, anom, cls = ([sets[id(td)][i] for td in series] for i in range(3))
    fleet = FT.FPEFleetTrainer(fpes, H=H)
    sts, gs, acc = [TR.TuneState(protos0()) for _ in range(3)], gen(), [[] for _ in range(3)]
    for ep in range(epochs):
        losses = fleet.backprop(sts, wins, [FT.draw_h0(len(w), g) for w, g in zip(wins, gs)], anom, cls)
        factors = [st.factor + TR.PROTO_UPDATE_MIN for st in sts]
        scores = fleet.accuracy(sts, wins, [FT.draw_h0(len(w), g) for w, g in zip(wins, gs)], anom, cls)
        for m in range(3):
            loss = float(np.mean([a for a, _ in losses[m]]) + np.mean([t for _, t in losses[m]]))
            acc[m].append((loss, factors[m]) + tuple(scores[m]))
    trained = FT.train_fleet(fpes, [protos0()] * 3, series, epochs, generators=gen(), H=H)
    for m, (ft, st, a) in enumerate(want):
        lone_w = ft.weights_numpy()
        for k, x in lone_w.items():
            eq(fleet.weights_numpy(m)[k], x, err_msg=f"model {m} {k}")
            eq(trained[m][0][k], x, err_msg=f"train_fleet model {m} {k}")
        eq(sts[m].protos, st.protos)
        eq(trained[m][1], st.protos)
        assert acc[m] == a and trained[m][2] == a, m
        assert (sts[m].factor, sts[m].num_zero, sts[m].num_ones) == (st.factor, st.num_zero, st.num_ones)
        ckpt_equal(fleet.trainer(m).checkpoint(epochs - 1, acc[m], sts[m].protos),
                   ft.checkpoint(epochs - 1, a, st.protos))
    assert not np.array_equal(fleet.P[0].cpu().numpy(), fleet.P[1].cpu().numpy())   # the two seeds diverged
    # a model that sits a call out keeps its slot; load() is trainer()'s inverse
    before = fleet.P.cpu().numpy().copy()
    out = fleet.backprop(sts, [None, wins[1], []], [None, FT.draw_h0(8), None], anom, cls)
    after = fleet.P.cpu().numpy()
    assert out[0] == [] and out[2] == [] and len(out[1]) == 8
    eq(after[[0, 2]], before[[0, 2]])
    assert not np.array_equal(after[1], before[1])
    fleet.load(0, fleet.trainer(1))
    eq(fleet.P[0].cpu().numpy(), after[1])
    assert [t["step"] for t in fleet.tensors[0]] == [t["step"] for t in fleet.tensors[1]]


def test_train_model_one_launch_equals_the_default():
    from preganplus_amd.recovery import PreGANRecovery
    w, extra = W.load_npz("preganplus_amd/data/pregan_simulator_16.npz")
    series = np.random.default_rng(6).uniform(0, 100, size=(9, 48))
    out = []
    for one in (True, False):
        rec = PreGANRecovery(16, "", training=False, weights=w, extra=extra)
        rec.fpe_epoch, rec.fpe_accuracy_list = -1, []                    # as _load_new_model does
        g = torch.Generator().manual_seed(21)
        fpe, protos = rec.train_model(w["fpe"], protos0(), series, num_epochs=2, generator=g, one_launch=one)
        out.append((fpe, protos, rec.fpe_accuracy_list, rec.fpe_epoch, [t["step"] for t in rec.fpe_trainer.tensors]))
    for k in out[0][0]:
        eq(out[0][0][k], out[1][0][k], err_msg=k)
    eq(out[0][1], out[1][1])
    assert out[0][2:] == out[1][2:] and out[0][3] == 1 and len(out[0][2]) == 2


# ---------------------------------------------------------------------------
# unsupported host counts
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("H", [8, 32])
def test_unsupported_host_counts_raise(H):
    L = _native.lib()
    buf = torch.zeros(4096, dtype=torch.float64, device="cuda")
    p = buf.data_ptr()
    jobs = np.zeros(1, dtype=FT.JOB_DTYPE)
    jobs[0] = (0, 0, 1, 0)
    desc = (TR._AdamTensor * 1)(TR._AdamTensor(0, 1, 1, 0.0, 0.0))
    hyper = (TR.PROTO_UPDATE_MIN, TR.PROTO_FACTOR_DECAY, 1e-4, 1e-5, 0.9, 0.999, 1e-8)
    calls = {
        "pgp_fpe_train_steps": lambda: L.pgp_fpe_train_steps(H, 3, 1, *[p] * 9, *hyper, desc, 1, p, p, None),
        "pgp_fpe_train_steps_many": lambda: L.pgp_fpe_train_steps_many(
            H, 3, 1, jobs.ctypes.data, 1, p, p, p, 1, *[p] * 8, *hyper, desc, 1, p, None),
        "pgp_fpe_forward_many_cells": lambda: L.pgp_fpe_forward_many_cells(H, 1, jobs.ctypes.data, 1, p, 1, p, p, p, p,
                                                                           p, None),
    }
    for name, call in calls.items():
        with pytest.raises(_native.NativeError, match="PGP_ERR_UNSUPPORTED"):
            _native.check(call(), name)
    torch.cuda.synchronize()
    assert not buf.any()
