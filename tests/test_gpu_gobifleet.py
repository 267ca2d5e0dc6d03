"""GPU: a fleet of GOBI surrogates: M models trained in one launch
(pgp_gobi_train_steps_many / _eval_many, GOBIFleetTrainer) and every
environment optimised against its own (pgp_gobi_optimize_groups,
GOBIOptimizer(weights=[...]).optimize(model_of=...)).

Every expected value comes from the single-model entries (GOBITrainer,
GOBIOptimizer on one state dict), which tests/test_gpu_gobitrain.py and
tests/test_gpu_gobi.py pin to the reference; the comparisons are bytewise.
The model is 61,890 parameters and the step counts are tens."""
import os
import random

import numpy as np
import pytest
import torch

from tests import gobitrain_ref as R

pytestmark = pytest.mark.gpu
SIM_CSV = os.path.join(R.GOLD, "energy_latency_16_scheduling_simulator400.csv")


def same(a, b, what=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    assert a.tobytes() == b.tobytes(), f"{what}: {int((a != b).sum())} of {a.size} values differ"


@pytest.fixture(scope="module")
def data():
    """[the committed 199-sample set, its samples 0-119, the 399-sample simulator set]"""
    from preganplus_amd.gobitrain import load_energy_latency_data
    z = R.fixture()
    fa, ta = np.asarray(z["feats"]), np.asarray(z["targets"])
    fc, tc, max_ips = load_energy_latency_data(SIM_CSV)
    assert fa.shape[0] == 199 and fc.shape[0] == 399 and abs(max_ips - 5028.639096) < 1e-6   # the header quirk
    return [(fa, ta), (fa[:120], ta[:120]), (fc, tc)]


@pytest.fixture(scope="module")
def seeds():
    from preganplus_amd.gobitrain import fresh_weights
    return {s: fresh_weights(s) for s in (16, 17, 18)}


def _single(weights, dataset, lr=None, state=None):
    from preganplus_amd.gobitrain import GOBITrainer
    t = GOBITrainer(weights=weights, state=state)
    if lr is not None:
        t.lr = lr
    t.set_data(*dataset)
    return t


def _state(t):
    return [a.cpu().numpy().copy() for a in (t.P, t.m, t.v)]


def _slot(f, m):
    return [a[m].cpu().numpy().copy() for a in (f.P, f.m, f.v)]


def _orders(rng_seed, sizes, counts):
    rng = np.random.RandomState(rng_seed)
    return [rng.randint(0, n, size=c).tolist() for n, c in zip(sizes, counts)]


# ---- 1, 2: ragged training ----

@pytest.fixture(scope="module")
def ragged(data, seeds):
    """M = 3: n = (24, 7, 0), step0 = (0, 12, 0), lr = (1e-4, 3e-4, 1e-4); job 1
    resumes a 12-step lone run with its moments.  Returns what builds the fleet
    and each model's lone run."""
    o0, o1, pre1 = _orders(3, (199, 120, 120), (24, 7, 12))
    one = _single(seeds[17], data[1], lr=3e-4)
    one.backprop(pre1)
    w1, ck1 = one.weights_numpy(), one.checkpoint(0, [])["optimizer_state_dict"]
    assert one.step == 12 and ck1["param_groups"][0]["lr"] == 3e-4
    l1 = one.backprop(o1)
    zero = _single(seeds[16], data[0])
    l0 = zero.backprop(o0)
    two = _single(seeds[18], data[2])
    return dict(weights=[seeds[16], w1, seeds[18]], states=[None, ck1, None], orders=[o0, o1, []],
                want=[_state(zero) + [l0], _state(one) + [l1], _state(two) + [np.zeros(0, np.float32)]],
                steps=[24, 19, 0])


def _fleet(ragged, data):
    from preganplus_amd.gobitrain import GOBIFleetTrainer
    f = GOBIFleetTrainer(weights=ragged["weights"], states=ragged["states"])
    f.set_data(data)
    assert f.steps == [0, 12, 0] and [h["lr"] for h in f.hypers] == [1e-4, 3e-4, 1e-4]
    return f


def test_ragged_train_bytewise(ragged, data):
    runs = []
    for _ in range(2):
        f = _fleet(ragged, data)
        losses = f.backprop(ragged["orders"])
        assert f.steps == ragged["steps"]
        runs.append([_slot(f, m) + [losses[m]] for m in range(3)])
    for m in range(3):
        for got, again, want, what in zip(runs[0][m], runs[1][m], ragged["want"][m], ("P", "m", "v", "loss")):
            same(got, want, f"model {m} {what} against its lone GOBITrainer")
            same(got, again, f"model {m} {what}, second run")
    assert not runs[0][2][1].any() and not runs[0][2][2].any()   # slot 2 (n = 0): moments still zero


def test_launch_equivalence(ragged, data):
    """One many-launch of n steps == the same jobs split as 5 + 2 + rest."""
    f = _fleet(ragged, data)
    parts = [f.backprop([o[a:b] for o in ragged["orders"]]) for a, b in ((0, 5), (5, 7), (7, None))]
    assert f.steps == ragged["steps"]
    for m in range(3):
        got = _slot(f, m) + [np.concatenate([p[m] for p in parts])]
        for g, want, what in zip(got, ragged["want"][m], ("P", "m", "v", "loss")):
            same(g, want, f"model {m} {what}")


# ---- 3: more models than compute units ----

def test_more_models_than_cus(data, seeds):
    from preganplus_amd.gobitrain import GOBIFleetTrainer
    M, order = 300, [150, 3]
    keys = (16, 17, 18)
    f = GOBIFleetTrainer(weights=[seeds[keys[m % 3]] for m in range(M)])
    f.set_data([data[0]])
    losses = np.stack(f.backprop([order] * M))
    P, mm, v = (a.cpu().numpy() for a in (f.P, f.m, f.v))
    for a in (P, mm, v, losses):
        assert not np.isnan(a).any()
    want = []
    for k in keys:
        t = _single(seeds[k], data[0])
        loss = t.backprop(order)
        want.append(_state(t) + [loss])
    for a, what in zip((P, mm, v, losses), ("P", "m", "v", "loss")):
        for r in range(3):   # all slots with equal inputs hold equal bits
            assert (a[r::3].view(np.uint32) == a[r].view(np.uint32)).all(), (what, r)
    for m in (0, 1, 2, 255, 256, 299):
        for a, w, what in zip((P, mm, v, losses), want[m % 3], ("P", "m", "v", "loss")):
            same(a[m], w, f"slot {m} {what}")


# ---- 4: eval ----

def test_eval_many(data, seeds):
    from preganplus_amd.gobitrain import GOBIFleetTrainer
    f = GOBIFleetTrainer(weights=[seeds[16], seeds[17], seeds[18]])
    f.set_data(data)
    lists = _orders(4, (199, 120, 399), (40, 0, 13))
    lists[2][5] = 398   # the pool's last sample
    want = [_single(seeds[k], d).accuracy(o) for k, d, o in zip((16, 17, 18), data, lists)]
    p0 = f.P.cpu().numpy().copy()
    got = f.accuracy(lists)
    parts = [f.accuracy([o[a:b] for o in lists]) for a, b in ((0, 3), (3, 11), (11, None))]
    for m in range(3):
        same(got[m], want[m], f"model {m}")
        same(np.concatenate([p[m] for p in parts]), want[m], f"model {m}, three launches")
    same(f.P.cpu().numpy(), p0, "accuracy leaves the parameters alone")
    assert f.steps == [0, 0, 0]


# ---- 5: the epoch loop ----

def test_epoch_loop(data, seeds):
    from preganplus_amd.gobitrain import GOBIFleetTrainer, GOBITrainer
    f = GOBIFleetTrainer(weights=[seeds[16], seeds[17]])
    f.set_data([data[0], data[2]])
    acc = f.train(2, rngs=[random.Random(1), random.Random(2)])
    lone = []
    for m, (k, d) in enumerate(((16, data[0]), (17, data[2]))):
        t = GOBITrainer(weights=seeds[k])
        want = t.train(d[0], d[1], 2, rng=random.Random(m + 1))
        assert acc[m] == want, (m, acc[m], want)
        assert f.orders[m] == t.orders
        assert f.steps[m] == t.step == 2 * int(0.8 * d[0].shape[0])
        for g, w, what in zip(_slot(f, m), _state(t), ("P", "m", "v")):
            same(g, w, f"model {m} {what}")
        lone.append(t)
    # trainer(m) goes on as a checkpoint of model m would
    more = [5, 0, 398, 17]
    t = f.trainer(1)
    same(t.backprop(more), lone[1].backprop(more), "resumed losses")
    for g, w, what in zip(_state(t), _state(lone[1]), ("P", "m", "v")):
        same(g, w, f"resumed {what}")
    ck = f.checkpoint(0, 2, acc[0])
    want = lone[0].checkpoint(2, acc[0])
    assert ck["accuracy_list"] == want["accuracy_list"] and ck["epoch"] == 2
    for k in R.ORDER:
        assert torch.equal(ck["model_state_dict"][k], want["model_state_dict"][k])
        same(f.weights_numpy(0)[k], lone[0].weights_numpy()[k], k)
    for i in range(len(R.ORDER)):
        a, b = ck["optimizer_state_dict"]["state"][i], want["optimizer_state_dict"]["state"][i]
        assert torch.equal(a["exp_avg"], b["exp_avg"]) and torch.equal(a["exp_avg_sq"], b["exp_avg_sq"])
        assert float(a["step"]) == float(b["step"])


# ---- 6, 7, 8: each environment against its own surrogate ----

E = 23


@pytest.fixture(scope="module")
def fleet3(data, seeds):
    """Three surrogates (the packaged one, two trained for 24 steps), 23 inits,
    and per (model, environment) the single-model optimiser's result, with and
    without the 3-step limit and its pre-projection tap."""
    from preganplus_amd.gobi import GOBIOptimizer, load_weights
    ws = [load_weights()[0]]
    for k, d in ((17, data[0]), (18, data[2])):
        t = _single(seeds[k], d)
        t.backprop(_orders(k, (d[0].shape[0],), (24,))[0])
        ws.append(t.weights_numpy())
    inits = np.load(os.path.join(R.GOLD, "gobi_h16.npz"))["inits"][:E].astype(np.float32)
    x = torch.tensor(inits, device="cuda")
    full, lim = {}, {}
    for m, w in enumerate(ws):
        opt = GOBIOptimizer(weights=w)
        for e in range(E):
            full[m, e] = [a.cpu().numpy() for a in opt.optimize(x[e:e + 1])]
            pre = torch.full((1, 16, 16), -3.0, device="cuda")
            lim[m, e] = [a.cpu().numpy() for a in opt.optimize(x[e:e + 1], max_iters=3, pre=pre)] + [pre.cpu().numpy()]
        opt.close()
    return ws, x, full, lim


def _check_env(got, want, e, what):
    for g, w, name in zip(got, want, ("result", "iterations", "fitness", "pre")):
        same(g[e:e + 1], w, f"{what}: environment {e} {name}")


MODEL_OF = np.array([2, 0, 2, 2, 1, 2, 0, 2, 0, 2, 2, 0, 0, 2, 0, 2, 0, 2, 2, 0, 2, 0, 2])


def test_grouped_optimize_bytewise(fleet3):
    from preganplus_amd.gobi import GOBIOptimizer
    ws, x, full, lim = fleet3
    assert MODEL_OF.shape == (E,) and (MODEL_OF == 1).sum() == 1 and (MODEL_OF == 0).sum() == 9
    opt = GOBIOptimizer(weights=ws)
    assert opt.n_models == 3
    perm = np.random.RandomState(2).permutation(E)
    for model_of in (MODEL_OF, MODEL_OF[perm]):
        got = [a.cpu().numpy() for a in opt.optimize(x, model_of=model_of)]
        for e in range(E):
            _check_env(got, full[int(model_of[e]), e], e, "200 iterations")
        pre = torch.full((E, 16, 16), -3.0, device="cuda")
        got = [a.cpu().numpy() for a in opt.optimize(x, model_of=model_of, max_iters=3, pre=pre)] + [pre.cpu().numpy()]
        for e in range(E):
            _check_env(got, lim[int(model_of[e]), e], e, "3 iterations")
    assert len(opt._plans) == 2   # one table per model_of content
    assert any((full[0, e][0] != full[2, e][0]).any() or full[0, e][2] != full[2, e][2] for e in range(E))  # the models differ


def test_inert_table_entries(fleet3):
    """A hand-built table with a -1 model, a model >= M, environments outside
    [0, E) and a duplicate: the valid environments equal their single runs and
    every other row keeps the value it was filled with (the kernel's bounds
    checks are what this verifies)."""
    from preganplus_amd.gobi import GOBIOptimizer
    ws, x, full, _ = fleet3
    opt = GOBIOptimizer(weights=ws)
    table = torch.tensor([[-1, 0, 1, 2, 3],            # no model: the whole group is inert
                          [3, 4, 5, 6, 7],             # model >= M
                          [0, 8, E, 9, 9],             # an environment >= E, and a duplicate of slot 2
                          [1, 10, -5, 2 ** 30, 11],    # far outside on both sides
                          [2, -1, -1, -1, -1]],        # a model with nothing to do
                         dtype=torch.int32, device="cuda")
    valid = {8: 0, 9: 0, 10: 1, 11: 1}
    out = (torch.full((E, 16, 18), -3.0, device="cuda"), torch.full((E,), -9, dtype=torch.int32, device="cuda"),
           torch.full((E,), -3.0, device="cuda"))
    pre = torch.full((E, 16, 16), -3.0, device="cuda")
    opt.optimize(x, out=out, groups=table, pre=pre)
    res, its, fit, pre = [a.cpu().numpy() for a in out + (pre,)]
    for e in range(E):
        if e in valid:
            _check_env((res, its, fit), full[valid[e], e], e, "valid entry")
            assert (pre[e] != -3.0).any()
        else:
            assert (res[e] == -3.0).all() and its[e] == -9 and fit[e] == -3.0 and (pre[e] == -3.0).all(), e


def test_handle_semantics(fleet3, seeds):
    from preganplus_amd.gobi import GOBIOptimizer
    ws, x, full, _ = fleet3
    opt = GOBIOptimizer(weights=ws)
    zero = GOBIOptimizer(weights=ws[0])
    for g, w, name in zip(opt.optimize(x), zero.optimize(x), ("result", "iterations", "fitness")):
        same(g.cpu().numpy(), w.cpu().numpy(), f"pgp_gobi_optimize on the 3-model handle: {name}")
    one = GOBIOptimizer(weights=[ws[1]])   # a one-model create_many is create
    for g, w, name in zip(one.optimize(x[:5]), GOBIOptimizer(weights=ws[1]).optimize(x[:5]), ("r", "i", "f")):
        same(g.cpu().numpy(), w.cpu().numpy(), f"one-model handle: {name}")
    model_of = np.arange(E) % 3
    opt.optimize(x, model_of=model_of)     # plans (and caches) the table before the update
    opt.set_model(1, seeds[16])
    got = [a.cpu().numpy() for a in opt.optimize(x, model_of=model_of)]
    fresh = [a.cpu().numpy() for a in GOBIOptimizer(weights=seeds[16]).optimize(x)]
    for e in range(E):
        if model_of[e] == 1:
            _check_env(got, [a[e:e + 1] for a in fresh], e, "after set_model(1)")
        else:
            _check_env(got, full[int(model_of[e]), e], e, "models 0 and 2 unchanged")
    with pytest.raises(IndexError):
        opt.set_model(3, seeds[16])
    with pytest.raises(ValueError):
        opt.optimize(x, model_of=model_of[:-1])
    with pytest.raises(ValueError):
        opt.optimize(x, model_of=model_of + 1)
