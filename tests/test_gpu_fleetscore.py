"""A fleet's interval finished on the device: accuracy()'s
scores of every cell in one launch inside the tuning graph
(pgp_tune_scores_many, FleetTuner.tune(score="device")) and every cell's
decision in one K5 call (PreGANPlusFleetRecovery(device_finish=True)).  The
reference is always the existing host function or path: train.accuracy_scores,
tune(score=True), the per-cell _recover loop."""
import ctypes
import types

import numpy as np
import pytest
import torch

from preganplus_amd import _native
from preganplus_amd import train as TR
from preganplus_amd import weights as W
from tests.test_fleet_scores_cpu import crafted_cells

pytestmark = pytest.mark.gpu
K = 16
SENT = -7.25          # sentinel for buffers nothing may write
FSENT = -9
GOLD = "tests/golden"


def dev(a, dtype):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def states_of(P):
    """[M,K,2] prototypes -> state slots [M,2K+3] (factor, num_zero, num_ones behind them)."""
    M = P.shape[0]
    return np.concatenate([P.reshape(M, -1), np.tile([0.3, 17.0, 5.0], (M, 1))], axis=1)


def run_raw(H, lg, pr, y, cls, P, active=None, n_protos=None):
    """pgp_tune_scores_many on sentinel-filled outputs -> (rc, scores [M,2], flag [M])."""
    M, n = lg.shape[0], lg.shape[1]
    Kp = P.shape[1] if n_protos is None else n_protos
    t = {"lg": dev(lg, torch.float64), "pr": dev(pr, torch.float64), "y": dev(y, torch.int32),
         "cls": dev(cls, torch.int32), "state": dev(states_of(P), torch.float64)}
    act = None if active is None else dev(active, torch.int32)
    scores = torch.full((M, 2), SENT, dtype=torch.float64, device="cuda")
    flag = torch.full((M,), FSENT, dtype=torch.int32, device="cuda")
    rc = _native.lib().pgp_tune_scores_many(
        H, Kp, M, n, None if act is None else act.data_ptr(), t["lg"].data_ptr(), t["pr"].data_ptr(),
        t["y"].data_ptr(), t["cls"].data_ptr(), t["state"].data_ptr(), scores.data_ptr(), flag.data_ptr(), None)
    torch.cuda.synchronize()
    return rc, scores.cpu().numpy(), flag.cpu().numpy()


def check_against_host(lg, pr, y, cls, P, scores, flag, cells):
    """Every listed cell's row against accuracy_scores on the same arrays, byte for byte."""
    for m in cells:
        try:
            want = TR.accuracy_scores(lg[m], pr[m], y[m], cls[m], P[m])
        except ZeroDivisionError:
            assert flag[m] == 1, m
            assert scores[m, 1] == SENT, m             # left unwritten
        else:
            assert flag[m] == 0, m
            assert scores[m].tobytes() == np.array(want, dtype=np.float64).tobytes(), (m, scores[m], want)


def random_cells(H, M, n, seed):
    r = np.random.default_rng(seed)
    lg = r.normal(size=(M, n, H, 2))
    pr = r.uniform(0, 1, (M, n, H, 2))
    y = (r.uniform(size=(M, n, H)) < 0.3).astype(np.int32)
    cls = r.integers(-1, 5, (M, n, H)).astype(np.int32)
    P = r.uniform(0.1, 0.9, (M, K, 2))
    return lg, pr, y, cls, P


# ---- 1. the raw entry ----

@pytest.mark.parametrize("H", [8, 16])
def test_raw_entry_equals_accuracy_scores(H):
    lg, pr, y, cls, P = crafted_cells(H, n=4)
    rc, scores, flag = run_raw(H, lg, pr, y, cls, P, active=[1, 0, 1])
    assert rc == 0
    assert (scores[1] == SENT).all() and flag[1] == FSENT          # the inactive cell's rows: untouched
    check_against_host(lg, pr, y, cls, P, scores, flag, [0, 2])
    assert flag.tolist() == [0, FSENT, 1]
    # and with every cell active (active = NULL)
    rc, scores, flag = run_raw(H, lg, pr, y, cls, P)
    assert rc == 0 and flag.tolist() == [0, 0, 1]
    check_against_host(lg, pr, y, cls, P, scores, flag, range(3))


@pytest.mark.parametrize("H", [8, 16])
def test_one_window(H):
    lg, pr, y, cls, P = random_cells(H, 4, 1, seed=30 + H)
    y[0, 0, 0] = 1
    y[1] = 0
    rc, scores, flag = run_raw(H, lg, pr, y, cls, P)
    assert rc == 0 and flag[0] == 0 and flag[1] == 1
    check_against_host(lg, pr, y, cls, P, scores, flag, range(4))


def test_grid_size():
    """The same cell as slot 0 of 1, slot 2 of 3 and the last of 600 (more cells than are resident at once)."""
    H, n = 16, 4
    lg, pr, y, cls, P = random_cells(H, 600, n, seed=77)
    y[5] = 0
    y[:, 0, 1] |= (np.arange(600) != 5)
    one = [a[599:600] for a in (lg, pr, y, cls, P)]
    rc, s1, f1 = run_raw(H, *one)
    assert rc == 0
    check_against_host(*one, s1, f1, [0])
    three = [np.concatenate([a[:2], a[599:600]]) for a in (lg, pr, y, cls, P)]
    rc, s3, f3 = run_raw(H, *three)
    assert rc == 0
    check_against_host(*three, s3, f3, range(3))
    rc, s600, f600 = run_raw(H, lg, pr, y, cls, P)
    assert rc == 0
    check_against_host(lg, pr, y, cls, P, s600, f600, range(600))
    assert f600.sum() == 1 and f600[5] == 1
    assert s1[0].tobytes() == s3[2].tobytes() == s600[599].tobytes()


def test_argument_errors_launch_nothing():
    H, M, n = 16, 2, 3
    L = _native.lib()
    lg, pr, y, cls, P = random_cells(H, M, n, seed=3)
    t = {"lg": dev(lg, torch.float64), "pr": dev(pr, torch.float64), "y": dev(y, torch.int32),
         "cls": dev(cls, torch.int32), "state": dev(states_of(P), torch.float64)}
    scores = torch.full((M, 2), SENT, dtype=torch.float64, device="cuda")
    flag = torch.full((M,), FSENT, dtype=torch.int32, device="cuda")
    names = ("lg", "pr", "y", "cls", "state", "scores", "flag")

    def call(H_=H, K_=K, M_=M, n_=n, null=None):
        p = {k: v.data_ptr() for k, v in t.items()}
        p["scores"], p["flag"] = scores.data_ptr(), flag.data_ptr()
        if null:
            p[null] = None
        return L.pgp_tune_scores_many(H_, K_, M_, n_, None, *[p[k] for k in names], None)

    UNSUPPORTED, ARG = -2, -1
    for h in (4, 32, 50, 64):
        assert call(H_=h) == UNSUPPORTED
        assert call(H_=h, M_=0) == UNSUPPORTED
    assert call(M_=-1) == ARG
    assert call(n_=-1) == ARG
    assert call(M_=0, n_=-1) == ARG
    assert call(n_=0) == ARG
    assert call(K_=2) == ARG
    for k in names:
        assert call(null=k) == ARG, k
    assert L.pgp_last_error()
    assert call(M_=0) == 0 and call(M_=0, n_=0) == 0
    assert L.pgp_tune_scores_many(H, K, 0, n, None, None, None, None, None, None, None, None, None) == 0
    torch.cuda.synchronize()
    assert (scores.cpu().numpy() == SENT).all() and (flag.cpu().numpy() == FSENT).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert (flag.cpu().numpy() == 0).all()


# ---- 2. FleetTuner.tune(score="device") against tune(score=True) ----

def cell_weights(H, seed):
    w = W.synth_weights(H, seed=seed)
    w["prototypes"] = np.random.default_rng(100 + seed).uniform(0.1, 0.9, (K, 2))
    return w


def tune_data(H, M, n, seed, no_positive=()):
    r = np.random.default_rng(seed)
    wins = r.uniform(0, 1, (M, n, 3, 3 * H)).astype(np.float32)
    anom = (r.uniform(size=(M, n, H)) < 0.25).astype(np.int32)
    anom[:, 0, 1] = 1
    for m in no_positive:
        anom[m] = 0
    cls = r.integers(0, 3, (M, n, H)).astype(np.int32)
    return wins, anom, cls


def same_tuners(a, b, what):
    torch.cuda.synchronize()
    for k in ("P", "m", "v", "state_dev"):
        assert getattr(a, k).cpu().numpy().tobytes() == getattr(b, k).cpu().numpy().tobytes(), f"{what}: {k}"
    for m in range(a.M):
        assert a.states[m].vector().tobytes() == b.states[m].vector().tobytes(), f"{what}: state {m}"
    assert a.sched.steps.tobytes() == b.sched.steps.tobytes()
    assert a.tune_errors.keys() == b.tune_errors.keys()
    for c in a.tune_errors:
        ea, eb = a.tune_errors[c], b.tune_errors[c]
        assert type(ea) is type(eb) and ea.args == eb.args, f"{what}: error of cell {c}"
        assert eb.__traceback__ is None


@pytest.mark.parametrize("H", [8, 16])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_device_scores_equal_host_scores(H, p):
    M, n = 3, 3
    ws = [cell_weights(H, 40 + m) for m in range(M)]
    kw = dict(dropout=p, dropout_seeds=[11, 12, 13] if p else None)
    a, b, c = (TR.FleetTuner(H, ws, **kw) for _ in range(3))
    for call in range(2):
        wins, anom, cls = tune_data(H, M, n, seed=60 + call, no_positive=(2,))
        act = np.array([1, 0, 1], dtype=bool) if call == 0 else np.array([1, 1, 1], dtype=bool)
        ra = a.tune(wins, anom, cls, act, score=True)
        rb = b.tune(wins, anom, cls, act, score="device")
        assert ra == rb, f"call {call}"
        assert rb[2][1] is None and type(b.tune_errors[2]) is ZeroDivisionError
        assert (ra[1] is None) == (call == 0)
        for m in np.flatnonzero(act):                   # == on tuples is not bytes: -0.0, and the floats' types
            assert all(type(x) is float for row in rb[m][0] for x in row)
            assert np.array(ra[m][0]).tobytes() == np.array(rb[m][0]).tobytes()
            if ra[m][1] is not None:
                assert type(rb[m][1]) is tuple and all(type(x) is float for x in rb[m][1])
                assert np.array(ra[m][1]).tobytes() == np.array(rb[m][1]).tobytes()
        same_tuners(a, b, f"call {call}")
        # the eager issue of the same launches, byte for byte the captured graph's download
        g = c.graph(n, "device", capture=False)
        assert g.graph is None
        an, cl, ac = c.stage(g, wins, anom, cls, act)
        g.din.copy_(g.hin, non_blocking=True)
        g.issue(c)
        g.hout.copy_(g.down, non_blocking=True)
        torch.cuda.synchronize()
        gb = b.graph(n, "device")
        assert g.hout.numpy().tobytes() == gb.hout.numpy().tobytes(), f"call {call}: eager != graph"
        assert g.hout.numel() == 2 * n * M + M * (2 * K + 3) + 2 * M + (M + 1) // 2      # loss|state|scores|flags
        rc = c.results(g, g.hout.numpy(), an, cl, ac)
        assert rc == rb
        same_tuners(b, c, f"call {call} eager")
    assert b.graph(n, True) is not b.graph(n, "device")
    with pytest.raises(ValueError):
        b.graph(n, "host")


# ---- 3. the fleet plugin with device_finish ----

def _snap(ft, m):
    torch.cuda.synchronize()
    return (ft.P[m].cpu().numpy().tobytes(), ft.m[m].cpu().numpy().tobytes(), ft.v[m].cpu().numpy().tobytes(),
            ft.states[m].vector().tobytes(), ft.sched.steps[m].tobytes(), ft.state_dev[m].cpu().numpy().tobytes())


def _same_entries(a, b, what):
    assert len(a) == len(b)
    for m, (x, y) in enumerate(zip(a, b)):
        if isinstance(x, BaseException) or isinstance(y, BaseException):
            assert type(x) is type(y) and x.args == y.args, f"{what}: cell {m}"
        else:
            assert x == y and type(x) is type(y), f"{what}: cell {m}"


def test_fleet_plugin_device_finish_equals_host_finish():
    from preganplus_amd.recovery import PreGANPlusFleetRecovery
    from tests.test_train_oracle_golden import fake_env
    H, M = 16, 3
    w, extra = W.load_npz("preganplus_amd/data/simulator_16.npz")
    z = np.load(f"{GOLD}/plugin_h16.npz")
    tt = extra["train_time_data"]

    def forced(w, label):
        """w with an anomaly decoder that answers `label` on every host whatever the window."""
        t = dict(w["transformer"])
        t["anomaly_decoder.0.weight"] = np.zeros_like(np.asarray(t["anomaly_decoder.0.weight"]))
        bias = np.zeros(2 * H)
        bias[label::2] = 2.0
        t["anomaly_decoder.0.bias"] = bias
        return dict(w, transformer=t)

    # cell 0: the recorded plugin; cell 1: never an anomaly; cell 2: always one, on a constant series (no label)
    weights = [w, forced(w, 0), forced(w, 1)]
    extras = [extra, extra, {"train_time_data": tt}]
    host = PreGANPlusFleetRecovery(H, weights, extras, training=True)
    devf = PreGANPlusFleetRecovery(H, weights, extras, training=True, device_finish=True)
    assert host.device_finish is False and devf.device_finish is True

    def envs_of(step):
        envs = [fake_env(z, (step + m) % 4, tt, z["schedule_series"]) for m in range(M)]
        rows = np.asarray(envs[2].stats.time_series)
        envs[2].stats.time_series = np.repeat(rows[-1:], rows.shape[0], axis=0)
        return envs

    for i in range(3):
        decisions = [[tuple(x) for x in z[f"s{(i + m) % 4}/decision_in"]] for m in range(M)]
        host.setEnvironments(envs_of(i))
        devf.setEnvironments(envs_of(i))
        want = host.run_model(decisions)
        got = devf.run_model(decisions)
        _same_entries(got, want, f"interval {i}")
        assert got[1] is decisions[1]                                   # no anomaly: the original decision
        assert type(got[2]) is ZeroDivisionError                        # no positive label
        assert isinstance(got[0], list)
        assert devf.hosts_from == host.hosts_from
        assert devf.classes == host.classes
        assert devf.epoch == host.epoch
        for m in range(M):
            assert len(devf.accuracy_list[m]) == len(host.accuracy_list[m])
            for x, y in zip(devf.accuracy_list[m], host.accuracy_list[m]):
                assert np.asarray(x, dtype=np.float64).tobytes() == np.asarray(y, dtype=np.float64).tobytes(), (i, m)
            assert _snap(devf.tuner, m) == _snap(host.tuner, m), f"interval {i}: slot {m}"
    assert len(host.accuracy_list[0]) > len(W.accuracy_list_from_arrays(extra, "meta/gen/accuracy_list"))


class _Container:
    def __init__(self, cid, host):
        self.id, self._h = cid, host

    def getHostID(self):
        return self._h


def test_batched_decisions_equal_per_cell_recover():
    """200 random placements at H = 16 in one K5 call (the plugin's _recover_many on a stand-in with the
    fields it reads) against 200 batch-1 _recover calls: unplaced containers, None entries, both gates."""
    from preganplus_amd import recovery as R
    H, M = 16, 200
    r = np.random.default_rng(2024)
    envs, originals, probs = [], [], np.zeros((M, 2), dtype=np.float32)
    for m in range(M):
        cl = []
        for c in range(H):
            u = r.uniform()
            cl.append(None if u < 0.1 else _Container(c, -1 if u < 0.25 else int(r.integers(0, H))))
        envs.append(types.SimpleNamespace(containerlist=cl))
        originals.append([(int(c), int(r.integers(0, H))) for c in r.permutation(H)[:int(r.integers(0, 6))]])
        probs[m] = (0.7, 0.3) if r.uniform() < 0.3 else (0.2, 0.8)
    probs[7] = (0.5, 0.5)                                               # a tie decides (p[0] > p[1] is False)
    final_target = r.integers(0, H, (M, H)).astype(np.int32)
    cells = [m for m in range(M) if m % 10 != 3]                        # the others: inactive
    errors = {15: ZeroDivisionError("division by zero")}
    device = torch.device("cuda", torch.cuda.current_device())

    fleet = types.SimpleNamespace(M=M, hosts=H, device=device, _rio_many=None, envs=envs,
                                  tuner=types.SimpleNamespace(gan_probs_after=probs), hosts_from=[None] * M)
    res = [errors.get(m, originals[m]) for m in range(M)]
    R.PreGANPlusFleetRecovery._recover_many(fleet, cells, res, originals, final_target)

    io = R._RecoverIO(H, device)
    n_keep = n_moved = 0
    for m in range(M):
        if m not in cells or m in errors:
            assert res[m] is errors.get(m, originals[m]) and fleet.hosts_from[m] is None
            continue
        keep = bool(probs[m][0] > probs[m][1])
        want, hf = R._recover(envs[m], H, None, originals[m], keep, device, final_target[m].tolist(), io=io)
        assert res[m] == want, m
        if keep:
            assert res[m] is originals[m] and fleet.hosts_from[m] is None
            n_keep += 1
        else:
            assert fleet.hosts_from[m] == hf and all(type(v) is int for v in fleet.hosts_from[m])
            n_moved += any(hf)
    assert n_keep > 20 and n_moved > 60
