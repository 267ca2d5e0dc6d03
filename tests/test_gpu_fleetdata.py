"""A fleet's tuning datasets built on the device: pgp_tune_dataset_cells against
the host functions and against pgp_tune_dataset called per cell, FleetTuner.dataset +
tune_launch(inputs="device") against tune_launch on host arrays, and the fleet plugin with
device_dataset=True against the default.  Every equality is on bytes."""
import numpy as np
import pytest
import torch

from preganplus_amd import _native
from preganplus_amd import train as TR
from preganplus_amd import weights as W
from tests.test_fleetdata_host import fleet_case, per_cell
from tests.test_gpu_fleetscore import _same_entries, _snap, cell_weights, same_tuners

pytestmark = pytest.mark.gpu
SENT, ISENT = -7.25, -9          # sentinels for buffers nothing may write
GOLD = "tests/golden"
NAMES = ("windows", "y", "cls", "positive", "infer")


def dev(a, dtype):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def run_raw(H, series, tmax, active=None, positive=True, infer=True):
    """pgp_tune_dataset_cells on sentinel-filled outputs -> {name: array}."""
    M, n = series.shape[:2]
    s, t = dev(series, torch.float64), dev(tmax, torch.float64)
    act = None if active is None else dev(active, torch.int32)
    f = lambda shp: torch.full(shp, SENT, dtype=torch.float32, device="cuda")
    i = lambda shp: torch.full(shp, ISENT, dtype=torch.int32, device="cuda")
    o = {"windows": f((M, n, 3, 3 * H)), "y": i((M, n, H)), "cls": i((M, n, H)), "positive": i((M, n)),
         "infer": f((M, 3, 3 * H))}
    rc = _native.lib().pgp_tune_dataset_cells(
        H, M, n, None if act is None else act.data_ptr(), s.data_ptr(), t.data_ptr(), o["windows"].data_ptr(),
        o["y"].data_ptr(), o["cls"].data_ptr(), o["positive"].data_ptr() if positive else None,
        o["infer"].data_ptr() if infer else None, None)
    torch.cuda.synchronize()
    assert rc == 0
    return {k: v.cpu().numpy() for k, v in o.items()}


def run_lone(H, series, tmax):
    """pgp_tune_dataset once per cell with that cell's train_max -> (windows, y, cls, infer) stacked."""
    M, n = series.shape[:2]
    out = []
    for m in range(M):
        s, t = dev(series[m:m + 1], torch.float64), dev(tmax[m], torch.float64)
        w = torch.full((n, 3, 3 * H), SENT, dtype=torch.float32, device="cuda")
        y, c = (torch.full((n, H), ISENT, dtype=torch.int32, device="cuda") for _ in range(2))
        inf = torch.full((3, 3 * H), SENT, dtype=torch.float32, device="cuda")
        _native.check(_native.lib().pgp_tune_dataset(H, 1, n, s.data_ptr(), t.data_ptr(), w.data_ptr(), y.data_ptr(),
                                                     c.data_ptr(), inf.data_ptr(), None), "pgp_tune_dataset")
        torch.cuda.synchronize()
        out.append([a.cpu().numpy() for a in (w, y, c, inf)])
    return [np.stack(a) for a in zip(*out)]


def same(got, want, cells, what=""):
    """The listed cells' rows of every output, byte for byte."""
    for k, w in zip(NAMES, want):
        for m in cells:
            assert got[k][m].dtype == w[m].dtype and got[k][m].tobytes() == w[m].tobytes(), (what, k, m)


def untouched(got, cells, skip=()):
    for k in NAMES:
        if k not in skip:
            for m in cells:
                assert (got[k][m] == (SENT if got[k].dtype == np.float32 else ISENT)).all(), (k, m)


# ---- 1. the raw entry ----

@pytest.mark.parametrize("H,M,n",
                         [(8, 5, 10), (16, 3, 10), (50, 3, 10), (16, 4, 16), (8, 3, 1), (16, 3, 2), (50, 2, 3)])
def test_raw_entry_bit_exact(H, M, n):
    series, trains, tmax = fleet_case(H, M, n)
    want = per_cell(series, trains)                      # the host functions (and oracle.inference_window)
    got = run_raw(H, series, tmax)                       # active = NULL
    same(got, want, range(M), "host")
    lw, ly, lc, li = run_lone(H, series, tmax)           # the lone entry, one cell at a time
    same(got, (lw, ly, lc, ly.any(axis=2).astype(np.int32), li), range(M), "pgp_tune_dataset")
    ones = run_raw(H, series, tmax, active=np.ones(M, dtype=np.int32))
    assert all(ones[k].tobytes() == got[k].tobytes() for k in NAMES)


def test_inactive_cell_in_a_shared_workgroup():
    H, M, n = 8, 3, 10                                   # the three cells share a workgroup
    series, trains, tmax = fleet_case(H, M, n)
    want = per_cell(series, trains)
    series[1] = np.nan                                   # its inputs are not used either
    got = run_raw(H, series, tmax, active=[1, 0, 1])
    untouched(got, [1])
    same(got, want, [0, 2])


def test_optional_outputs():
    H, M, n = 16, 3, 10
    series, trains, tmax = fleet_case(H, M, n)
    full = run_raw(H, series, tmax)
    for off in ("positive", "infer"):
        got = run_raw(H, series, tmax, **{off: False})
        untouched(got, range(M), skip=[k for k in NAMES if k != off])
        assert all(got[k].tobytes() == full[k].tobytes() for k in NAMES if k != off), off


def test_one_active_cell_at_any_grid_size():
    """The same cell alone, as slot 2 of 3 and as the last of 600 (150 workgroups), the others inactive."""
    H, n = 16, 10
    series, trains, tmax = fleet_case(H, 3, n)
    want = per_cell(series[2:], trains[2:])
    got = run_raw(H, series[2:], tmax[2:], active=[1])
    same(got, want, [0])
    got = run_raw(H, series, tmax, active=[0, 0, 1])
    same(got, [np.concatenate([w] * 3) for w in want], [2])
    untouched(got, [0, 1])
    big, bmax = np.tile(series[:1], (600, 1, 1)), np.tile(tmax[:1], (600, 1))
    big[599], bmax[599] = series[2], tmax[2]
    act = np.zeros(600, dtype=np.int32)
    act[599] = 1
    got = run_raw(H, big, bmax, active=act)
    for k, w in zip(NAMES, want):
        assert got[k][599].tobytes() == w[0].tobytes(), k
    untouched(got, range(599))                           # every other slot of the 600


@pytest.mark.parametrize("H", [8, 16, 50])
def test_positive_is_any_label_of_the_row(H):
    M, n = 3, 10
    series, trains, tmax = fleet_case(H, M, n)
    y = per_cell(series, trains)[1]
    rows = y.any(axis=2)
    assert rows.any() and not rows.all()                 # of the inputs: a row with a positive label, a row without
    got = run_raw(H, series, tmax)
    assert got["positive"].tobytes() == got["y"].any(axis=2).astype(np.int32).tobytes()
    assert got["positive"].tobytes() == rows.astype(np.int32).tobytes()


# ---- 2. tune_launch(inputs="device") against tune_launch on host arrays ----

@pytest.mark.parametrize("H", [8, 16])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("score", [True, "device"])
def test_tune_launch_device_inputs_equal_host_inputs(H, p, score):
    M, n = 4, 3
    ws = [cell_weights(H, 40 + m) for m in range(M)]
    kw = dict(dropout=p, dropout_seeds=[11, 12, 13, 14] if p else None)
    a, b, c = (TR.FleetTuner(H, ws, **kw) for _ in range(3))
    for call in range(2):
        series, trains, tmax = fleet_case(H, M, n, seed=call)
        wins, y, cls, pos, inf = TR.on_the_fly_dataset_many(series, tmax)
        assert not pos[0].any() and pos[2].any() and pos[3].any()  # cell 0 (constant rows) has no positive label
        act = np.array([1, 1, 0, 1], dtype=bool) if call == 0 else np.ones(M, dtype=bool)
        ra = a.tune_launch(wins, y, cls, act, score=score)()
        d = b.dataset(n, series, tmax, None, score)
        torch.cuda.synchronize()
        assert (d.y.tobytes(), d.cls.tobytes(), d.positive.tobytes()) == (y.tobytes(), cls.tobytes(), pos.tobytes())
        assert b.infer_windows.cpu().numpy().tobytes() == inf.tobytes()
        gb = b.graph(n, score)
        assert gb.W.cpu().numpy().tobytes() == wins.tobytes()
        labels = (d.y, d.cls) if call == 0 else (d.y, d.cls, d.positive)      # with and without the kernel's flags
        rb = b.tune_launch(None, None, None, act, score=score, inputs="device", labels=labels)()
        assert ra == rb, f"call {call}"
        assert rb[0][1] is None and type(b.tune_errors[0]) is ZeroDivisionError
        assert (ra[2] is None) == (call == 0)
        for m in np.flatnonzero(act):
            assert np.array(ra[m][0]).tobytes() == np.array(rb[m][0]).tobytes()
            if ra[m][1] is not None:
                assert np.array(ra[m][1]).tobytes() == np.array(rb[m][1]).tobytes()
        same_tuners(a, b, f"call {call}")
        # the eager issue of the same launches, byte for byte the captured graph's download
        dc = c.dataset(n, series, tmax, None, score, capture=False)
        g = c.graph(n, score, capture=False)
        assert g.graph is None
        torch.cuda.synchronize()
        an, cl, ac = c.stage(g, None, dc.y, dc.cls, act, device_inputs=True)
        o = g.span["sched"][0]
        assert o >= g.span["C"][1] > 0                              # the windows and labels are not uploaded
        g.din[o:].copy_(g.hin[o:], non_blocking=True)
        g.issue(c)
        g.hout.copy_(g.down, non_blocking=True)
        torch.cuda.synchronize()
        assert g.hout.numpy().tobytes() == gb.hout.numpy().tobytes(), f"call {call}: eager != graph"
        assert c.results(g, g.hout.numpy(), an, cl, ac) == rb
        same_tuners(b, c, f"call {call} eager")
    with pytest.raises(ValueError):
        b.tune_launch(None, None, None, inputs="device")
    with pytest.raises(ValueError):
        b.tune_launch(wins, y, cls, inputs="pinned")


# ---- 3. the fleet plugin with device_dataset ----

@pytest.mark.parametrize("device_finish", [False, True])
def test_fleet_plugin_device_dataset_equals_default(device_finish):
    from preganplus_amd.recovery import PreGANPlusFleetRecovery
    from tests.test_train_oracle_golden import fake_env
    H, M = 16, 5
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

    # cell 0: the recorded plugin; 1: never an anomaly; 2: always one, on a constant series of 5 rows (no label);
    # 3 / 4: always one, on the last 1 / 2 rows, cell 4 on a training series of its own
    weights = [w, forced(w, 0), forced(w, 1), forced(w, 1), forced(w, 1)]
    extras = [extra, extra, {"train_time_data": tt}, {"train_time_data": tt}, {"train_time_data": tt * 2.0}]
    ref = PreGANPlusFleetRecovery(H, weights, extras, training=True, device_finish=device_finish)
    new = PreGANPlusFleetRecovery(H, weights, extras, training=True, device_finish=device_finish, device_dataset=True)
    assert ref.device_dataset is False and new.device_dataset is True and new.device_finish is device_finish
    assert PreGANPlusFleetRecovery.__init__.__defaults__[-1] is False

    def envs_of(step):
        envs = [fake_env(z, (step + m) % 4, tt, z["schedule_series"]) for m in range(M)]
        rows = np.asarray(envs[2].stats.time_series)
        envs[2].stats.time_series = np.repeat(rows[-1:], 5, axis=0)
        envs[3].stats.time_series = np.asarray(envs[3].stats.time_series)[-1:]
        envs[4].stats.time_series = [r for r in np.asarray(envs[4].stats.time_series)[-2:]]   # a list of rows
        return envs

    for i in range(3):
        decisions = [[tuple(x) for x in z[f"s{(i + m) % 4}/decision_in"]] for m in range(M)]
        ref.setEnvironments(envs_of(i))
        new.setEnvironments(envs_of(i))
        want = ref.run_model(decisions)
        got = new.run_model(decisions)
        assert sorted(set(new._rows)) == [1, 2, 5, 10]                  # three short length groups and the full one
        _same_entries(got, want, f"interval {i}")
        assert got[1] is decisions[1]                                   # no anomaly: the original decision
        assert type(got[2]) is ZeroDivisionError and type(got[3]) is ZeroDivisionError     # no positive label
        assert isinstance(got[0], list) and isinstance(got[4], list)
        assert new.hosts_from == ref.hosts_from
        assert new.classes == ref.classes
        assert new.epoch == ref.epoch
        for m in range(M):
            assert len(new.accuracy_list[m]) == len(ref.accuracy_list[m])
            for x, y in zip(new.accuracy_list[m], ref.accuracy_list[m]):
                assert np.asarray(x, dtype=np.float64).tobytes() == np.asarray(y, dtype=np.float64).tobytes(), (i, m)
            assert _snap(new.tuner, m) == _snap(ref.tuner, m), f"interval {i}: slot {m}"
    assert len(ref.accuracy_list[0]) > len(W.accuracy_list_from_arrays(extra, "meta/gen/accuracy_list"))
