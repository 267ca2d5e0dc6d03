"""GPU tests of train-mode dropout in the fused batch-1 tuning step
(``pgp_tune_step1_dropout`` / ``pgp_tune_dropout_masks``, pgp_tune1.hip;
DESIGN.md §19), through the C-ABI, ``Trainer`` and the plugin: the masks are the
restated Philox masks byte for byte, p = 0 is the old step bit for bit, the
gradients match fp64 autograd with the masks inserted, the step is
reproducible, the captured graph equals the host loop, and the plugin trains
with it."""
import math

import numpy as np
import pytest
import torch

from preganplus_amd import weights as W
from tests import dropout_ref as DR

pytestmark = pytest.mark.gpu
GOLD = "tests/golden"
SEEDS, STEPS = DR.TEST_SEEDS, DR.TEST_STEPS


def load16():
    return W.load_npz("preganplus_amd/data/simulator_16.npz")


def close(got, want, rel, abs_scale, what=""):
    """fp32 HIP vs fp64 reference: |got - want| <= rel*|want| + abs_scale*max|want|."""
    want = np.asarray(want, dtype=np.float64)
    got = np.asarray(got, dtype=np.float64)
    tol = rel * np.abs(want) + abs_scale * (np.abs(want).max() + 1e-30)
    bad = np.abs(got - want) > tol
    assert not bad.any(), f"{what}: {bad.sum()} of {bad.size} off, max err {np.abs(got - want).max():.3e}"


def _trainer(H, **kw):
    from preganplus_amd import train as TR
    return TR.Trainer(H, W.synth_weights(H, seed=3), max_batch=1, **kw)


@pytest.mark.parametrize("H", [8, 16])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_mask_tap_equals_restatement(H, p):
    tr = _trainer(H, dropout=p, dropout_seed=SEEDS[0])
    assert int(tr._L.pgp_tune_dropout_mask_len(H)) == sum(DR.site_counts(H)) == {8: 4320, 16: 10560}[H]
    assert int(tr._L.pgp_tune_dropout_mask_len(50)) == 0
    for seed in SEEDS:
        tr.dropout_seed = seed
        for base, step in STEPS:
            tr.set_dropout_base(base)
            got = tr.dropout_masks(step=step).cpu().numpy()
            want = DR.keep_masks(H, p, seed, base + step)
            assert got.dtype == np.uint8 and np.array_equal(got, want), (seed, base, step)
            if H == 16 and p == 0.1:
                assert abs(int((got == 0).sum()) - 1056) <= 154
    # the optimizer step is base + step, however it is split
    tr.set_dropout_base(1)
    a = tr.dropout_masks(step=0)
    tr.set_dropout_base(0)
    assert torch.equal(a, tr.dropout_masks(step=1))


def _case(H, seed=0, force_positive=True):
    """A spiky window, labels with at least one positive, classes, a fixed state."""
    x, y, _, _ = DR.spiky_case(H, seed)
    y = y[0].copy()
    if force_positive:
        y[1] = 1
    c = np.random.default_rng(seed).integers(0, 3, H).astype(np.int32)
    protos0 = np.random.default_rng(seed + 1).uniform(0.1, 0.9, (H, 2))
    return x[0], y.astype(np.int32), c, protos0


def _run_step(tr, x, y, c, protos0, step=0, entry=None):
    """One fused step on a fresh state; returns every output as numpy."""
    from preganplus_amd import train as TR
    dev = tr.device
    st = TR.TuneState(protos0, 0.2)
    st.num_zero, st.num_ones = 7, 3
    state = st.to_device(dev)
    loss = torch.zeros(2, dtype=torch.float64, device=dev)
    win = torch.tensor(x, dtype=torch.float32, device=dev)
    yd, cd = torch.from_numpy(y).to(dev), torch.from_numpy(c).to(dev)
    end = tr.sec_end["transformer"]
    tr.G[:end].fill_(float("nan"))          # every transformer entry must be written
    if entry is None:
        tr.tune_step1(win, yd, cd, state, loss, step=step)
    else:
        entry(win, yd, cd, state, loss)
    torch.cuda.synchronize()
    return {"G": tr.G[:end].cpu().numpy(), "logits": tr.logits[0].cpu().numpy(), "protos": tr.protos[0].cpu().numpy(),
            "loss": loss.cpu().numpy(), "state": state.cpu().numpy()}


@pytest.mark.parametrize("H", [8, 16])
def test_p0_through_the_dropout_entry_is_the_old_step(H):
    from preganplus_amd import _native
    from preganplus_amd import train as TR
    tr = _trainer(H)
    x, y, c, protos0 = _case(H)
    old = _run_step(tr, x, y, c, protos0)

    def entry(win, yd, cd, state, loss):
        K = (state.numel() - 3) // 2
        _native.check(tr._L.pgp_tune_step1_dropout(
            H, K, win.data_ptr(), yd.data_ptr(), cd.data_ptr(), tr.P.data_ptr(), tr.G.data_ptr(), state.data_ptr(),
            TR.PROTO_UPDATE_MIN, TR.PROTO_FACTOR_DECAY, tr.logits.data_ptr(), tr.protos.data_ptr(), loss.data_ptr(),
            0.0, tr.drop_rng.data_ptr(), 3, tr._stream()), "pgp_tune_step1_dropout")

    new = _run_step(tr, x, y, c, protos0, entry=entry)
    for k in old:
        assert old[k].tobytes() == new[k].tobytes(), k
    assert not np.isnan(old["G"]).any()


def test_dropout_entry_rejects_bad_arguments():
    from preganplus_amd import _native
    from preganplus_amd import train as TR
    tr = _trainer(8)
    x, y, c, protos0 = _case(8)
    for p in (1.0, -0.1, float("nan")):      # PGP_ERR_ARG from the C-ABI itself
        with pytest.raises(_native.NativeError):
            tr.dropout_masks(p=p)
    tr.dropout = 1.0                         # past the constructor's own check, to reach the step entry's
    with pytest.raises(_native.NativeError):
        _run_step(tr, x, y, c, protos0)
    with pytest.raises(ValueError):
        TR.Trainer(8, W.synth_weights(8, seed=3), max_batch=1, dropout=1.0)


@pytest.mark.parametrize("H", [8, 16])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_step_matches_autograd_with_the_masks(H, p):
    from preganplus_amd import train as TR
    w = W.synth_weights(H, seed=3)
    seed, base, step = SEEDS[1], 40, 2
    tr = TR.Trainer(H, w, max_batch=1, dropout=p, dropout_seed=seed)
    tr.set_dropout_base(base)
    x, y, c, protos0 = _case(H)
    assert (y > 0).any()
    out = _run_step(tr, x, y, c, protos0, step=step)
    keep = tr.dropout_masks(step=step).cpu().numpy()
    assert np.array_equal(keep, DR.keep_masks(H, p, seed, base + step))
    # the kernel's bookkeeping == the numpy restatement on the kernel's own outputs
    st_h = TR.TuneState(protos0, 0.2)
    st_h.num_zero, st_h.num_ones = 7, 3
    mult, tgt, a_h, l_h = TR.loss_targets(out["logits"], out["protos"], y, c, st_h)
    np.testing.assert_allclose(out["loss"], [a_h, l_h], rtol=1e-12, atol=1e-12)
    np.testing.assert_array_equal(out["state"], st_h.vector())
    mult = np.asarray(mult, np.float32).astype(np.float64)
    tgt = np.asarray(tgt, np.float32).astype(np.float64)
    tw, logits, protos = DR.autograd_drop(w, x[None], y[None], mult[None], tgt[None],
                                          DR.split_masks(keep, H), DR.keep_scale(p))
    close(out["logits"], logits[0], rel=1e-4, abs_scale=1e-5, what="logits")
    close(out["protos"], protos[0], rel=1e-4, abs_scale=1e-5, what="protos")
    # the p = 0 step on the same inputs: some gradient must move by more than the tolerance
    g0 = _run_step(TR.Trainer(H, w, max_batch=1), x, y, c, protos0)["G"]
    moved = []
    for t in tr.tensors:
        if t["section"] != "transformer":
            continue
        seg = out["G"][t["offset"]:t["offset"] + t["n"]]
        if not t["trainable"]:
            assert np.all(seg == 0), t["name"]
            continue
        gr = tw[t["name"]].grad
        ref = np.zeros(t["n"]) if gr is None else gr.numpy().reshape(-1)
        worst = DR.ratio_to_tolerance(DR.drop_key_bias(t["name"], seg, H), DR.drop_key_bias(t["name"], ref, H),
                                      1e-3, 1e-4)
        print(f"H={H} p={p} {t['name']}: error / tolerance {worst:.4f}")
        close(DR.drop_key_bias(t["name"], seg, H), DR.drop_key_bias(t["name"], ref, H), rel=1e-3, abs_scale=1e-4,
              what=t["name"])
        z = g0[t["offset"]:t["offset"] + t["n"]]
        if DR.ratio_to_tolerance(DR.drop_key_bias(t["name"], seg, H), DR.drop_key_bias(t["name"], z, H),
                                 1e-3, 1e-4) > 1.0:
            moved.append(t["name"])
    assert moved, "the masks changed no gradient"


def test_dropout_step_is_reproducible_and_advances():
    H = 16
    tr = _trainer(H, dropout=0.1, dropout_seed=SEEDS[0])
    tr.set_dropout_base(9)
    x, y, c, protos0 = _case(H)
    a = _run_step(tr, x, y, c, protos0, step=4)
    b = _run_step(tr, x, y, c, protos0, step=4)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    nxt = _run_step(tr, x, y, c, protos0, step=5)
    assert not np.array_equal(a["G"], nxt["G"])
    tr.set_dropout_base(10)                 # the same optimizer step, split differently
    same = _run_step(tr, x, y, c, protos0, step=4)
    assert same["G"].tobytes() == nxt["G"].tobytes()


def _host_loop(tr, st, wins, anom, cls):
    """backprop's steps issued one by one: tune_step1(step=i) + one adam_step
    each, the masks based at the trainer's step count before the call."""
    dev = tr.device
    st.num_zero, st.num_ones = 1, 1
    tr.set_dropout_base(tr.dropout_base())
    state = st.to_device(dev)
    n = wins.shape[0]
    loss = torch.zeros((n, 2), dtype=torch.float64, device=dev)
    W_ = torch.tensor(wins, dtype=torch.float32, device=dev)
    Y = torch.tensor(anom, dtype=torch.int32, device=dev)
    C = torch.tensor(cls, dtype=torch.int32, device=dev)
    for i in range(n):
        tr.tune_step1(W_[i], Y[i], C[i], state, loss[i], step=i)
        inactive = () if np.any(anom[i] > 0) else ("prototype_decoder.0.weight", "prototype_decoder.0.bias")
        tr.adam_step("transformer", inactive)
    st.from_device(state)
    return [tuple(r) for r in loss.cpu().numpy().tolist()]


def test_dropout_graph_equals_host_loop():
    from preganplus_amd import train as TR
    w, extra = load16()
    z = np.load(f"{GOLD}/tune_h16.npz")
    wins, anom, cls = z["windows"][:4], z["anom"][:4].copy(), z["cls"][:4]
    anom[3] = 0                              # a step with an inactive prototype decoder
    mk = lambda: (TR.Trainer(16, w, extra, dropout=0.1, dropout_seed=7),
                  TR.TuneState(z["protos0"], float(z["factor0"])))
    (a, sa), (b, sb) = mk(), mk()
    base = a.dropout_base()
    first = None
    for call in range(2):
        la = TR.backprop(a, sa, wins, anom, cls)
        lb = _host_loop(b, sb, wins, anom, cls)
        np.testing.assert_allclose(np.array(la), np.array(lb), rtol=1e-12, atol=1e-12)
        for u, v in ((a.P, b.P), (a.m, b.m), (a.v, b.v)):
            assert u.cpu().numpy().tobytes() == v.cpu().numpy().tobytes()
        np.testing.assert_array_equal(sa.protos, sb.protos)
        assert a.dropout_base() == base + 4 * (call + 1)
        first = la if first is None else first
    # a second call on the same windows is not a fresh trainer's first call: the base advanced
    # (and so did the weights)
    assert not np.allclose(np.array(la), np.array(first), rtol=1e-12, atol=1e-12)
    assert len(a._graphs) == 1
    # against the p = 0 graph: dropout changed the training
    c, sc = TR.Trainer(16, w, extra), TR.TuneState(z["protos0"], float(z["factor0"]))
    TR.backprop(c, sc, wins, anom, cls)
    TR.backprop(c, sc, wins, anom, cls)
    assert not torch.equal(a.P, c.P)


class _Obj:
    pass


class _FakeContainer:
    def __init__(self, cid, hid):
        self.id, self._h = cid, hid

    def getHostID(self):
        return self._h


def _fake_env(z, step, train_time, ss_all_rows):
    """The stand-in environment of tests/golden/plugin_h16.npz (as
    test_train_oracle_golden.fake_env)."""
    tt = int(z["T0"]) + step
    env = _Obj()
    env.hostlist = list(range(16))
    placement = z[f"s{step}/placement"]
    cl = [_FakeContainer(c, int(placement[c])) for c in range(16)]
    cl[int(z["container_none"]) if "container_none" in z.files else 3] = None
    env.containerlist = cl
    env.scheduler = _Obj()
    env.scheduler.result_cache = z[f"s{step}/sched"]
    env.stats = _Obj()
    env.stats.time_series = train_time[:tt + 1]
    env.stats.schedule_series = ss_all_rows[:tt + 1]
    sc = [tuple(x) for x in z[f"s{step}/scores"]]
    env.stats.runSimulation = lambda sched: sc.pop(0)
    return env


def _plugin_run(**kw):
    from preganplus_amd.recovery import PreGANPlusRecovery
    w, extra = load16()
    z = np.load(f"{GOLD}/plugin_h16.npz")
    rec = PreGANPlusRecovery(16, "", training=True, weights=w, extra=extra, **kw)
    decisions = []
    for step in range(4):
        rec.setEnvironment(_fake_env(z, step, extra["train_time_data"], z["schedule_series"]))
        decisions.append(rec.run_model(None, [tuple(x) for x in z[f"s{step}/decision_in"]]))
    torch.cuda.synchronize()
    return rec, decisions


def test_plugin_trains_with_dropout():
    drop, dec = _plugin_run(dropout=0.1, dropout_seed=1)
    assert drop.trainer.dropout == pytest.approx(0.1) and drop.trainer.dropout_seed == 1
    for d in dec:                            # a decision list: (container id, host id) pairs, a container once
        assert isinstance(d, list)
        cids = [int(cid) for cid, _ in d]
        assert len(set(cids)) == len(cids)
        assert all(len(e) == 2 and 0 <= int(e[1]) < 16 and 0 <= int(e[0]) < 16 for e in d)
    assert len(drop.accuracy_list) >= 8      # (gen_loss, disc_loss) and (loss, factor, AScore, CScore) per call
    flat = np.concatenate([np.asarray(e, dtype=np.float64) for e in drop.accuracy_list])
    assert np.isfinite(flat).all()
    assert torch.isfinite(drop.trainer.P).all()
    zero, dec0 = _plugin_run(dropout=0.0, dropout_seed=1)
    plain, decp = _plugin_run()
    end = drop.trainer.sec_end["transformer"]
    assert not torch.equal(drop.trainer.P[:end], zero.trainer.P[:end])
    # dropout = 0 is the plugin built without the argument, bit for bit
    assert zero.trainer.P.cpu().numpy().tobytes() == plain.trainer.P.cpu().numpy().tobytes()
    assert dec0 == decp
    assert zero.accuracy_list == plain.accuracy_list
    np.testing.assert_array_equal(zero.tune_state.protos, plain.tune_state.protos)


def test_dropout_is_refused_where_it_is_not_built():
    from preganplus_amd import _native
    from preganplus_amd import train as TR
    from preganplus_amd.recovery import PreGANPlusRecovery
    w50 = W.synth_weights(50, seed=1)
    with pytest.raises(ValueError, match="8, 16"):
        PreGANPlusRecovery(50, "", weights=w50, extra={"train_time_data": np.ones((4, 150))}, dropout=0.1)
    with pytest.raises(ValueError, match="8, 16"):
        TR.Trainer(50, w50, max_batch=1, dropout=0.1)
    with pytest.raises(_native.NativeError):  # PGP_ERR_UNSUPPORTED from the C-ABI
        TR.Trainer(50, w50, max_batch=1).dropout_masks(p=0.1)
    tr = _trainer(16, dropout=0.1)
    st = TR.TuneState(np.full((3, 2), 0.5))
    z = np.load(f"{GOLD}/tune_h16.npz")
    with pytest.raises(ValueError):          # the token-major (non-fused) path
        TR.backprop(tr, st, z["windows"][:2], z["anom"][:2], z["cls"][:2], fused=False)
    with pytest.raises(ValueError):
        TR.DPTuner(tr, st, 4)
    with pytest.raises(ValueError):
        tr.tune_backward(1, z["anom"][:1], np.ones((1, 16)), np.zeros((1, 16, 2)))
    with pytest.raises(ValueError):
        TR.OnlineTrainStep(tr, st, None, np.zeros((1, 10, 48)), np.ones(48), np.zeros((1, 16, 16)),
                           np.zeros((1, 4)))
    # the p = 0 trainer is untouched by all of this
    assert math.isclose(_trainer(16).dropout, 0.0)
