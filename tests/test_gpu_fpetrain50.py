"""PreGAN's offline FPE training on the device at 50 hosts
(preganplus_amd/fpetrain.py, csrc/pgp_fpetrain.hip fpe_step_kernel<50, .>)
against the reference's own modules: tests/golden/fpe_train_h50*.npz
(make_golden_fpetrain50.py) hold two epochs of train.backprop + accuracy of the
reference FPE_16 class at n_hosts = 50 over 24 windows of a synthetic series,
every GRU state the forwards drew, and three single steps.  The oracle the
steps are also compared with is pinned to that fixture on the CPU
(test_fpetrain50_fixture.py).  Tolerances: those of the 16-host tests
(test_gpu_fpetrain.py); fp32 torch autograd of the oracle stays below 0.01 of
the gradient tolerance on such data, so a failure is a bug, not rounding."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import pregan_oracle as O
from oracle import pregan_train_oracle as TO
from tests import fpetrain50_common as C
from tests.decision_bounds import ATOL_LOGIT, ATOL_PROB, RTOL

pytestmark = pytest.mark.gpu

H = C.H


def _dev(a, dt):
    return torch.as_tensor(np.asarray(a), dtype=dt).cuda().contiguous()


def _step(ft, win, h0, y, c, state):
    """One pgp_fpe_train_step from the trainer's P into its G: (loss [2], state) as numpy."""
    from preganplus_amd import _native
    from preganplus_amd import train as TR
    w, h = _dev(win, torch.float32), _dev(h0, torch.float32)
    yy, cc = _dev(y, torch.int32), _dev(np.clip(c, 0, 2), torch.int32)
    sv = torch.tensor(state, dtype=torch.float64, device="cuda")
    loss = torch.zeros(2, dtype=torch.float64, device="cuda")
    _native.check(ft._L.pgp_fpe_train_step(H, 3, w.data_ptr(), h.data_ptr(), yy.data_ptr(), cc.data_ptr(),
                                           ft.P.data_ptr(), ft.G.data_ptr(), sv.data_ptr(), TR.PROTO_UPDATE_MIN,
                                           TR.PROTO_FACTOR_DECAY, loss.data_ptr(), ft._stream()),
                  "pgp_fpe_train_step")
    torch.cuda.synchronize()
    return loss.cpu().numpy(), sv.cpu().numpy()


def _step_state(zs, protos):
    from preganplus_amd import train as TR
    st = TR.TuneState(protos, float(zs["factor"]))
    st.num_zero, st.num_ones = int(zs["num_zero"]), int(zs["num_ones"])
    return st


@pytest.mark.parametrize("j", [0, 1, 2])
def test_fpe50_step_gradient_matches_fixture_and_autograd(j):
    """One device step from the initial weights on the recorded many-positives
    / idle / other window: losses, the gradient of every tensor and the updated
    state, against the reference's record and torch autograd of the oracle."""
    from preganplus_amd import fpetrain as FT
    z, _, zs, init, protos = C.fixture()
    i = int(zs["index"][j])
    h0 = zs[f"s{j}/h0"][None]
    ft = FT.FPETrainer(init, H=H)
    lo, sv = _step(ft, z["wins"][i], h0, z["anom"][i], z["cls"][i], _step_state(zs, protos).vector())
    fw = TO.leaf_params(init, skip=())
    sto = TO.TuneState(protos, float(zs["factor"]))
    sto.num_zero, sto.num_ones = int(zs["num_zero"]), int(zs["num_ones"])
    probs, pr = TO.fpe_t(fw, torch.tensor(z["wins"][i:i + 1]), torch.tensor(h0))
    aloss, tloss = TO.custom_loss(probs[0], pr[0], z["anom"][i], z["cls"][i], sto)
    (aloss + tloss).backward()
    for wa, wt in ((float(aloss), float(tloss)), tuple(zs[f"s{j}/loss"])):
        print(f"step {j}: loss {lo} want {(wa, wt)}")
        assert lo[0] == pytest.approx(wa, rel=1e-4) and lo[1] == pytest.approx(wt, rel=1e-3, abs=1e-6)
    g = ft.G.cpu().numpy()
    worst = 0.0

    def cmp(got, want, what):
        nonlocal worst
        got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
        tol = 1e-3 * np.abs(want) + 1e-4 * (scale + 1e-30)
        worst = max(worst, float((np.abs(got - want) / tol).max()))
        assert np.all(np.abs(got - want) <= tol), (what, np.abs(got - want).max(), scale)

    for t in ft.tensors:
        want = fw[t["name"]].grad
        want = np.zeros(t["n"]) if want is None else want.numpy().reshape(-1)
        got = g[t["offset"]:t["offset"] + t["n"]]
        scale = np.abs(want).max()                       # the tensor's largest gradient entry (fp64 autograd)
        cmp(got, want, t["name"] + " vs autograd")
        C.recorded(zs, f"s{j}/g/{t['name']}", got.reshape(t["shape"]), cmp, key=t["name"])
    print(f"step {j}: worst |got - want| / tol over all tensors {worst:.3g}")
    for want_p, want_s in ((np.stack([p.numpy() for p in sto.protos]), (sto.factor, sto.num_zero, sto.num_ones)),
                           (zs[f"s{j}/prototypes"], tuple(zs[f"s{j}/state"]))):
        np.testing.assert_allclose(sv[:6].reshape(3, 2), want_p, rtol=1e-6)
        assert sv[6] == pytest.approx(want_s[0], rel=1e-15) and (sv[7], sv[8]) == tuple(want_s[1:])


def test_fpe50_idle_window_writes_every_gradient():
    """A window without a positive label: the step writes every element of G
    (prefilled with NaN), the prototype decoder's gradient is exactly 0, and
    backprop leaves that tensor's AdamW step count unchanged (torch skips a
    parameter without a gradient)."""
    from preganplus_amd import fpetrain as FT
    from preganplus_amd import train as TR
    z, _, zs, init, protos = C.fixture()
    i = int(zs["index"][1])
    assert z["anom"][i].sum() == 0
    ft = FT.FPETrainer(init, H=H)
    ft.G.fill_(float("nan"))
    _step(ft, z["wins"][i], zs["s1/h0"][None], z["anom"][i], z["cls"][i], _step_state(zs, protos).vector())
    g = ft.G.cpu().numpy()
    assert np.isfinite(g).all(), int((~np.isfinite(g)).sum())
    for t in ft.tensors:
        if t["name"] in FT.COND:
            assert np.all(g[t["offset"]:t["offset"] + t["n"]] == 0.0), t["name"]
    assert np.abs(g).max() > 0
    st = TR.TuneState(protos, 0.2)
    ft.backprop(st, z["wins"][i:i + 1], z["ep0/h0_backprop"][i:i + 1], z["anom"][i:i + 1], z["cls"][i:i + 1])
    for t in ft.tensors:
        assert t["step"] == (0.0 if t["name"] in FT.COND else 1.0), (t["name"], t["step"])


def _cscore_within_decision_bounds(ft, st, z, ep, wins, anom, cls, csc):
    """test_gpu_fpetrain._cscore_within_decision_bounds at 50 hosts (the epoch's
    reference parameters come whole or, for encoder.0.weight, cannot: the
    reference forward is therefore the oracle's own training run on the CPU,
    pinned to the fixture by test_fpetrain50_fixture.py, passed in as z["_ref"]).
    class_accuracy (train.py:75-92) counts, per positive host, whether its
    prototype output is closest to its own class.  The device model is the
    reference's up to fp32 training, so a host's verdict may differ only where
    the reference's own distance margin is inside what that difference can
    move: |d_k(a') - d_k(a)| <= |a' - a|_inf * (|a - P_k|_1 + |a' - a|_1 / 2)
    per distance (d_k = mean over the 2 dims of (a - P_k)^2), plus the device
    prototypes' deviation from the reference's.  The reference's CScore must
    equal the fixture's, and the device CScore must equal the reference's with
    exactly the in-bound flips applied."""
    from preganplus_amd import train as TR
    n = wins.shape[0]
    fw = z["_ref"]
    h0 = z[f"ep{ep}/h0_accuracy"]
    with torch.no_grad():
        rp, rq = TO.fpe_t(fw, torch.tensor(wins), torch.tensor(h0))
    rp, rq = rp.numpy().reshape(n, H, 2), rq.numpy().reshape(n, H, 2)
    Pref = np.asarray(z[f"ep{ep}/prototypes"], dtype=np.float64)[:3]
    _, csc_ref = TR.accuracy_scores(rp, rq, anom, cls, Pref)
    assert csc_ref == pytest.approx(float(z[f"ep{ep}/cscore"]), rel=1e-12, abs=1e-12)
    _, dq = ft.forward_many(wins, h0)
    P = np.asarray(st.protos, dtype=np.float64)[:3]

    def hits(q, PP):
        d = np.mean((q[:, :, None, :] - PP[None, None]) ** 2, axis=-1)       # [n,H,3]
        c = np.clip(cls, 0, 2)
        pos = np.take_along_axis(d, c[..., None], -1)[..., 0]
        negs = np.where(np.arange(3)[None, None] == c[..., None], np.inf, d).min(-1)
        return (anom > 0) & (pos <= negs), negs - pos, d

    h_ref, margin, d_ref = hits(rq, Pref)
    h_dev, _, _ = hits(dq, P)
    da = np.abs(dq - rq).max(-1)                                                # per host, inf-norm
    dP = np.abs(P - Pref).max()
    span = np.abs(rq[:, :, None, :] - Pref[None, None]).sum(-1).max(-1)        # max_k |a - P_k|_1
    bound = 2 * ((da + dP) * (span + (da + dP)))                               # pos and neg both move
    flip = h_ref != h_dev
    assert np.all(np.abs(margin[flip]) <= bound[flip]), (np.abs(margin[flip]), bound[flip])
    # the device score is the reference's with those flips: the count is exact
    cc, tot = 0.0, 0
    for i in range(n):
        npos = int(np.sum(anom[i] > 0))
        if npos:
            tot += 1
            cc += int(np.sum(h_dev[i])) / (1e-4 + npos)
    assert csc == pytest.approx(cc / tot, rel=1e-12)
    assert int(flip.sum()) <= max(2, int((np.abs(margin) <= bound).sum()))


def test_fpe50_offline_training_epochs_match_reference():
    """test_fpe_offline_training_epochs_match_reference at 50 hosts, through
    FPETrainer(H=50).backprop and accuracy: fp32 device training vs the fp64
    reference, the same tolerance forms, key-bias exclusion and step counts (the
    AdamW update itself, without them: test_gpu_adamw_fused.py::test_fpe_step_replays)."""
    from preganplus_amd import fpetrain as FT
    from preganplus_amd import train as TR
    z, _, _, init, protos = C.fixture()
    ft = FT.FPETrainer(init, H=H)
    st = TR.TuneState(protos, 0.2)
    wins, anom, cls = z["wins"], z["anom"], z["cls"]
    # the reference's own run restated in fp64 (its parameters after each epoch, whole)
    fw = TO.leaf_params(init, skip=())
    ropt, rst = TO.AdamW(fw, 1e-4), TO.TuneState(protos, 0.2)
    for ep in range(2):
        losses = ft.backprop(st, wins, z[f"ep{ep}/h0_backprop"], anom, cls)
        TO.fpe_backprop(fw, ropt, rst, wins, z[f"ep{ep}/h0_backprop"], anom, cls)
        loss = np.mean([a for a, _ in losses]) + np.mean([t for _, t in losses])
        assert loss == pytest.approx(float(z[f"ep{ep}/loss"]), rel=1e-4)
        assert st.factor + O.PROTO_UPDATE_MIN == pytest.approx(float(z[f"ep{ep}/factor"]), rel=1e-14)
        assert (st.num_zero, st.num_ones) == (z[f"ep{ep}/num_zero"], z[f"ep{ep}/num_ones"])
        np.testing.assert_allclose(st.protos, z[f"ep{ep}/prototypes"], rtol=1e-4, atol=1e-6)
        pw = ft.weights_numpy()
        lr = FT.FPE_LR
        fails = []

        def cmp(got, want, what):
            # fp32 tolerance for all but entries whose gradient is rounding noise: those take
            # AdamW steps of arbitrary sign on both sides, at most 2 lr apart per step.  The
            # attention's key bias (in_proj_bias[E:2E]) is such an entry everywhere: its exact
            # gradient is zero (softmax is invariant to a shift of all scores of a query)
            got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
            noise = np.zeros(want.size, dtype=bool)
            if what.endswith("mha.in_proj_bias"):
                E = want.size // 3
                noise[E:2 * E] = True
            tol = 1e-4 * np.abs(want) + 1e-5 * wmax
            bad = (np.abs(got - want) > tol) & ~noise
            if bad.mean() >= 0.01:
                fails.append((what, int(bad.sum()), float(np.abs(got - want).max())))
            if not np.all(np.abs(got - want) <= 2 * lr * 24 * (ep + 1)):
                fails.append((what, "beyond the lr bound", float(np.abs(got - want).max())))

        for t in ft.tensors:
            k = t["name"]
            wmax = np.abs(fw[k].detach().numpy()).max()      # the reference tensor's largest entry
            # the restated run is the recorded one (pinned on the CPU); the record is compared directly
            C.recorded(z, f"ep{ep}/p/{k}", pw[k], cmp, key=k)
            if t["step"] != float(z[f"ep{ep}/step/{k}"]):
                fails.append((k, "step", t["step"]))
        assert not fails, (ep, fails)
        asc, csc = ft.accuracy(st, wins, z[f"ep{ep}/h0_accuracy"], anom, cls)
        assert asc == pytest.approx(float(z[f"ep{ep}/ascore"]), abs=1.0 / (H * 24) + 1e-12)
        zz = dict(z, _ref={k: q.detach().clone() for k, q in fw.items()})
        _cscore_within_decision_bounds(ft, st, zz, ep, wins, anom, cls, csc)


def test_fpe50_forward_many_batch_invariance():
    """Row i of an n = 300 launch (more workgroups than CUs) is bitwise the
    n = 1 launch on window i."""
    from preganplus_amd import fpetrain as FT
    _, _, _, init, _ = C.fixture()
    ft = FT.FPETrainer(init, H=H)
    rng = np.random.Generator(np.random.PCG64(300))
    wins = rng.uniform(0, 1.1, size=(300, 3, 3 * H)).astype(np.float32)
    h0 = rng.standard_normal((300, 3)).astype(np.float32)
    probs, protos = ft.forward_many(wins, h0)
    assert probs.shape == (300, H, 2) and np.isfinite(probs).all() and np.isfinite(protos).all()
    np.testing.assert_allclose(probs.sum(-1), 1.0, atol=1e-6)
    for i in (0, 150, 299):
        p1, q1 = ft.forward_many(wins[i:i + 1], h0[i:i + 1])
        assert np.array_equal(p1[0], probs[i]) and np.array_equal(q1[0], protos[i]), i


def test_fpe50_step_is_bit_reproducible():
    """The same step twice from the same buffers: identical bits in G, loss and
    state (fixed-order reductions, no atomics)."""
    from preganplus_amd import fpetrain as FT
    z, _, zs, init, protos = C.fixture()
    i = int(zs["index"][0])
    ft = FT.FPETrainer(init, H=H)
    runs = []
    for _ in range(2):
        ft.G.fill_(float("nan"))
        lo, sv = _step(ft, z["wins"][i], zs["s0/h0"][None], z["anom"][i], z["cls"][i],
                       _step_state(zs, protos).vector())
        runs.append((ft.G.cpu().numpy().copy(), lo, sv))
    for a, b in zip(runs[0], runs[1]):
        assert a.tobytes() == b.tobytes()


def test_fpe50_trained_weights_run_in_k4():
    """Train -> infer: after epoch 0 the trainer's weights, loaded into
    FPEDecisionModel(50, ...), give K4 scores and prototypes on the 24 windows
    (same h0) that agree with forward_many: both kernels within K4's tolerance
    (tests/test_gpu_fpe.py) of the fp64 oracle on those weights."""
    from preganplus_amd import fpetrain as FT
    from preganplus_amd import train as TR
    from preganplus_amd import weights as W
    from preganplus_amd.model import FPEDecisionModel, to_numpy
    z, _, _, init, protos = C.fixture()
    ft = FT.FPETrainer(init, H=H)
    st = TR.TuneState(protos, 0.2)
    wins, h0 = z["wins"], z["ep0/h0_accuracy"]
    ft.backprop(st, wins, z["ep0/h0_backprop"], z["anom"], z["cls"])
    fpe = ft.weights_numpy()
    probs, prs = ft.forward_many(wins, h0)
    full = W.synth_fpe_weights(H, seed=0)
    m = FPEDecisionModel(H, {"fpe": fpe, "gen": full["gen"], "disc": full["disc"], "prototypes": st.protos})
    sched = np.zeros((C.N_WIN, H, H), dtype=np.float32)
    sched[:, np.arange(H), np.arange(H)] = 1.0
    out = to_numpy(m.forward(_dev(wins, torch.float32), _dev(h0, torch.float32), _dev(sched, torch.float32)))
    with torch.no_grad():
        rp, rq = TO.fpe_t({k: torch.tensor(v) for k, v in fpe.items()}, torch.tensor(wins), torch.tensor(h0))
    rp, rq = rp.numpy().reshape(-1, H, 2), rq.numpy().reshape(-1, H, 2)
    for name, sc, pq in (("K4", out["scores"], out["protos"]), ("forward_many", probs, prs)):
        print(name, "max abs err scores", np.abs(sc - rp).max(), "protos", np.abs(pq - rq).max())
        np.testing.assert_allclose(sc, rp, rtol=RTOL, atol=ATOL_LOGIT, err_msg=name + " scores")
        np.testing.assert_allclose(pq, rq, rtol=RTOL, atol=ATOL_PROB, err_msg=name + " protos")


def test_fpe50_optimizer_state_round_trip():
    """FPETrainer(state=..., H=50) restores the AdamW moments and step counts
    that checkpoint() writes: a restored trainer's next step equals the
    original's."""
    from preganplus_amd import fpetrain as FT
    from preganplus_amd import train as TR
    z, _, _, init, protos = C.fixture()
    wins, anom, cls = z["wins"][3:9], z["anom"][3:9], z["cls"][3:9]    # holds idle windows 5 and 6
    h0 = z["ep0/h0_backprop"][3:9]
    a = FT.FPETrainer(init, H=H)
    st = TR.TuneState(protos, 0.2)
    a.backprop(st, wins[:4], h0[:4], anom[:4], cls[:4])
    ck = a.checkpoint(0, [], st.protos)
    b = FT.FPETrainer({k: np.asarray(v) for k, v in ck["model_state_dict"].items()},
                      state=ck["optimizer_state_dict"]["state"], H=H)
    assert [t["step"] for t in b.tensors] == [t["step"] for t in a.tensors] and a.tensors[0]["step"] > 0
    np.testing.assert_array_equal(b.m.cpu().numpy(), a.m.cpu().numpy())
    np.testing.assert_array_equal(b.v.cpu().numpy(), a.v.cpu().numpy())
    st2 = TR.TuneState(st.protos, st.factor)
    a.backprop(st, wins[4:], h0[4:], anom[4:], cls[4:])
    b.backprop(st2, wins[4:], h0[4:], anom[4:], cls[4:])
    np.testing.assert_array_equal(b.P.cpu().numpy(), a.P.cpu().numpy())


def test_fpe50_unsupported_host_count():
    from preganplus_amd import fpetrain as FT
    with pytest.raises(ValueError, match="16, 50"):
        FT.FPETrainer({}, H=32)
    L = FT._native.lib()
    one = ctypes.c_void_p(torch.zeros(8, device="cuda").data_ptr())
    assert L.pgp_fpe_forward_many(32, 1, one, one, one, one, one, None) == -2      # PGP_ERR_UNSUPPORTED
    assert L.pgp_fpe_train_step(32, 3, one, one, one, one, one, one, one, 0.02, 0.995, one, None) == -2


def test_pregan50_new_model_trains_offline(tmp_path, monkeypatch):
    """test_pregan_new_model_trains_offline at 50 hosts: no FPE checkpoint, no
    packaged weights; PreGANRecovery trains a new FPE for 2 epochs on a [30,150]
    series, rewriting framework_FPE_50.ckpt each epoch in the reference's
    format, then runs on the trained encoder; a second plugin loads it."""
    from preganplus_amd import recovery as RC
    from preganplus_amd import weights as W
    rng = np.random.default_rng(4)
    d = tmp_path / "recovery" / "PreGANSrc" / "data" / "framework"
    d.mkdir(parents=True)
    np.save(d / "time_series.npy", rng.uniform(0, 100, size=(30, 3 * H)))
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(RC, "NUM_EPOCHS", 2)
    saved = []
    real_save = RC._save_atomic
    monkeypatch.setattr(RC, "_save_atomic", lambda ck, path: (saved.append((int(ck["epoch"]), path)),
                                                              real_save(ck, path))[1])
    torch.manual_seed(5)
    rec = RC.PreGANRecovery(H, "framework", training=False, model_folder=str(tmp_path / "ck"))
    assert rec.fpe_epoch == 1 and len(rec.fpe_accuracy_list) == 2
    path = str(tmp_path / "ck" / "framework_FPE_50.ckpt")
    assert saved == [(0, path), (1, path)]                      # written after every epoch
    ck = W._safe_load(path)
    assert int(ck["epoch"]) == 1 and len(ck["accuracy_list"]) == 2 and len(ck["model_prototypes"]) == 3
    assert rec.fpe_trainer.H == H and rec.model.H == H
    fw = rec.fpe_trainer.weights_numpy()
    assert set(ck["model_state_dict"]) == set(W.fpe_shapes(H))
    for k, v in ck["model_state_dict"].items():
        assert tuple(v.shape) == tuple(W.fpe_shapes(H)[k])
        np.testing.assert_array_equal(np.asarray(v), fw[k])
    assert rec.epoch == -1            # a new GAN (load_gan without checkpoints)
    np.testing.assert_array_equal(rec.weights["fpe"]["encoder.0.weight"], fw["encoder.0.weight"])
    rec2 = RC.PreGANRecovery(H, "framework", training=True, model_folder=str(tmp_path / "ck"))
    assert rec2.epoch == -1 and rec2.accuracy_list == []
    np.testing.assert_array_equal(rec2.weights["fpe"]["encoder.0.weight"], fw["encoder.0.weight"])
    np.testing.assert_array_equal(rec2.weights["gen"]["delta.0.weight"], rec.weights["gen"]["delta.0.weight"])
