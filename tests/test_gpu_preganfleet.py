"""The PreGAN fleet forward and plugin on the GPU: pgp_fpe_forward1 /
pgp_fpe_forward1_many (the FPE training kernel's forward continued by detect / embed /
get_classes and Gen_16 / Disc_16 from the training master, one workgroup per cell),
``PreGANFleetRecovery`` and ``PreGANRecovery(master_forward=True)``.  16 hosts, K = 3."""
import numpy as np
import pytest
import torch

from oracle import pregan_oracle as O
from preganplus_amd import _native
from preganplus_amd import fpetrain as FT
from preganplus_amd import weights as W
from tests.parity_utils import ATOL_PROB, RTOL, assert_parity

pytestmark = pytest.mark.gpu

H, K = 16, 3
OUT = (("scores", np.float32, (H, 2)), ("protos", np.float32, (H, 2)), ("cls", np.int32, (H,)), ("any", np.int32, ()),
       ("probs", np.float32, (2,)), ("keep", np.int32, ()), ("final_target", np.int32, (H,)),
       ("gen_target", np.int32, (H,)))
_T = {np.float32: torch.float32, np.int32: torch.int32}


def shipped():
    return W.load_npz("preganplus_amd/data/pregan_simulator_16.npz")


def cell_arrays(w):
    """One cell's weight arrays as the entries read them: the natural FPE blob, a training master with
    the cell's Gen / Disc (zero Transformer), the prototypes fp64."""
    from preganplus_amd.recovery import _gan_only
    n = int(_native.lib().pgp_master_len(H))
    return {"P_fpe": FT.fpe_blob(w["fpe"], H).numpy(),
            "P_master": W.pack_blob(_gan_only(H, w), H)[:n].astype(np.float32),
            "prototypes": np.ascontiguousarray(w["prototypes"], dtype=np.float64).reshape(-1)}


def forward(cells, windows, h0, sched, lone=False, active=None, sentinel=None, stride=None):
    """The entry on M cells (cells[m]: ``cell_arrays``) -> numpy outputs with a leading M axis.
    sentinel: the value every output row starts from."""
    L, dev = _native.lib(), "cuda"
    M = len(cells)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    P, Pm = (up(np.stack([c[k] for c in cells]), np.float32) for k in ("P_fpe", "P_master"))
    pr = np.stack([c["prototypes"] for c in cells])
    if stride is not None:          # rows of a tuning state [2K+3]: the prototypes at the head
        pr = np.concatenate([pr, np.full((M, stride - 2 * K), 1e30)], axis=1)
    pr = up(pr, np.float64)
    w, h, s = up(windows, np.float32), up(h0, np.float32), up(sched, np.float32)
    assert w.shape == (M, 3, 3 * H) and h.shape == (M, 3) and s.shape == (M, H, H)
    out = {k: torch.full((M,) + shp, 0 if sentinel is None else sentinel, dtype=_T[dt], device=dev)
           for k, dt, shp in OUT}
    p = lambda t: t.data_ptr()
    outs = [p(out[k]) for k, _, _ in OUT]
    if lone:
        assert M == 1 and active is None and stride is None
        _native.check(L.pgp_fpe_forward1(H, K, p(w), p(h), p(s), p(P), p(Pm), p(pr), *outs, None), "pgp_fpe_forward1")
    else:
        act = None if active is None else up(active, np.int32)
        _native.check(L.pgp_fpe_forward1_many(H, K, M, None if act is None else p(act), p(w), p(h), p(s), p(P), p(Pm),
                                              p(pr), pr.shape[1], *outs, None), "pgp_fpe_forward1_many")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def as_parity(got, ref):
    """tests/test_gpu_fpe.as_parity: the anomaly softmax plays the detect logits, the Disc's probs are 'probs'."""
    return dict(got, logits=got["scores"]), dict(ref, logits=ref["probs"], probs=ref["gprobs"])


def synth_inputs(s, n=64):
    rng = np.random.Generator(np.random.PCG64(s))
    x = rng.uniform(0, 1.2, size=(n, 3, 3 * H)).astype(np.float32)
    h0 = rng.standard_normal((n, 3)).astype(np.float32)
    sched = rng.uniform(0, 1, size=(n, H, H)).astype(np.float32)
    return x, h0, sched


_cache = {}


def synth_case(s):
    """Seed s: the weights, their arrays, 64 inputs and the fp64 oracle on them (computed once)."""
    if s not in _cache:
        w = W.synth_fpe_weights(H, seed=s)
        x, h0, sched = synth_inputs(s)
        ref = O.forward_fpe(w, x.astype(np.float64), h0.astype(np.float64), sched.astype(np.float64))
        _cache[s] = (w, cell_arrays(w), x, h0, sched, ref)
    return _cache[s]


# ---- 1. the forward is the training kernel's forward ----

def test_forward_is_the_training_kernels_forward():
    w, _ = shipped()
    z = np.load("tests/golden/fpe_h16.npz")
    c = cell_arrays(w)
    L, n = _native.lib(), 8
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()
    wd, hd, P = t(z["windows"][:n], np.float32), t(z["h0"][:n], np.float32), t(c["P_fpe"], np.float32)
    probs, protos = (torch.zeros((n, H, 2), dtype=torch.float64, device="cuda") for _ in range(2))
    _native.check(L.pgp_fpe_forward_many(H, n, wd.data_ptr(), hd.data_ptr(), P.data_ptr(), probs.data_ptr(),
                                         protos.data_ptr(), None), "pgp_fpe_forward_many")
    torch.cuda.synchronize()
    probs, protos = probs.cpu().numpy(), protos.cpu().numpy()
    for i in range(n):
        got = forward([c], z["windows"][i:i + 1], z["h0"][i:i + 1], z["sched"][i:i + 1], lone=True)
        assert got["scores"][0].astype(np.float64).tobytes() == probs[i].tobytes(), i
        assert got["protos"][0].astype(np.float64).tobytes() == protos[i].tobytes(), i


# ---- 2. the reference fixture ----

def test_reference_fixture_as_160_cells():
    """All 160 recorded windows as one launch of 160 cells of the shipped weights.  Every decision but the
    class equals the fixture; the class may differ only inside decision_bounds' fp32 bound and at no more than
    7 hosts (the reference's own near-ties: 7 of 1,408 class margins lie below 1e-4, 2 below 1e-5)."""
    w, _ = shipped()
    z = np.load("tests/golden/fpe_h16.npz")
    ref = {k: z[k] for k in z.files}
    n = len(ref["windows"])
    assert n == 160
    got = forward([cell_arrays(w)] * n, ref["windows"], ref["h0"], ref["sched"])
    g, r = as_parity(got, ref)
    r["sched32"] = ref["sched"].astype(np.float32)
    st = assert_parity(g, r, w, ref["sched"], check_latent=False)
    for k in ("any", "keep", "final_target", "gen_target"):
        assert np.array_equal(got[k], ref[k]), k
    assert np.array_equal(got["scores"][..., 1] > got["scores"][..., 0], ref["probs"][..., 1] > ref["probs"][..., 0])
    print("class census:", st["class"])
    assert st["class"]["mismatch"] <= 7 and int((got["cls"] != ref["cls"]).sum()) <= 7, st["class"]


# ---- 3. every branch, against the fp64 oracle ----

def test_every_branch_against_the_oracle():
    seeds = (11, 12, 13)
    cases = [synth_case(s) for s in seeds]
    cells = [c[1] for c in cases for _ in range(64)]
    x, h0, sched = (np.concatenate([c[i] for c in cases]) for i in (2, 3, 4))
    got = forward(cells, x, h0, sched)
    assert len(cells) == 192
    for j, (w, _, _, _, sc, ref) in enumerate(cases):
        part = {k: v[64 * j:64 * j + 64] for k, v in got.items()}
        g, r = as_parity(part, ref)
        r["sched32"] = sc
        assert_parity(g, r, w, sc, check_latent=False)
    a, k = got["any"].reshape(3, 64), got["keep"].reshape(3, 64)
    assert a[0].all() and k[0].all()                    # every window anomalous, the original decision kept
    assert not a[1].any() and (got["cls"][64:128] == -1).all()   # no anomalous host at all
    assert a[2].all() and 0 < k[2].sum() < 64           # anomalous, both gate outcomes
    # the GAN part runs whether or not a host is anomalous: every output of those cells is defined
    assert np.isfinite(got["probs"][64:128]).all() and np.allclose(got["probs"][64:128].sum(axis=1), 1, atol=1e-6)


# ---- 4. cell independence ----

def test_cell_independence_and_inactive_cells():
    seeds = (11, 12, 13)
    cases = [synth_case(s) for s in seeds]
    arr = [c[1] for c in cases]
    inp = lambda j, i: tuple(cases[j][k][i:i + 1] for k in (2, 3, 4))       # window i of seed j's inputs
    lone = lambda j, i: forward([arr[j]], *inp(j, i), lone=True)
    same = lambda a, b, m, what: [pytest.fail(f"{what}: {k}") for k in a if a[k][m].tobytes() != b[k][0].tobytes()]
    # slot 0 of 1
    same(forward([arr[2]], *inp(2, 5)), lone(2, 5), 0, "slot 0 of 1")
    # slot 2 of 3, distinct weights per slot; prototypes at the head of a state row (stride 2K + 3)
    idx = [(0, 1), (1, 2), (2, 3)]
    ins = [np.concatenate([inp(j, i)[k] for j, i in idx]) for k in range(3)]
    three = forward([arr[j] for j, _ in idx], *ins, stride=2 * K + 3)
    for m, (j, i) in enumerate(idx):
        same(three, lone(j, i), m, f"slot {m} of 3")
    # slot 299 of 300 (more cells than CUs), weights cycling over the three seeds
    idx = [(m % 3, m % 64) for m in range(300)]
    ins = [np.concatenate([inp(j, i)[k] for j, i in idx]) for k in range(3)]
    many = forward([arr[j] for j, _ in idx], *ins)
    for m in (0, 1, 2, 150, 298, 299):
        same(many, lone(*idx[m]), m, f"slot {m} of 300")
    # an inactive cell: its sentinel-filled rows come back untouched, its neighbours are as without it
    active = np.ones(300, dtype=np.int32)
    active[[0, 7, 299]] = 0
    masked = forward([arr[j] for j, _ in idx], *ins, active=active, sentinel=-77)
    for k, v in masked.items():
        assert (v[[0, 7, 299]] == -77).all(), k
        on = active.astype(bool)
        assert v[on].tobytes() == many[k][on].tobytes(), k


# ---- 5. the GAN tail against the existing fused GAN forward ----

def test_gan_tail_against_fused_gan_forward():
    L = _native.lib()
    w, c, x, h0, sched, _ = synth_case(13)
    n = 8
    got = forward([c] * n, x[:n], h0[:n], sched[:n])
    anom = got["scores"][..., 1] > got["scores"][..., 0]
    emb = np.where(anom[..., None], got["protos"], 0).astype(np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    P = t(c["P_master"])
    ws = torch.zeros(int(L.pgp_gan_workspace_len(H, 1)), dtype=torch.float32, device="cuda")
    for i in range(n):
        e, s = t(emb[i].reshape(-1)), t(sched[i])
        ns, probs = torch.zeros(H * H, device="cuda"), torch.zeros(2, device="cuda")
        _native.check(L.pgp_gan_forward1(H, e.data_ptr(), s.data_ptr(), P.data_ptr(), ws.data_ptr(), ns.data_ptr(),
                                         probs.data_ptr(), None), "pgp_gan_forward1")
        torch.cuda.synchronize()
        np.testing.assert_allclose(got["probs"][i], probs.cpu().numpy(), rtol=RTOL, atol=ATOL_PROB, err_msg=str(i))
        assert np.array_equal(got["gen_target"][i], ns.cpu().numpy().reshape(H, H).argmax(axis=1)), i


# ---- 6. the plugin against the recorded intervals ----

def draw_h0(seed):
    torch.manual_seed(seed)
    return torch.randn(1, 1, 3, dtype=torch.double).numpy().reshape(3)


def test_fleet_plugin_matches_recorded_intervals():
    from preganplus_amd.recovery import PreGANFleetRecovery
    from tests.test_gpu_train import close
    from tests.test_train_oracle_golden import fake_env
    w, extra = shipped()
    z = np.load("tests/golden/pregan_plugin_h16.npz")
    M = 3
    rec = PreGANFleetRecovery(16, [w] * M, [extra] * M, training=True)
    for step in range(4):
        rec.setEnvironments([fake_env(z, step, extra["train_time_data"], z["schedule_series"]) for _ in range(M)])
        din = [tuple(x) for x in z[f"s{step}/decision_in"]]
        decs = rec.run_model([list(din) for _ in range(M)], h0=np.tile(draw_h0(2000 + step), (M, 1)))
        for m in range(M):
            assert [tuple(map(int, d)) for d in decs[m]] == [tuple(x) for x in z[f"s{step}/decision_out"].tolist()], \
                (step, m)
    for m in range(M):
        pw = rec.tuner.trainer(m)[0].weights_numpy()
        for k, v in pw["gen"].items():
            close(v, z[f"end/g/{k}"], rel=1e-4, abs_scale=1e-5, what=f"cell {m} g {k}")
        for k, v in pw["disc"].items():
            close(v, z[f"end/d/{k}"], rel=1e-4, abs_scale=1e-5, what=f"cell {m} d {k}")
        np.testing.assert_allclose(np.array(rec.accuracy_list[m][-4:]), z["end/accuracy_list"], rtol=1e-4, atol=1e-6)
        assert rec.epoch[m] == int(extra["meta/gen/epoch"]) + 4


# ---- 7. the fleet equals lone plugins ----

def test_fleet_equals_lone_plugins():
    from preganplus_amd.recovery import PreGANFleetRecovery, PreGANRecovery
    from tests.test_train_oracle_golden import fake_env
    w0, extra = shipped()
    z = np.load("tests/golden/pregan_plugin_h16.npz")
    ws = [w0] + [W.synth_fpe_weights(16, seed=s) for s in (11, 12, 13)]     # seed 12: never an anomaly
    M = len(ws)
    env = lambda step: fake_env(z, step, extra["train_time_data"], z["schedule_series"])
    fleet = PreGANFleetRecovery(16, ws, [extra] * M, training=True)
    lones = [PreGANRecovery(16, "", training=True, master_forward=True, weights=w, extra=extra) for w in ws]
    snap = lambda P, m_, v: tuple(t.cpu().numpy().tobytes() for t in (P, m_, v))
    first = [snap(fleet.tuner.P[m], fleet.tuner.m[m], fleet.tuner.v[m]) for m in range(M)]
    for step in range(2):
        din = [tuple(x) for x in z[f"s{step}/decision_in"]]
        seeds = [3000 + 10 * step + m for m in range(M)]
        fleet.setEnvironments([env(step) for _ in range(M)])
        decs = fleet.run_model([list(din) for _ in range(M)], h0=np.stack([draw_h0(s) for s in seeds]))
        for m, rec in enumerate(lones):
            rec.setEnvironment(env(step))
            torch.manual_seed(seeds[m])           # the lone plugin draws its own h0 (models.py:70)
            assert rec.run_model(None, list(din)) == decs[m], (step, m)
    torch.cuda.synchronize()
    for m, rec in enumerate(lones):
        now = snap(fleet.tuner.P[m], fleet.tuner.m[m], fleet.tuner.v[m])
        assert now == snap(rec.trainer.P, rec.trainer.m, rec.trainer.v), m
        assert fleet.accuracy_list[m] == rec.accuracy_list and fleet.epoch[m] == rec.epoch, m
        assert fleet.classes[m] == getattr(rec, "classes", None), m
        assert fleet.hosts_from[m] == getattr(rec, "hosts_from", None), m
        if m == 2:
            assert now == first[m] and fleet.epoch[m] == int(extra["meta/gen/epoch"])   # the cell without an anomaly
        else:
            assert now != first[m] and fleet.epoch[m] == int(extra["meta/gen/epoch"]) + 2
    # master_forward=False stays the old path: the recorded decision of interval 0
    old = PreGANRecovery(16, "", training=True, weights=w0, extra=extra)
    assert old.master_forward is False
    old.setEnvironment(env(0))
    torch.manual_seed(2000)
    dec = old.run_model(None, [tuple(x) for x in z["s0/decision_in"]])
    assert [tuple(map(int, d)) for d in dec] == [tuple(x) for x in z["s0/decision_out"].tolist()]


# ---- 8. inference only ----

def test_fleet_inference_only_and_set_fpe():
    from preganplus_amd.recovery import PreGANFleetRecovery, _recover
    from tests.test_train_oracle_golden import fake_env
    w0, extra = shipped()
    z = np.load("tests/golden/pregan_plugin_h16.npz")
    ws = [w0, W.synth_fpe_weights(16, seed=11), W.synth_fpe_weights(16, seed=13)]
    M = len(ws)
    rec = PreGANFleetRecovery(16, ws, [extra] * M, training=False)
    before = [t.cpu().numpy().tobytes() for t in (rec.tuner.P, rec.tuner.m, rec.tuner.v, rec.fpe_P, rec.prototypes)]
    kept = set()
    for step in range(2):
        envs = [fake_env(z, step, extra["train_time_data"], z["schedule_series"]) for _ in range(M)]
        rec.setEnvironments(envs)
        din = [tuple(x) for x in z[f"s{step}/decision_in"]]
        h0 = np.stack([draw_h0(3000 + 10 * step + m) for m in range(M)])
        decs = rec.run_model([list(din) for _ in range(M)], h0=h0)
        wins = np.stack([rec._input_window(m) for m in range(M)])
        out = {k: v.copy() for k, v in rec.forward(wins, h0, np.stack([z[f"s{step}/sched"]] * M)).items()}
        for m in range(M):
            assert out["any"][m]
            kept.add(bool(out["keep"][m]))
            if out["keep"][m]:               # the forward's own gate: the original decision stands
                assert decs[m] == list(din), (step, m)
            else:                            # the lone plugin's recover_decision on the forward's targets
                want, _ = _recover(envs[m], 16, z[f"s{step}/sched"], list(din), False, rec.device,
                                   out["final_target"][m].tolist())
                assert decs[m] == want, (step, m)
    assert kept == {True, False}
    torch.cuda.synchronize()
    assert before == [t.cpu().numpy().tobytes() for t in (rec.tuner.P, rec.tuner.m, rec.tuner.v, rec.fpe_P,
                                                          rec.prototypes)]
    # set_fpe(1, ...) changes cell 1's outputs and no other cell's
    step = 0
    rec.setEnvironments([fake_env(z, step, extra["train_time_data"], z["schedule_series"]) for _ in range(M)])
    wins = np.stack([rec._input_window(m) for m in range(M)])
    h0 = np.stack([draw_h0(3000 + m) for m in range(M)])
    scheds = np.stack([z["s0/sched"]] * M)
    a = {k: v.copy() for k, v in rec.forward(wins, h0, scheds).items()}
    w12 = W.synth_fpe_weights(16, seed=12)
    rec.set_fpe(1, w12["fpe"], w12["prototypes"])
    b = {k: v.copy() for k, v in rec.forward(wins, h0, scheds).items()}
    for k in a:
        assert a[k][[0, 2]].tobytes() == b[k][[0, 2]].tobytes(), k
    assert a["scores"][1].tobytes() != b["scores"][1].tobytes() and a["any"][1] == 1 and b["any"][1] == 0
    lone = forward([dict(cell_arrays(ws[1]), P_fpe=FT.fpe_blob(w12["fpe"], H).numpy(),
                         prototypes=np.asarray(w12["prototypes"], dtype=np.float64).reshape(-1))],
                   wins[1:2], h0[1:2], scheds[1:2], lone=True)
    for k in b:
        assert b[k][1].tobytes() == lone[k][0].tobytes(), k
    with pytest.raises(ValueError):
        rec.set_fpe(3, w12["fpe"], w12["prototypes"])
