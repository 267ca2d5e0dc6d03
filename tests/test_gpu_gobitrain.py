"""GPU: the training of GOBI's surrogate (csrc/pgp_gobitrain.hip through the
C-ABI and preganplus_amd/gobitrain.py) against the reference's own runs
(tests/golden/gobitrain_h16*.npz) and the restatement (tests/gobitrain_ref.py).

The trajectory bound is per tensor 8 x the max-abs deviation of the reference's
own fp32 run from its fp64 run at the same step count, as the fixture script
measured it (bound/{p,m,v}/n{1,8,64} in the fixture; DESIGN §20 lists them).
Every test is the fixed 61,890-parameter model over at most 159 steps."""
import numpy as np
import pytest
import torch

from tests import gobitrain_ref as R

pytestmark = pytest.mark.gpu
OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -2


def close(got, want, rel, abs_scale, what=""):
    """fp32 HIP vs fp64 reference: |got - want| <= rel*|want| + abs_scale*max|want|."""
    want = np.asarray(want, dtype=np.float64)
    got = np.asarray(got, dtype=np.float64)
    tol = rel * np.abs(want) + abs_scale * (np.abs(want).max() + 1e-30)
    bad = np.abs(got - want) > tol
    assert not bad.any(), f"{what}: {bad.sum()} of {bad.size} off, max err {np.abs(got - want).max():.3e}"


@pytest.fixture(scope="module")
def z():
    return R.fixture()


def _trainer(z, **kw):
    from preganplus_amd.gobitrain import GOBITrainer
    t = GOBITrainer(weights=R.initial(z), **kw)
    t.set_data(z["feats"], z["targets"])
    return t


def _state(t):
    return [a.cpu().numpy().copy() for a in (t.P, t.m, t.v)]


def test_gradient_alone(z):
    """One step from zero moments: exp_avg / (1 - beta1) is the gradient
    (L2 included): against fp64 autograd + wd p, on a sample with unplaced
    containers (all-zero one-hot rows), a full one and the order's first."""
    for s in (int(z["sample_unplaced"]), int(z["sample_full"]), int(z["order"][0])):
        t = _trainer(z)
        loss = t.backprop([s])
        P = {k: torch.tensor(z["w0/" + k], dtype=torch.float64, requires_grad=True) for k in R.ORDER}
        x = torch.tensor(z["feats"][s], dtype=torch.float32).double().flatten()
        y = torch.tensor(z["targets"][s]).double()
        ref = R.loss_of(P, x, y)
        ref.backward()
        np.testing.assert_allclose(loss[0], float(ref.detach()), rtol=1e-4)
        got = R.unblob(t.m.cpu().numpy().astype(np.float64) / (1 - 0.9))
        for k in R.ORDER:
            want = P[k].grad.numpy() + 1e-5 * P[k].detach().numpy()
            close(got[k], want, rel=1e-3, abs_scale=1e-4, what=f"sample {s} {k}")


@pytest.mark.parametrize("n", R.STEPS)
def test_trajectory_against_the_reference_fp64(z, n):
    t = _trainer(z)
    loss = t.backprop(z["order"][:n])
    assert t.step == n
    np.testing.assert_allclose(loss, z["loss_f64"][:n], rtol=1e-4)
    for kind, got, want in zip("pmv", _state(t), R.snapshot("f64", n, z)):
        err, b = np.abs(got.astype(np.float64) - want), R.bounds(z, kind, n)
        worst = (err / b).reshape(-1)
        print(f"n={n} {kind}: worst err/bound per tensor",
              " ".join(f"{worst[R.OFFS[j]:R.OFFS[j + 1]].max():.2f}" for j in range(len(R.ORDER))))
        assert np.all(err <= b), (kind, n, R.ORDER[int(np.searchsorted(R.OFFS, int(worst.argmax()), "right")) - 1],
                                  float(worst.max()))


def test_launch_equivalence_and_determinism(z):
    """One launch of n steps == n launches of one step, bytewise in P, m, v and
    the losses; a second run gives the same bits."""
    order = z["order"][:24]
    a = _trainer(z)
    la = a.backprop(order)
    b = _trainer(z)
    lb = np.concatenate([b.backprop([s]) for s in order[:5]] + [b.backprop(order[5:7]), b.backprop(order[7:])])
    c = _trainer(z)
    lc = c.backprop(order)
    for x, y, w in zip(_state(a) + [la], _state(b) + [lb], _state(c) + [lc]):
        assert x.tobytes() == y.tobytes()
        assert x.tobytes() == w.tobytes()


def test_resume_from_checkpoint(z):
    """train n, checkpoint, new trainer from it, train n == train 2n, bytewise."""
    from preganplus_amd.gobitrain import GOBITrainer
    order, n = z["order"], 12
    a = _trainer(z)
    a.backprop(order[:n])
    ck = a.checkpoint(0, [])
    b = GOBITrainer(weights={k: v.numpy() for k, v in ck["model_state_dict"].items()},
                    state=ck["optimizer_state_dict"])
    assert b.step == n
    b.set_data(z["feats"], z["targets"])
    lb = b.backprop(order[n:2 * n])
    c = _trainer(z)
    lc = c.backprop(order[:2 * n])
    assert lb.tobytes() == lc[n:].tobytes()
    for x, y in zip(_state(b), _state(c)):
        assert x.tobytes() == y.tobytes()
    opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(R.SHAPES[k])) for k in R.ORDER], lr=1e-4, weight_decay=1e-5)
    opt.load_state_dict(c.checkpoint(1, [(0.1, 0.2)])["optimizer_state_dict"])


def test_accuracy_losses(z):
    """accuracy(order) against the restatement, and independent of how the
    samples are split over launches / workgroups."""
    t = _trainer(z)
    t.backprop(z["order"][:8])
    w = t.weights_numpy()
    idx = np.arange(199)
    got = t.accuracy(idx)
    np.testing.assert_allclose(got, R.losses(w, z["feats"], z["targets"], idx), rtol=1e-5)
    part = np.concatenate([t.accuracy(idx[:1]), t.accuracy(idx[1:41]), t.accuracy(idx[41:])])
    assert part.tobytes() == got.tobytes()
    perm = np.random.Generator(np.random.PCG64(3)).permutation(199)
    assert t.accuracy(perm).tobytes() == got[perm].tobytes()
    assert t.accuracy([]).shape == (0,)


def test_two_epochs_through_train(z):
    """train() under the fixture's seed: the reference's shuffles exactly, its
    accuracy_list within the loss tolerance."""
    import random

    from preganplus_amd.gobitrain import GOBITrainer
    t = GOBITrainer(seed=int(z["init_seed"]))
    for k, a in t.weights_numpy().items():
        assert np.array_equal(a, z["w0/" + k]), k
    random.seed(int(z["epoch_seed"]))
    acc = t.train(z["feats"], z["targets"], 2)
    assert np.array_equal(np.array(t.orders), z["epoch_orders"])
    assert t.step == 2 * 159
    np.testing.assert_allclose(np.array(acc), z["accuracy_list"], rtol=1e-4)


def test_trained_weights_are_consumed_by_gobi(z):
    """The trained surrogate in GOBIOptimizer / GOBIScheduler: one optimiser
    step on gobi_h16.npz's first inits agrees with the oracle run with the same
    weights, by test_gpu_gobi.py's comparison, and differs from the shipped
    weights' result."""
    import random

    from oracle import gobi_oracle as GO
    from preganplus_amd.gobi import GOBIOptimizer, GOBIScheduler
    from preganplus_amd.gobitrain import GOBITrainer
    t = GOBITrainer(seed=int(z["init_seed"]))
    random.seed(int(z["epoch_seed"]))
    t.train(z["feats"], z["targets"], 2)
    w = t.weights_numpy()
    sd = {k: torch.tensor(w[k]) for k in R.ORDER}
    inits = np.load("tests/golden/gobi_h16.npz")["inits"][:24]
    g = GOBIOptimizer(weights=w)
    pre = torch.empty((len(inits), 16, 16), device="cuda")
    res, its, _ = g.optimize(inits, max_iters=1, pre=pre)
    res, pre = res.cpu().numpy(), pre.cpu().numpy()
    shipped = GOBIOptimizer()
    pre0 = torch.empty((len(inits), 16, 16), device="cuda")
    shipped.optimize(inits, max_iters=1, pre=pre0)
    assert np.abs(pre - pre0.cpu().numpy()).max() > 1e-2
    robust = agree = near = 0
    worst = 0.0
    for i in range(len(inits)):
        r_ref, _, _, p_ref = GO.opt(sd, inits[i], max_it=1, return_pre=True)
        d = np.abs(pre[i] - p_ref)
        near += int(np.sum(d <= 1e-6 + 1e-5 * np.abs(p_ref)))
        worst = max(worst, float(d.max()))
        top2 = np.sort(p_ref, axis=1)[:, -2:]
        for c in range(16):
            if top2[c, 1] - top2[c, 0] > 2 * d[c].max() + 1e-7:
                robust += 1
                agree += int(np.array_equal(res[i][c], r_ref[c]))
    n = len(inits)
    assert near >= 0.995 * n * 256, near
    assert worst <= 1e-3, worst
    assert robust > 0.5 * n * 16, robust
    assert agree == robust, f"{robust - agree} of {robust} robust rows disagree"
    sch = GOBIScheduler(weights=w, max_ips=float(z["max_ips"]))
    assert sch.max_container_ips == float(z["max_ips"])
    with pytest.raises(ValueError):
        GOBIScheduler(weights=w)
    with pytest.raises(ValueError):
        GOBIScheduler("energy_latency_50", weights=w, max_ips=1.0)


def test_argument_checks_on_the_device(z):
    """Unsupported host counts and bad arguments return before any launch and
    n = 0 leaves P, m, v untouched."""
    t = _trainer(z)
    before = _state(t)
    L, o = t._L, torch.zeros(4, dtype=torch.int32, device="cuda")
    loss = torch.zeros(4, device="cuda")

    def steps(H=16, n=2, step0=0, lr=1e-4, b1=0.9, b2=0.999):
        return L.pgp_gobi_train_steps(H, t.n_samples, n, t.feats.data_ptr(), t.targets.data_ptr(), o.data_ptr(),
                                      t.P.data_ptr(), t.m.data_ptr(), t.v.data_ptr(), step0, lr, 1e-5, b1, b2, 1e-8,
                                      loss.data_ptr(), None)
    assert steps(H=8) == ERR_UNSUPPORTED and steps(H=50) == ERR_UNSUPPORTED
    for kw in (dict(n=-1), dict(lr=0.0), dict(lr=-1.0), dict(b1=1.0), dict(b2=-0.5), dict(step0=-1)):
        assert steps(**kw) == ERR_ARG, kw
    assert steps(n=0) == OK
    assert t.backprop([]).shape == (0,)
    torch.cuda.synchronize()
    for x, y in zip(before, _state(t)):
        assert x.tobytes() == y.tobytes()
    with pytest.raises(IndexError):
        t.backprop([199])
