"""Second-order GOBI on the GPU (pgp_gobi_so_optimize / _groups, csrc/pgp_gobi_so.hip)
against the fp64 statement of so_opt() in tests/sogobi_ref.py and the reference's
own runs in tests/golden/sogobi_h16.npz.  Explicit probes unless said otherwise.

Tolerances (sogobi_ref.py): g and hv within TOL_G / TOL_HV = 4 x the reference's
own fp32 error against fp64 (test_sogobi_oracle.py measures it), max-normalised
per environment; decisions are compared where the fp64 top-2 gap exceeds what
such an error can move (Trajectory64.margin)."""
import functools

import numpy as np
import pytest
import torch

import sogobi_ref as S
from oracle import gobi_oracle as GO

pytestmark = pytest.mark.gpu
ULP = 2.0 ** -23      # fp32's unit roundoff step relative to a magnitude: "1 ulp at magnitude m" is ULP * m
TINY = 2.0 ** -149    # fp32's smallest spacing: a moment held in fp32 is never finer


@functools.lru_cache(maxsize=None)
def optimizer():
    from preganplus_amd.gobi import GOBIOptimizer
    return GOBIOptimizer()


def run(inits, signs=None, seeds=None, max_iters=0, taps=True, opt=None, **kw):
    """optimize_so -> (result, iterations, fitness, taps) as numpy."""
    g = opt or optimizer()
    E = len(inits)
    tp = torch.full((E, 3, 16, 18), float("nan"), device="cuda") if taps else None
    res, its, fit = g.optimize_so(inits, signs=signs, seeds=seeds, max_iters=max_iters, taps=tp, **kw)
    torch.cuda.synchronize()
    return res.cpu().numpy(), its.cpu().numpy(), fit.cpu().numpy(), (tp.cpu().numpy() if taps else None)


@functools.lru_cache(maxsize=None)
def stepped():
    """The 240 fixture inits and 96 non-one-hot ones (the dense layer-1 value
    path at iteration 0), stopped after 1, 2 and 3 steps, with the fp64 trajectory."""
    f = S.fixture()
    sd, _ = GO.load(S.WEIGHTS)
    inits = np.concatenate([f["inits"], S.non_one_hot_inits(96)])
    signs = np.concatenate([f["signs"], f["signs"][:96]])
    T = S.Trajectory64(sd, inits, signs, max_it=3, keep=3)
    return inits, T, [run(inits, signs, max_iters=s) for s in (1, 2, 3)]


@functools.lru_cache(maxsize=None)
def full():
    f = S.fixture()
    return run(f["inits"], f["signs"], taps=False)


def agreed(T, gpu, s):
    """Environments whose projections of steps 1..s equal the fp64 trajectory's."""
    ok = np.ones(len(T.result), bool)
    for k in range(s):
        ok &= (gpu[k][0].astype(np.float64) == T.after[k]).all((1, 2))
    return ok


def test_g_and_hv_at_steps_1_2_3():
    """The tapped g and hv of the last executed step against fp64, all 288
    entries, for the environments whose earlier projections agreed with it."""
    inits, T, gpu = stepped()
    for s in range(3):
        ok = agreed(T, gpu, s)
        tp = gpu[s][3]
        assert np.isfinite(tp).all()
        eg, eh = S.max_normalised(tp[:, 0], T.g[s])[ok], S.max_normalised(tp[:, 1], T.hv[s])[ok]
        print(f"step {s + 1}: {ok.sum()} of {len(ok)} compared; g {eg.max():.3e} (tol {S.TOL_G:.2e})  "
              f"hv {eh.max():.3e} (tol {S.TOL_HV:.2e}); non-one-hot g {eg[ok[:240].sum():].max():.3e}")
        assert ok.sum() >= len(ok) // 2
        assert eg.max() <= S.TOL_G and eh.max() <= S.TOL_HV


def replay_pre(x_prev, gs, hvs):
    """fp64 Adahessian step len(gs) from the steps' g and hv: (pre, magnitude of its larger term)."""
    lrs = GO.cosine_lrs()
    t = len(gs)
    m = sum(0.9 ** (t - 1 - k) * 0.1 * g for k, g in enumerate(gs))
    ma = sum(0.9 ** (t - 1 - k) * 0.1 * np.abs(g) for k, g in enumerate(gs))
    s = sum(0.999 ** (t - 1 - k) * 0.001 * hv * hv for k, hv in enumerate(hvs))
    bc1 = 1 - 0.9 ** t
    denom = np.sqrt(s) / np.sqrt(1 - 0.999 ** t) + S.EPS
    pre = x_prev - lrs[t - 1] * (m / bc1 / denom)
    return pre, np.maximum(np.abs(x_prev), lrs[t - 1] * (ma / bc1 / denom)), lrs[t - 1] / (bc1 * S.EPS)


def test_update_replayed_from_the_kernels_own_taps():
    """Step 1: the tapped pre against x - 0.8 g / (|hv| + 1e-4) evaluated in fp64
    on the tapped g and hv, within 4 ulp at the magnitude of the larger term
    (ulp at magnitude m: 2^-23 m; the reference's own fp32 step 1 is within 2.6
    of its own g and hv).  Step 3: the same from the three steps' taps; the
    magnitude there is that of x or of the update with |g| in place of g, so
    that steps cancelling in the first moment do not shrink it.  Below fp32's
    normal range a moment is no finer than 2^-149, which the step multiplies
    by at most lr / (bc1 eps): that much per ulp is allowed on top (the
    saturated environments' gradients are subnormal, and the reference's own
    step is 2.4e4 spacings off there).  The projection is the first-argmax
    one-hot of the tapped pre exactly, and the cpu / ips columns are the
    init's bytes."""
    inits, T, gpu = stepped()
    a = slice(2, 18)
    x = [inits.astype(np.float64)] + [gpu[k][0].astype(np.float64) for k in range(3)]
    g = [gpu[k][3][:, 0].astype(np.float64) for k in range(3)]
    hv = [gpu[k][3][:, 1].astype(np.float64) for k in range(3)]
    for s, n_ulp in ((1, 4.0), (3, 4.0)):
        pre, big, gain = replay_pre(x[s - 1], g[:s], hv[:s])
        got = gpu[s - 1][3][:, 2].astype(np.float64)
        err = (np.abs(got - pre) / (ULP * big + TINY * gain))[:, :, a]
        print(f"step {s}: pre against its fp64 replay, worst {err.max():.2f} ulp (allowed {n_ulp})")
        assert err.max() <= n_ulp
        res = gpu[s - 1][0]
        tapped = torch.tensor(gpu[s - 1][3][:, 2][:, :, a])
        want = np.zeros_like(res[:, :, a])
        np.put_along_axis(want, torch.stack([GO.first_argmax(r) for r in tapped]).numpy()[:, :, None], 1.0, axis=2)
        assert np.array_equal(res[:, :, a], want)
        assert res[:, :, :2].tobytes() == inits[:, :, :2].tobytes()
        assert np.array_equal(gpu[s - 1][3][:, 2][:, :, :2], x[s - 1][:, :, :2].astype(np.float32))   # the restored columns
        assert (gpu[s - 1][1] == s).all()    # no environment stops before step 31


def test_decisions_at_step_1():
    """Every row whose fp64 top-2 gap exceeds 2 max_row(B) takes the fp64 one-hot;
    at least 90 % of the fixture's rows are such (the fp64 trajectories give 96.5 %)."""
    inits, T, gpu = stepped()
    rob = T.robust_rows1.numpy()
    same = (gpu[0][0][:, :, 2:].astype(np.float64) == T.after[0][:, :, 2:]).all(2)
    print(f"robust rows at step 1: {rob[:240].sum()} of 3840 (fixture), {rob[240:].sum()} of {rob[240:].size} "
          f"(non-one-hot); rows equal to fp64: {same.sum()} of {same.size}")
    assert rob[:240].sum() >= 0.9 * 3840
    assert same[rob].all()


def test_end_to_end_against_the_fixture():
    """Full runs on the reference's probes.  An environment whose every row of
    every fp64 step is robust (Trajectory64.qualifies; at least 40 % must be)
    ends in the fixture's schedule with its iteration count, exactly.  All 240:
    valid schedules, the stop rule, fitness = the surrogate of the result, and
    the fitness / iteration statistics of the fixture."""
    f, T = S.fixture(), S.fixture_trajectory()
    res, its, fit, _ = full()
    q = T.qualifies
    hit = (res == f["results"]).all((1, 2)) & (its == f["iterations"])
    print(f"qualifying: {q.sum()} of 240, equal to the fixture among them: {hit[q].sum()}; among all: {hit.sum()}")
    assert q.sum() >= 0.4 * 240
    assert hit[q].all()
    assert res[:, :, :2].tobytes() == f["inits"][:, :, :2].tobytes()
    alloc = res[:, :, 2:]
    assert np.all((alloc == 0) | (alloc == 1)) and np.all(alloc.sum(-1) == 1)
    assert np.all((its >= 30) & (its <= 200))
    sd, _ = GO.load(S.WEIGHTS)
    want = np.array([float(GO.surrogate(sd, torch.tensor(res[i]))) for i in range(240)])
    rel = np.abs(fit - want) / np.abs(want)
    print(f"fitness against the surrogate of the result, all 240: worst relative {rel.max():.2e} (rtol 1e-5)")
    assert rel.max() <= 1e-5
    assert abs(np.mean(fit) - np.mean(f["fitness"])) <= 0.15 * np.mean(f["fitness"])
    assert abs(np.mean(its) - np.mean(f["iterations"])) <= 0.25 * np.mean(f["iterations"])


def test_batch_invariance_and_ragged():
    """An environment's bits do not depend on the batch, its position or its
    workgroup partner: 7 alone, 100..102 and 0..64 give the full batch's; E = 0 works."""
    f = S.fixture()
    res, its, fit, _ = full()
    for sel in ([7], [100, 101, 102], list(range(65))):
        r, i, t, _ = run(f["inits"][sel], f["signs"][sel], taps=False)
        assert r.tobytes() == res[sel].tobytes() and np.array_equal(i, its[sel]) and t.tobytes() == fit[sel].tobytes()
    r, i, t, _ = run(f["inits"][:0], f["signs"][:0], taps=False)
    assert r.shape == (0, 16, 18) and i.shape == (0,)
    # the taps are per environment too (an odd batch: the last workgroup has one)
    r3 = run(f["inits"][:3], f["signs"][:3], max_iters=2)
    r1 = run(f["inits"][2:3], f["signs"][2:3], max_iters=2)
    assert r3[3][2].tobytes() == r1[3][0].tobytes() and r3[0][2].tobytes() == r1[0][0].tobytes()


def test_grouped_form():
    """Three surrogates (the packaged one and two perturbed copies), model_of
    interleaved: each environment has the bits of the plain entry on a
    one-model handle of its surrogate; a padded group, inert slots and an
    environment no group names (its sentinel rows stay)."""
    from preganplus_amd.gobi import GOBIOptimizer, load_weights
    f = S.fixture()
    w0, _ = load_weights()
    rng = np.random.Generator(np.random.PCG64(8))
    ws = [w0] + [{k: (v * (1 + 0.05 * rng.standard_normal(v.shape))).astype(np.float32) for k, v in w0.items()}
                 for _ in range(2)]
    E = 11
    inits, signs = f["inits"][40:40 + E], f["signs"][40:40 + E]
    model_of = np.arange(E) % 3                        # models 0, 1: 4 environments; model 2: 3 (a padded group)
    fleet = GOBIOptimizer(ws)
    want = [None] * E
    for m in range(3):
        one = GOBIOptimizer(ws[m])
        sel = np.nonzero(model_of == m)[0]
        r = run(inits[sel], signs[sel], opt=one, max_iters=40)
        for k, e in enumerate(sel):
            want[e] = [a[k] for a in r]
        one.close()
    got = run(inits, signs, opt=fleet, model_of=model_of, max_iters=40)
    for e in range(E):
        for a, b in zip(got, want[e]):
            assert np.asarray(a[e]).tobytes() == np.asarray(b).tobytes(), e
    # a hand-made table: environment 4 unnamed, a model outside the handle, an id outside the batch, a repeat
    table = torch.tensor([[0, 0, 3, -1, 0], [1, 1, 99, 7, -1], [2, 2, 5, 8, -1], [3, 4, -1, -1, -1],
                          [1, -1, -1, 10, -1]], dtype=torch.int32, device="cuda")
    named = {0: [0, 3], 1: [1, 7, 10], 2: [2, 5, 8]}
    tp = torch.full((E, 3, 16, 18), -7.0, device="cuda")
    out = (torch.full((E, 16, 18), -7.0, device="cuda"), torch.full((E,), -7, dtype=torch.int32, device="cuda"),
           torch.full((E,), -7.0, device="cuda"))
    fleet.optimize_so(inits, out=out, signs=signs, max_iters=40, taps=tp, groups=table)
    torch.cuda.synchronize()
    got = [t.cpu().numpy() for t in out] + [tp.cpu().numpy()]
    hit = sorted(e for es in named.values() for e in es)
    for e in range(E):
        if e in hit:
            for a, b in zip(got, want[e]):
                assert np.asarray(a[e]).tobytes() == np.asarray(b).tobytes(), e
        else:
            assert all((np.asarray(a[e]) == -7).all() for a in got), e
    fleet.close()


def test_generated_signs():
    """seeds gives the bits of the explicit path fed so_signs(seeds, 200), and an
    environment's result does not depend on the other environments' seeds."""
    from preganplus_amd.gobi import so_signs
    f = S.fixture()
    inits = f["inits"][200:217]
    seeds = np.array([3, 2 ** 63 + 11, 0] + list(range(100, 114)), dtype=np.uint64)
    a = run(inits, seeds=seeds)
    b = run(inits, signs=so_signs(seeds, 200))
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    d = run(inits, seeds=torch.tensor(seeds.view(np.int64), device="cuda"))   # device-resident seeds, used in place
    for x, y in zip(a, d):
        assert x.tobytes() == y.tobytes()
    other = seeds.copy()
    other[1:] += np.uint64(1000)
    c = run(inits, seeds=other)
    for x, z in zip(a, c):
        assert x[0].tobytes() == z[0].tobytes()
    assert any(not np.array_equal(a[3][e], c[3][e]) for e in range(1, 17))   # the seed does reach the probes
    alloc = a[0][:, :, 2:]
    assert np.all((alloc == 0) | (alloc == 1)) and np.all(alloc.sum(-1) == 1) and np.all((a[1] >= 30) & (a[1] <= 200))


def test_sogobi_scheduler_run():
    """SOGOBIScheduler.run_GOBI on a duck-typed environment: result_cache and the
    decision list are consistent with optimize_so under the call's seed."""
    from preganplus_amd.gobi import SOGOBIScheduler
    sch = SOGOBIScheduler(seed=5)
    rng = np.random.Generator(np.random.PCG64(12))
    for trial in range(2):
        env = S.duck_env(rng, sch.max_container_ips)
        sch.setEnvironment(env)
        np.random.seed(trial)
        dec = sch.run_GOBI()
        np.random.seed(trial)
        init, prev = sch.init_matrix()
        res, _, _ = sch.opt.optimize_so(init[None], seeds=[sch.call_seed(trial)])
        res = res[0].cpu().numpy()
        assert np.array_equal(sch.result_cache, res[:, -16:])
        assert dec == GO.decision(res, prev) and sch.calls == trial + 1
