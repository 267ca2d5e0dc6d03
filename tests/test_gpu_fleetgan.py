"""GPU tests of the fleet's per-cell GAN step (``FleetTuner.train_gan``, the
cell-indexed entries pgp_gan_forward1_many / pgp_gan_step1_many, and the fleet
plugin ``PreGANPlusFleetRecovery``): every cell of a fleet
computes, byte for byte, what a lone ``Trainer`` + ``train_gan`` (and a lone
``PreGANPlusRecovery``) computes on that cell's weights and inputs — whatever
the fleet's size, the cell's position and the other cells do.  8 and 16 hosts,
16 prototypes."""
import numpy as np
import pytest
import torch

from preganplus_amd import _native
from preganplus_amd import simulate as SIM
from preganplus_amd import train as TR
from preganplus_amd import weights as W

pytestmark = pytest.mark.gpu
K = 16
GOLD = "tests/golden"


def cell_weights(H, seed):
    w = W.synth_weights(H, seed=seed)
    w["prototypes"] = np.random.default_rng(100 + seed).uniform(0.1, 0.9, (K, 2))
    return w


def gan_inputs(H, M, seed):
    """emb [M,H,2] (run_model's masked prototypes: some hosts zero), scheds [M,H,H]."""
    r = np.random.default_rng(seed)
    emb = r.uniform(0.1, 0.9, (M, H, 2)) * (r.uniform(size=(M, H, 1)) < 0.4)
    return emb.astype(np.float32), r.uniform(0, 1, (M, H, H))


def scripted(scores):
    """A simulator that returns the scripted scores in call order (the new schedule's first)."""
    it = iter(scores)
    return lambda sched: next(it)


def lone(H, w, **kw):
    return TR.Trainer(H, w, max_batch=1, **kw), TR.TuneState(w["prototypes"])


def sections(ft):
    go = int(ft._L.pgp_master_offset(ft.H, 1))
    return go, ft.slot_len


def snap_lone(tr, st=None):
    torch.cuda.synchronize()
    d = {"P": tr.P.cpu().numpy(), "m": tr.m.cpu().numpy(), "v": tr.v.cpu().numpy(),
         "steps": np.array([t["step"] for t in tr.tensors])}
    if st is not None:
        d["state"] = st.vector()
    return d


def snap_cell(ft, m, state=False):
    torch.cuda.synchronize()
    d = {"P": ft.P[m].cpu().numpy(), "m": ft.m[m].cpu().numpy(), "v": ft.v[m].cpu().numpy(),
         "steps": ft.sched.steps[m].copy()}
    if state:
        d["state"] = ft.states[m].vector()
    return d


def same(a, b, what=""):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), f"{what}: {k} differs"


def same_gan_result(a, b, what=""):
    """Two train_gan results (ns, new_score, orig_score, gen_loss, disc_loss), bit for bit."""
    assert a[0].dtype == b[0].dtype and a[0].shape == b[0].shape and a[0].tobytes() == b[0].tobytes(), f"{what}: ns"
    assert np.array(a[1:], dtype=np.float64).tobytes() == np.array(b[1:], dtype=np.float64).tobytes(), \
        f"{what}: {a[1:]} != {b[1:]}"


def pattern(t, k):
    """A sentinel pattern of t's shape and dtype that no computation produces by chance."""
    return (torch.arange(t.numel(), device=t.device, dtype=torch.float64) * 0.37 + k).to(t.dtype).view(t.shape)


# ---- 1. bytewise equal to lone runs ----

@pytest.mark.parametrize("H", [8, 16])
def test_fleet_equals_lone_runs(H):
    M = 5
    ws = [cell_weights(H, 10 + m) for m in range(M)]
    ft = TR.FleetTuner(H, ws)
    go, end = sections(ft)
    lones = [lone(H, ws[m])[0] for m in range(M)]
    # cell 4 starts from two lone GAN steps: non-zero step counts and moments
    e0, s0 = gan_inputs(H, 2, seed=900 + H)
    for i in range(2):
        TR.train_gan(lones[4], e0[i], s0[i], scripted([1.0 + i, 2.0 - i]), fused=True)
    ft.load_cell(4, lones[4], TR.TuneState(ws[4]["prototypes"]))
    same(snap_cell(ft, 4), snap_lone(lones[4]), "load_cell")
    assert ft.sched.steps[4].max() == 2
    # cell 3 is inactive: sentinels in everything of its slot, its workspace slot and its output rows
    active = [True, True, True, False, True]
    g = ft.gan_graph(False)
    guarded = (("P", ft.P), ("G", ft.G), ("m", ft.m), ("v", ft.v), ("gscr", g.gscr), ("ns", g.ns),
               ("probs", g.probs), ("probs_gen", g.probs_gen), ("probs_after", g.probs_after))
    for k, (_, t) in enumerate(guarded):
        t[3].copy_(pattern(t[3], k))
    before3 = {k: t[3].clone() for k, t in guarded}
    steps3 = ft.sched.steps[3].copy()
    ft.gan_probs_after[3] = (-3.0, -4.0)
    P0 = ft.P.cpu().numpy().copy()
    # labels mixed over cells and calls: new <= orig is "better" ([0,1]), else "worse" ([1,0])
    script = {0: [(1.0, 2.0), (3.0, 1.0), (2.0, 2.0)], 1: [(3.0, 1.0), (3.0, 1.5), (0.5, 2.0)],
              2: [(0.1, 0.2), (0.3, 0.2), (5.0, 1.0)], 4: [(2.5, 1.0), (1.0, 2.0), (4.0, 3.0)]}
    labels = set()
    for call in range(3):
        emb, scheds = gan_inputs(H, M, seed=50 * H + call)
        sims = [scripted(script[m][call]) if m in script else None for m in range(M)]
        res = ft.train_gan(emb, scheds, simulate=sims, active=active)
        Gf = ft.G.cpu().numpy()
        for m in (0, 1, 2, 4):
            want = TR.train_gan(lones[m], emb[m], scheds[m], scripted(script[m][call]), fused=True)
            same_gan_result(res[m], want, f"call {call} cell {m}")
            labels.add(tuple(TR.bce_target(want[1], want[2])))
            assert ft.gan_probs_after[m].tobytes() == np.asarray(lones[m].gan_probs_after).tobytes(), (call, m)
            same(snap_cell(ft, m), snap_lone(lones[m]), f"call {call} cell {m}")      # whole slots of P, m, v; counts
            assert Gf[m, go:].tobytes() == lones[m].G.cpu().numpy()[go:].tobytes(), (call, m)   # gen / disc sections
        # the inactive cell: untouched
        assert res[3] is None
        for k, t in guarded:
            assert torch.equal(t[3], before3[k]), k
        assert (ft.sched.steps[3] == steps3).all() and tuple(ft.gan_probs_after[3]) == (-3.0, -4.0)
    assert labels == {(0.0, 1.0), (1.0, 0.0)}
    P1 = ft.P.cpu().numpy()
    assert P1[:, :go].tobytes() == P0[:, :go].tobytes()           # no transformer section moved
    assert all(P1[m, go:].tobytes() != P0[m, go:].tobytes() for m in (0, 1, 2, 4))
    gan_cols = [i for i, t in enumerate(ft.tensors) if t["section"] in ("gen", "disc")]
    assert (ft.sched.steps[0, gan_cols] == 3).all() and (ft.sched.steps[4, gan_cols] == 5).all()


# ---- 2. position and size independence, through the raw entries; more cells than the device holds at once ----

def _raw_cells(H, n_seeds):
    """Per seed the arrays of one cell: slot (P, m, v), emb, sched, target, AdamW rows."""
    L = _native.lib()
    n = int(L.pgp_master_len(H))
    sel = {s: [t for t in TR.master_tensors(H) if t["section"] == s] for s in ("disc", "gen")}
    cells = []
    for j in range(n_seeds):
        r = np.random.default_rng(7 + j)
        P = W.pack_blob(cell_weights(H, 60 + j), H)[:n].astype(np.float32)
        e, s = gan_inputs(H, 1, seed=70 + j)
        step = 1.0 + 3 * j
        row = lambda lr: np.array([1.0, lr / (1 - 0.9 ** step), np.sqrt(1 - 0.999 ** step)], dtype=np.float32)
        cells.append({"P": P, "m": (r.normal(0, 1e-3, n) * (j > 0)).astype(np.float32),
                      "v": (r.uniform(0, 1e-5, n) * (j > 0)).astype(np.float32),
                      "emb": e[0].reshape(-1), "sched": s[0].astype(np.float32).reshape(-1),
                      "target": np.array([[0.0, 1.0], [1.0, 0.0], [0.0, 1.0]][j % 3], dtype=np.float32),
                      "tabD": np.tile(row(5e-5), (len(sel["disc"]), 1)),
                      "tabG": np.tile(row(4e-5), (len(sel["gen"]), 1))})
    desc = {s: (TR._AdamTensor * len(v))(*[TR._AdamTensor(t["offset"], t["n"], 1, 0.0, 0.0) for t in v])
            for s, v in sel.items()}
    return cells, desc, n


def _run_raw(H, cells, desc, idx, lone_entries):
    """The two entries on the fleet cells[idx[0]], cells[idx[1]], ... (the lone entries if ``lone_entries``:
    then idx has one cell).  Returns every array a cell owns, per slot."""
    L, dev = _native.lib(), "cuda"
    M = len(idx)
    up = lambda k: torch.from_numpy(np.stack([cells[j][k] for j in idx])).to(dev)
    P, m, v, emb, sched, target, tabD, tabG = (up(k) for k in ("P", "m", "v", "emb", "sched", "target", "tabD", "tabG"))
    G = torch.zeros_like(P)
    ws = torch.zeros((M, int(L.pgp_gan_workspace_len(H, 1))), dtype=torch.float32, device=dev)
    ns = torch.zeros((M, H * H), dtype=torch.float32, device=dev)
    probs, pg, pa = (torch.zeros((M, 2), dtype=torch.float32, device=dev) for _ in range(3))
    nD, nG = len(desc["disc"]), len(desc["gen"])
    p = lambda t: t.data_ptr()
    hyper = (5e-5, 4e-5, 1e-5, 0.9, 0.999, 1e-8)
    if lone_entries:
        assert M == 1
        _native.check(L.pgp_gan_forward1(H, p(emb), p(sched), p(P), p(ws), p(ns), p(probs), None), "forward1")
        _native.check(L.pgp_gan_step1(H, p(target), p(P), p(G), p(m), p(v), *hyper, desc["disc"], nD, p(tabD),
                                      desc["gen"], nG, p(tabG), p(ws), p(pg), p(pa), None), "step1")
    else:
        _native.check(L.pgp_gan_forward1_many(H, M, None, p(emb), p(sched), p(P), p(ws), p(ns), p(probs), None),
                      "forward1_many")
        _native.check(L.pgp_gan_step1_many(H, M, None, p(target), p(P), p(G), p(m), p(v), *hyper, desc["disc"], nD,
                                           p(tabD), 3 * nD, desc["gen"], nG, p(tabG), 3 * nG, p(ws), p(pg), p(pa),
                                           None), "step1_many")
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in (("P", P), ("G", G), ("m", m), ("v", v), ("ws", ws), ("ns", ns),
                                            ("probs", probs), ("probs_gen", pg), ("probs_after", pa))}


def test_position_and_size_independence():
    """The same cell at slot 0 of 1, slot 2 of 3 and the last slot of 600 (more than the 512 workgroups of 1,024
    threads 256 CUs hold at once: some queue) has the bits of the lone entries on its arrays; so has every other
    slot of the 600 (their contents repeat over three seeds)."""
    H = 8
    cells, desc, n = _raw_cells(H, 3)
    want = [_run_raw(H, cells, desc, [j], lone_entries=True) for j in range(3)]
    for j in range(3):
        assert want[j]["P"].tobytes() != cells[j]["P"].tobytes() and want[j]["ns"].any()   # the step did something
    for M in (1, 3, 600):
        idx = [2] if M == 1 else [c % 3 for c in range(M)]
        got = _run_raw(H, cells, desc, idx, lone_entries=False)
        last = M - 1
        assert idx[last] == 2
        for k, a in got.items():
            assert a[last].tobytes() == want[2][k][0].tobytes(), f"M={M}: {k} of the last slot"
        if M == 600:      # every slot (a superset of a spread sample), whole arrays at once
            for k, a in got.items():
                ref = np.concatenate([want[j][k] for j in range(3)])[idx]
                assert a.tobytes() == ref.tobytes(), f"M=600: {k}"


# ---- 3. envs= mode: the simulator on the device, one graph ----

ENV_SEEDS = (3, 4)     # synth_envs seeds of the two calls: with these both labels occur (asserted below)


def test_envs_mode_equals_simulate_mode():
    H, M = 16, 4
    active = [True, False, True, True]
    ws = [cell_weights(H, 80 + m) for m in range(M)]
    fa, fb = TR.FleetTuner(H, ws), TR.FleetTuner(H, ws)
    sim = SIM.Simulation(H)
    labels = set()
    for call in range(2):
        emb, scheds = gan_inputs(H, M, seed=300 + call)
        envs = SIM.synth_envs(M, H, seed=ENV_SEEDS[call])

        def score_on(c):   # Simulation.score on cell c's record alone; the schedule scored as the "new" one
            def f(s):
                x = np.asarray(s, dtype=np.float32)[None]
                return float(sim.score(envs[c:c + 1], x, x)[0][0, 1].item())
            return f

        ra = fa.train_gan(emb, scheds, envs=envs, active=active)
        rb = fb.train_gan(emb, scheds, simulate=[score_on(c) for c in range(M)], active=active)
        for m in range(M):
            if not active[m]:
                assert ra[m] is None and rb[m] is None
                continue
            same_gan_result(ra[m], rb[m], f"call {call} cell {m}")
            labels.add(tuple(TR.bce_target(ra[m][1], ra[m][2])))
            assert fa.gan_probs_after[m].tobytes() == fb.gan_probs_after[m].tobytes()
            same(snap_cell(fa, m), snap_cell(fb, m), f"call {call} cell {m}")
        assert torch.equal(fa.P, fb.P) and torch.equal(fa.m, fb.m) and torch.equal(fa.v, fb.v)
        assert torch.equal(fa.G, fb.G)
    assert labels == {(0.0, 1.0), (1.0, 0.0)}, "the chosen records must give both label outcomes"
    assert (fa.sched.steps == fb.sched.steps).all()
    assert not fa.gan_graph(True).ns[1].any()          # the inactive cell's ns rows: zero as allocated


# ---- 4. the captured graphs equal the eager sequence of the two entries ----

def test_graph_equals_eager():
    H, M = 16, 3
    ws = [cell_weights(H, 90 + m) for m in range(M)]
    fg, fe = TR.FleetTuner(H, ws), TR.FleetTuner(H, ws)
    fe.gan_capture = False
    for call in range(2):
        emb, scheds = gan_inputs(H, M, seed=400 + call)
        sc = [(1.0, 2.0), (2.0, 1.0), (1.0 + call, 1.5)]
        rg = fg.train_gan(emb, scheds, simulate=[scripted(s) for s in sc])
        re_ = fe.train_gan(emb, scheds, simulate=[scripted(s) for s in sc])
        for m in range(M):
            same_gan_result(rg[m], re_[m], f"call {call} cell {m}")
        for k in ("P", "G", "m", "v"):
            assert torch.equal(getattr(fg, k), getattr(fe, k)), (call, k)
        assert fg.gan_probs_after.tobytes() == fe.gan_probs_after.tobytes()
    assert fg.gan_graph(False).graphs is not None and fe.gan_graph(False).graphs is None


# ---- 5. interleaved with tuning: the sections and counts stay apart ----

def test_interleaved_with_tuning():
    H, M, n = 16, 3, 2
    ws = [cell_weights(H, 110 + m) for m in range(M)]
    ft = TR.FleetTuner(H, ws)
    lones = [lone(H, ws[m]) for m in range(M)]
    r = np.random.default_rng(5)
    for call in range(2):
        wins = r.uniform(0, 1, (M, n, 3, 3 * H)).astype(np.float32)
        anom = (r.uniform(size=(M, n, H)) < 0.25).astype(np.int32)
        anom[:, 0, 1] = 1
        cls = r.integers(0, 3, (M, n, H)).astype(np.int32)
        emb, scheds = gan_inputs(H, M, seed=500 + call)
        sc = [(1.0, 2.0), (2.0, 1.0), (3.0, 3.0)]
        rt = ft.tune(wins, anom, cls)
        rg = ft.train_gan(emb, scheds, simulate=[scripted(s) for s in sc])
        for m in range(M):
            tr, st = lones[m]
            (la, sa), (lb, sb) = rt[m], TR.backprop(tr, st, wins[m], anom[m], cls[m], score=True)
            assert np.array(la).tobytes() == np.array(lb).tobytes() and np.array(sa).tobytes() == np.array(sb).tobytes()
            same_gan_result(rg[m], TR.train_gan(tr, emb[m], scheds[m], scripted(sc[m]), fused=True), f"{call} {m}")
            same(snap_cell(ft, m, state=True), snap_lone(tr, st), f"call {call} cell {m}")
    for m in range(M):
        tr, st = ft.trainer(m)
        same(snap_lone(tr, st), snap_lone(*lones[m]), f"trainer({m})")


# ---- 6. the fleet plugin against lone plugins ----

def test_fleet_plugin_equals_lone_plugins():
    from preganplus_amd.recovery import PreGANPlusFleetRecovery, PreGANPlusRecovery
    from tests.test_train_oracle_golden import fake_env
    H, M = 16, 3
    w, extra = W.load_npz("preganplus_amd/data/simulator_16.npz")
    z = np.load(f"{GOLD}/plugin_h16.npz")
    tt = extra["train_time_data"]
    w2 = W.synth_weights(H, 123)
    w2["prototypes"] = np.random.default_rng(9).uniform(0.1, 0.9, np.asarray(w["prototypes"]).shape)
    weights, extras = [w, w, w2], [extra, extra, {"train_time_data": tt}]
    fleet = PreGANPlusFleetRecovery(H, weights, extras, training=True)
    lones = [PreGANPlusRecovery(H, "", training=True, weights=weights[m], extra=extras[m], save_folder=None)
             for m in range(M)]
    ft = fleet.tuner

    def env_of(step, calls):
        env = fake_env(z, step, tt, z["schedule_series"])
        run = env.stats.runSimulation

        def counted(s):
            calls.append(step)
            return run(s)
        env.stats.runSimulation = counted
        return env

    gan_calls0 = []
    for i in range(4):
        steps = [(m + i) % 4 for m in range(M)]
        decisions = [[tuple(x) for x in z[f"s{s}/decision_in"]] for s in steps]
        before = [snap_cell(ft, m) for m in range(M)]
        seen = []
        fleet.setEnvironments([env_of(steps[m], seen if m == 0 else []) for m in range(M)])
        got = fleet.run_model(decisions)
        gan_calls0.append(len(seen))
        for m in range(M):
            lp = lones[m]
            lp.setEnvironment(env_of(steps[m], []))
            n_acc = len(lp.accuracy_list)
            try:
                want = lp.run_model(None, decisions[m])
            except ZeroDivisionError:
                assert type(got[m]) is ZeroDivisionError, (i, m)
            else:
                assert [tuple(map(int, d)) for d in got[m]] == [tuple(map(int, d)) for d in want], (i, m)
                if len(lp.accuracy_list) == n_acc:       # the no-anomaly early return: the slot is untouched
                    assert got[m] is decisions[m]
                    same(snap_cell(ft, m), before[m], f"call {i} cell {m}: early return")
            assert len(fleet.accuracy_list[m]) == len(lp.accuracy_list), (i, m)
            for a, b in zip(fleet.accuracy_list[m], lp.accuracy_list):
                assert np.asarray(a, dtype=np.float64).tobytes() == np.asarray(b, dtype=np.float64).tobytes(), (i, m)
            assert fleet.epoch[m] == lp.epoch
            assert fleet.classes[m] == getattr(lp, "classes", None)
            assert fleet.hosts_from[m] == getattr(lp, "hosts_from", None)
            same(snap_cell(ft, m, state=True), snap_lone(lp.trainer, lp.tune_state), f"call {i} cell {m}")
            assert fleet.prototypes[m].tobytes() == lp.tune_state.protos.tobytes()
    # cell 0 went through the GAN step in all four calls: both recorded simulator scores consumed each time
    assert gan_calls0 == [2, 2, 2, 2]
    assert fleet.epoch[0] == int(extra["meta/gen/epoch"]) + 4


# ---- 7. refusals ----

def test_other_host_counts_are_refused():
    from preganplus_amd.recovery import PreGANPlusFleetRecovery
    L = _native.lib()
    buf = torch.zeros(1 << 16, dtype=torch.float32, device="cuda")
    p = buf.data_ptr()
    desc = (TR._AdamTensor * 1)(TR._AdamTensor(0, 1, 1, 0.0, 0.0))
    with pytest.raises(_native.NativeError):
        _native.check(L.pgp_gan_forward1_many(50, 1, None, p, p, p, p, p, p, None), "pgp_gan_forward1_many")
    with pytest.raises(_native.NativeError):
        _native.check(L.pgp_gan_step1_many(50, 1, None, p, p, p, p, p, 5e-5, 5e-5, 1e-5, 0.9, 0.999, 1e-8, desc, 1, p,
                                           3, desc, 1, p, 3, p, p, p, None), "pgp_gan_step1_many")
    torch.cuda.synchronize()
    assert not buf.any()
    with pytest.raises(ValueError):
        PreGANPlusFleetRecovery(50, [{}], [None])
