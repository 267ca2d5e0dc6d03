"""GPU tests of the fleet tuner (``FleetTuner``, preganplus_amd/train.py; the
cell-indexed entries pgp_tune_step1_many / pgp_adamw_table_many /
pgp_tune_forward_cells / pgp_forward1_many): every cell of a
fleet computes, byte for byte, what a lone ``Trainer`` + ``backprop`` computes
on that cell's weights and windows — whatever the fleet's size, the cell's
position and the other cells do.  8 and 16 hosts, 16 prototypes."""
import ctypes

import numpy as np
import pytest
import torch

from preganplus_amd import _native
from preganplus_amd import train as TR
from preganplus_amd import weights as W

pytestmark = pytest.mark.gpu
K = 16
SENT = -7.25          # sentinel for buffers nothing may write


def cell_weights(H, seed):
    w = W.synth_weights(H, seed=seed)
    w["prototypes"] = np.random.default_rng(100 + seed).uniform(0.1, 0.9, (K, 2))
    return w


def data(H, M, n, seed, no_positive=()):
    """wins [M,n,3,3H], anom / cls [M,n,H]: every cell but those in no_positive has a positive label in window 0."""
    r = np.random.default_rng(seed)
    wins = r.uniform(0, 1, (M, n, 3, 3 * H)).astype(np.float32)
    anom = (r.uniform(size=(M, n, H)) < 0.25).astype(np.int32)
    anom[:, 0, 1] = 1
    for m in no_positive:
        anom[m] = 0
    cls = r.integers(0, 3, (M, n, H)).astype(np.int32)
    return wins, anom, cls


def lone(H, w, **kw):
    return TR.Trainer(H, w, max_batch=1, **kw), TR.TuneState(w["prototypes"])


def snap_lone(tr, st):
    torch.cuda.synchronize()
    return {"P": tr.P.cpu().numpy(), "m": tr.m.cpu().numpy(), "v": tr.v.cpu().numpy(), "state": st.vector(),
            "steps": np.array([t["step"] for t in tr.tensors])}


def snap_cell(ft, m):
    torch.cuda.synchronize()
    return {"P": ft.P[m].cpu().numpy(), "m": ft.m[m].cpu().numpy(), "v": ft.v[m].cpu().numpy(),
            "state": ft.states[m].vector(), "steps": ft.sched.steps[m].copy()}


def same(a, b, what=""):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), f"{what}: {k} differs"


def same_result(a, b, what=""):
    """Two backprop(score=True) results, bit for bit."""
    (la, sa), (lb, sb) = a, b
    assert np.array(la).tobytes() == np.array(lb).tobytes(), f"{what}: losses differ"
    assert (sa is None) == (sb is None) and (sa is None or np.array(sa).tobytes() == np.array(sb).tobytes()), \
        f"{what}: scores {sa} != {sb}"


def pattern(t, k):
    """A sentinel pattern of t's shape and dtype that no computation produces by chance."""
    return (torch.arange(t.numel(), device=t.device, dtype=torch.float64) * 0.37 + k).to(t.dtype).view(t.shape)


# ---- 1. bytewise equal to lone runs ----

@pytest.mark.parametrize("H", [8, 16])
def test_fleet_equals_lone_runs(H):
    M, n = 5, 3
    ws = [cell_weights(H, 10 + m) for m in range(M)]
    ft = TR.FleetTuner(H, ws)
    lones = [lone(H, ws[m]) for m in range(M)]
    lone1b = lone(H, ws[1])                      # cell 1 once more, for its losses (below)
    # cell 4 starts from a lone 2-step run: non-zero step counts and moments
    pw, pa, pc = data(H, 1, 2, seed=900 + H)
    TR.backprop(*lones[4], pw[0], pa[0], pc[0], score=False)
    ft.load_cell(4, *lones[4])
    same(snap_cell(ft, 4), snap_lone(*lones[4]), "load_cell")
    assert ft.sched.steps[4].max() == 2
    # cell 3 is inactive: sentinels in everything of its slot
    active = [True, True, True, False, True]
    for k, t in enumerate((ft.P, ft.G, ft.m, ft.v, ft.logits, ft.protos)):
        t[3].copy_(pattern(t[3], k))
    sp = TR.TuneState(np.full((K, 2), 0.4321), 0.123)
    sp.num_zero, sp.num_ones = 5, 9
    ft.states[3] = sp
    g = ft.graph(n, True)
    g.dout.fill_(SENT)
    before3 = {k: t[3].clone() for k, t in (("P", ft.P), ("G", ft.G), ("m", ft.m), ("v", ft.v),
                                             ("logits", ft.logits), ("protos", ft.protos))}
    steps3 = ft.sched.steps[3].copy()
    for call in range(2):                        # the second call: counts, state and factor carried
        wins, anom, cls = data(H, M, n, seed=50 * H + call, no_positive=(1,))
        res = ft.tune(wins, anom, cls, active=active)
        out = g.hout.numpy().copy()
        for m in (0, 2, 4):
            want = TR.backprop(*lones[m], wins[m], anom[m], cls[m], score=True)
            same_result(res[m], want, f"call {call} cell {m}")
            same(snap_cell(ft, m), snap_lone(*lones[m]), f"call {call} cell {m}")
        # cell 1 has no positive label: the lone scored call raises after its graph ran (class_total = 0,
        # train.py:109); the fleet reports no scores for that cell.  Its losses come from an unscored lone run.
        with pytest.raises(ZeroDivisionError):
            TR.backprop(*lones[1], wins[1], anom[1], cls[1], score=True)
        same(snap_cell(ft, 1), snap_lone(*lones[1]), f"call {call} cell 1")
        losses1 = TR.backprop(*lone1b, wins[1], anom[1], cls[1], score=False)
        same_result(res[1], (losses1, None), f"call {call} cell 1")
        same(snap_lone(*lone1b), snap_lone(*lones[1]), "scored and unscored lone runs")
        # the inactive cell: untouched
        assert res[3] is None
        for k, t in (("P", ft.P), ("G", ft.G), ("m", ft.m), ("v", ft.v), ("logits", ft.logits), ("protos", ft.protos)):
            assert torch.equal(t[3], before3[k]), k
        assert (ft.sched.steps[3] == steps3).all()
        assert ft.states[3].vector().tobytes() == sp.vector().tobytes()
        S = 2 * K + 3
        assert (out[:g.o_state].reshape(M, n, 2)[3] == SENT).all()                       # losses
        assert out[g.o_state:g.o_lg].reshape(M, S)[3].tobytes() == sp.vector().tobytes()  # the state as uploaded
        assert (out[g.o_lg:g.o_pr].reshape(M, n, H, 2)[3] == SENT).all()
        assert (out[g.o_pr:].reshape(M, n, H, 2)[3] == SENT).all()
    # the prototype decoder of cell 1 never stepped, everything else of it did 2n times
    cond = [i for i, t in enumerate(ft.tensors) if t["name"] in TR.COND_TENSORS]
    assert (ft.sched.steps[1, cond] == 0).all() and ft.sched.steps[1, ft.sched.base_col] == 2 * n


# ---- 2. dropout ----

@pytest.mark.parametrize("H", [8, 16])
def test_dropout_fleet_equals_lone_dropout_runs(H):
    M, n, seeds = 3, 2, [1, 2 ** 32 + 5, 7]
    ws = [cell_weights(H, 20 + m) for m in range(M)]
    ft = TR.FleetTuner(H, ws, dropout=0.1, dropout_seeds=seeds)
    lones = [lone(H, ws[m], dropout=0.1, dropout_seed=seeds[m]) for m in range(M)]
    plain = TR.FleetTuner(H, ws)
    first = None
    for call in range(2):
        wins, anom, cls = data(H, M, n, seed=70 * H + call)
        res = ft.tune(wins, anom, cls)
        if call == 0:
            first = plain.tune(wins, anom, cls)
        for m in range(M):
            want = TR.backprop(*lones[m], wins[m], anom[m], cls[m], score=True)
            same_result(res[m], want, f"call {call} cell {m}")
            same(snap_cell(ft, m), snap_lone(*lones[m]), f"call {call} cell {m}")
    assert not torch.equal(ft.P, plain.P)               # the masks did something


@pytest.mark.parametrize("H", [8, 16])
def test_p0_through_the_many_entries_is_the_fleet_without_dropout(H):
    """dropout = 0 with seeds set (p = 0 reaches pgp_tune_step1_many beside an rng table) = no dropout at all."""
    M, n = 2, 2
    ws = [cell_weights(H, 30 + m) for m in range(M)]
    a = TR.FleetTuner(H, ws, dropout=0.0, dropout_seeds=[3, 2 ** 40])
    b = TR.FleetTuner(H, ws)
    wins, anom, cls = data(H, M, n, seed=H)
    ra, rb = a.tune(wins, anom, cls), b.tune(wins, anom, cls)
    for m in range(M):
        same_result(ra[m], rb[m])
        same(snap_cell(a, m), snap_cell(b, m))
    tr, st = lone(H, ws[1])
    same_result(ra[1], TR.backprop(tr, st, wins[1], anom[1], cls[1], score=True))


# ---- 3. more cells than CUs; position and size invariance ----

def test_more_cells_than_cus():
    H, M, n = 8, 300, 2
    base = [cell_weights(H, 40 + j) for j in range(3)]
    w3, a3, c3 = data(H, 3, n, seed=4)
    idx = np.arange(M) % 3
    ft = TR.FleetTuner(H, [base[j] for j in idx])
    res = ft.tune(w3[idx], a3[idx], c3[idx])
    torch.cuda.synchronize()
    for t in (ft.P, ft.G, ft.m, ft.v, ft.logits, ft.protos, ft.state_dev):
        a = t.cpu().numpy()
        assert a.tobytes() == a[idx].tobytes()           # every slot equals slot j mod 3
    for j in range(3, M):
        same_result(res[j], res[j % 3], f"cell {j}")
    small = TR.FleetTuner(H, base)
    rs = small.tune(w3, a3, c3)
    for j in range(3):
        same_result(rs[j], res[j], f"M=3 cell {j}")
        same(snap_cell(small, j), snap_cell(ft, j), f"M=3 cell {j}")
        one = TR.FleetTuner(H, [base[j]])
        r1 = one.tune(w3[j:j + 1], a3[j:j + 1], c3[j:j + 1])
        same_result(r1[0], res[j], f"M=1 cell {j}")
        same(snap_cell(one, 0), snap_cell(ft, j), f"M=1 cell {j}")


# ---- 4. the graph equals the eager sequence of the C entries ----

@pytest.mark.parametrize("H, p", [(8, 0.0), (16, 0.1)])
def test_graph_equals_eager_entries(H, p):
    M, n = 3, 2
    ws = [cell_weights(H, 50 + m) for m in range(M)]
    seeds = [11, 12, 2 ** 33 + 1]
    active = [True, False, True]
    wins, anom, cls = data(H, M, n, seed=9 * H)
    a = TR.FleetTuner(H, ws, dropout=p, dropout_seeds=seeds)
    a.tune(wins, anom, cls, active=active)
    ga = a.graph(n, True)
    b = TR.FleetTuner(H, ws, dropout=p, dropout_seeds=seeds)
    g = b.graph(n, True, capture=False)
    b.stage(g, wins, anom, cls, active)
    g.din.copy_(g.hin)
    L, T, vp = b._L, len(b.sel), ctypes.c_void_p
    ptr = lambda t: vp(t.data_ptr())
    for i in range(n):
        _native.check(L.pgp_tune_step1_many(
            H, K, M, n, i, ptr(g.active), ptr(g.W), ptr(g.Y), ptr(g.C), ptr(b.P), ptr(b.G), ptr(g.state),
            TR.PROTO_UPDATE_MIN, TR.PROTO_FACTOR_DECAY, ptr(b.logits), ptr(b.protos), ptr(g.dout), p, ptr(g.rng),
            b._stream()), "pgp_tune_step1_many")
        _native.check(L.pgp_adamw_table_many_d(    # the entry the graph holds (the betas as doubles)
            M, b.slot_len, ptr(g.active), ptr(b.P), ptr(b.G), ptr(b.m), ptr(b.v), b.lrs["transformer"], b.wd, b.b1,
            b.b2, b.eps, b._desc, T, ptr(g.sched[:, i]), n * T * 3, b._stream()), "pgp_adamw_table_many_d")
    g.dout[g.o_state:g.o_lg].copy_(g.state.view(-1))
    _native.check(L.pgp_tune_forward_cells(H, M, n, ptr(g.active), ptr(g.W), ptr(b.P), ptr(g.dout[g.o_lg:]),
                                           ptr(g.dout[g.o_pr:]), b._stream()), "pgp_tune_forward_cells")
    torch.cuda.synchronize()
    for k in ("P", "G", "m", "v", "logits", "protos"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert ga.dout.cpu().numpy().tobytes() == g.dout.cpu().numpy().tobytes()
    assert not torch.equal(a.P[0], torch.from_numpy(W.pack_blob(ws[0], H)[:b.slot_len].astype(np.float32)).to(a.device))
    assert torch.equal(a.P[1], torch.from_numpy(W.pack_blob(ws[1], H)[:b.slot_len].astype(np.float32)).to(a.device))


# ---- 5. detect ----

def _forward1_of(ft, m, win, sched):
    tr, st = ft.trainer(m)
    H, dev = ft.H, ft.device
    f32, i32 = torch.float32, torch.int32
    out = {"logits": torch.zeros((1, H, 2), dtype=f32, device=dev), "protos": torch.zeros((1, H, 2), dtype=f32, device=dev),
           "cls": torch.zeros((1, H), dtype=i32, device=dev), "any": torch.zeros(1, dtype=i32, device=dev),
           "probs": torch.zeros((1, 2), dtype=f32, device=dev), "keep": torch.zeros(1, dtype=i32, device=dev),
           "final_target": torch.zeros((1, H), dtype=i32, device=dev),
           "gen_target": torch.zeros((1, H), dtype=i32, device=dev)}
    tr.forward1(torch.tensor(win, device=dev), torch.tensor(sched, device=dev),
                torch.tensor(st.protos, dtype=torch.float64, device=dev), out)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy()[0] for k, v in out.items()}


@pytest.mark.parametrize("H", [8, 16])
def test_detect_rows_are_the_cells_own_forward1(H):
    M, n = 3, 2
    ws = [cell_weights(H, 60 + m) for m in range(M)]
    ft = TR.FleetTuner(H, ws)
    r = np.random.default_rng(H)
    win = r.uniform(0, 1, (M, 3, 3 * H)).astype(np.float32)
    win[:, 2, ::3] += 2.0                                   # spikes, so that some hosts are detected
    sched = r.uniform(0, 1, (M, H, H)).astype(np.float32)
    keys = ("logits", "protos", "cls", "any", "probs", "keep", "final_target", "gen_target")

    def rows():
        out = ft.detect(win, sched)
        torch.cuda.synchronize()
        assert out["logits"].shape == (M, H, 2) and out["any"].shape == (M,) and out["latent"] is None
        return {k: out[k].cpu().numpy().copy() for k in keys}

    def check(o):
        for m in range(M):
            want = _forward1_of(ft, m, win[m], sched[m])
            for k in keys:
                assert o[k][m].tobytes() == want[k].tobytes(), (m, k)

    o0 = rows()
    check(o0)
    assert len({o0["logits"][m].tobytes() for m in range(M)}) == M       # each row from its own weights
    wins, anom, cls = data(H, M, n, seed=3 * H)
    ft.tune(wins, anom, cls, active=[True, False, True])
    o1 = rows()
    check(o1)
    for m, tuned in enumerate((True, False, True)):
        for k in ("logits", "protos", "probs"):
            assert (o1[k][m].tobytes() != o0[k][m].tobytes()) == tuned, (m, k)


# ---- 6. round trip through a lone Trainer ----

@pytest.mark.parametrize("H, p", [(8, 0.0), (16, 0.1)])
def test_trainer_round_trip(H, p):
    M, n = 2, 2
    ws = [cell_weights(H, 70 + m) for m in range(M)]
    seeds = [5, 2 ** 35 + 3]
    calls = [data(H, M, n, seed=11 * H + c) for c in range(4)]
    a = TR.FleetTuner(H, ws, dropout=p, dropout_seeds=seeds)
    b = TR.FleetTuner(H, ws, dropout=p, dropout_seeds=seeds)
    a.tune(*calls[0])
    b.tune(*calls[0])
    tr, st = a.trainer(0)
    same(snap_lone(tr, st), snap_cell(a, 0), "trainer(0)")
    assert tr.dropout == p and tr.dropout_seed == seeds[0]
    for c in (1, 2):
        w, y, k = calls[c]
        want = TR.backprop(tr, st, w[0], y[0], k[0], score=True)
        got = b.tune(w, y, k, active=[True, False])
        same_result(got[0], want, f"call {c}")
    a.load_cell(0, tr, st)
    ra, rb = a.tune(*calls[3]), b.tune(*calls[3])
    for m in range(M):
        same_result(ra[m], rb[m], f"cell {m}")
        same(snap_cell(a, m), snap_cell(b, m), f"cell {m}")


# ---- 7. arguments: refused calls touch nothing ----

@pytest.mark.parametrize("H", [8, 16])
def test_refused_calls_leave_the_outputs_untouched(H):
    M, n, dev = 2, 2, "cuda"
    L, vp = _native.lib(), ctypes.c_void_p
    N, T = int(L.pgp_master_len(H)), 3
    f32, f64, i32 = torch.float32, torch.float64, torch.int32
    full = lambda shp, dt: torch.full(shp, SENT if dt != i32 else -7, dtype=dt, device=dev)
    P, G, m_, v_ = (full((M, N), f32) for _ in range(4))
    state, loss = full((M, 2 * K + 3), f64), full((M, n, 2), f64)
    logits, protos = full((M, H, 2), f32), full((M, H, 2), f32)
    lg64, pr64 = full((M, n, H, 2), f64), full((M, n, H, 2), f64)
    o_cls, o_any, o_probs, o_keep, o_ft, o_gt = (full((M, H), i32), full((M,), i32), full((M, 2), f32),
                                                 full((M,), i32), full((M, H), i32), full((M, H), i32))
    outs = [P, G, m_, v_, state, loss, logits, protos, lg64, pr64, o_cls, o_any, o_probs, o_keep, o_ft, o_gt]
    win = torch.zeros((M, n, 3, 3 * H), dtype=f32, device=dev)
    y = torch.zeros((M, n, H), dtype=i32, device=dev)
    sched = torch.zeros((M, H, H), dtype=f32, device=dev)
    tab = torch.ones((M, n, T, 3), dtype=f32, device=dev)
    rng = torch.zeros((M, 2), dtype=torch.int64, device=dev)
    desc = (TR._AdamTensor * T)(*[TR._AdamTensor(100 * i, 50, 1, 0.0, 0.0) for i in range(T)])
    p_ = lambda t: None if t is None else vp(t.data_ptr())

    def step(H_=H, M_=M, n_=n, i=0, p=0.0, K_=K, rng_=rng, null=None):
        a = {"win": win, "y": y, "cls": y, "P": P, "G": G, "state": state, "logits": logits, "protos": protos,
             "loss": loss}
        if null:
            a[null] = None
        return L.pgp_tune_step1_many(H_, K_, M_, n_, i, None, p_(a["win"]), p_(a["y"]), p_(a["cls"]), p_(a["P"]),
                                     p_(a["G"]), p_(a["state"]), 0.02, 0.995, p_(a["logits"]), p_(a["protos"]),
                                     p_(a["loss"]), p, p_(rng_), None)

    def adamw(M_=M, slot=N, nt=T, stride=n * T * 3, null=None, d=desc):
        a = {"P": P, "G": G, "m": m_, "v": v_, "tab": tab}
        if null:
            a[null] = None
        return L.pgp_adamw_table_many(M_, slot, None, p_(a["P"]), p_(a["G"]), p_(a["m"]), p_(a["v"]), 1e-4, 1e-5, 0.9,
                                      0.999, 1e-8, d, nt, p_(a["tab"]), stride, None)

    def fwd(H_=H, M_=M, n_=n, null=None):
        a = {"win": win, "P": P, "lg": lg64, "pr": pr64}
        if null:
            a[null] = None
        return L.pgp_tune_forward_cells(H_, M_, n_, None, p_(a["win"]), p_(a["P"]), p_(a["lg"]), p_(a["pr"]), None)

    def infer(H_=H, M_=M, K_=K, null=None):
        a = [win, sched, P, state, logits, protos, o_cls, o_any, o_probs, o_keep, o_ft, o_gt]
        if null is not None:
            a[null] = None
        return L.pgp_forward1_many(H_, K_, M_, None, *[p_(t) for t in a], None)

    UNS, ARG, OK = -2, -1, 0
    for other in (32, 50, 0):
        assert step(H_=other) == UNS and fwd(H_=other) == UNS and infer(H_=other) == UNS
    cases = [step(M_=-1), step(n_=-1), step(i=-1), step(i=n), step(p=1.0), step(p=-0.1), step(p=float("nan")),
             step(K_=2), step(p=0.1, rng_=None)]
    cases += [step(null=k) for k in ("win", "y", "cls", "P", "G", "state", "logits", "protos", "loss")]
    cases += [adamw(M_=-1), adamw(slot=-1), adamw(nt=-1), adamw(nt=49), adamw(stride=-1), adamw(M_=65536),
              adamw(slot=120)]                                        # a tensor outside the slot
    cases += [adamw(null=k) for k in ("P", "G", "m", "v", "tab")]
    cases += [fwd(M_=-1), fwd(n_=-1), fwd(M_=65536)] + [fwd(null=k) for k in ("win", "P", "lg", "pr")]
    cases += [infer(M_=-1), infer(K_=0), infer(K_=65)] + [infer(null=k) for k in range(12)]
    assert cases == [ARG] * len(cases)
    assert step(M_=0) == OK and adamw(M_=0) == OK and fwd(M_=0) == OK and fwd(n_=0) == OK and infer(M_=0) == OK
    assert step(M_=0, null="P") == OK and infer(M_=0, null=0) == OK   # nothing is read with no cell
    torch.cuda.synchronize()
    for t in outs:
        assert bool((t == (SENT if t.dtype != i32 else -7)).all())
