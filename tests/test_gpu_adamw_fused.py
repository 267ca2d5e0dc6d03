"""Every training step that ends in AdamW, replayed in fp64 from the gradient it
leaves in ``G`` (tests/adamw_replay.py): P / m / v before the step, G / P / m / v
after it, torch's single-tensor AdamW on those G bits, the rounding bound of
``adamw_update``.  The same G enters both sides, so there is no sign noise, no
key-bias exclusion and no lr-sized waiver: "is the gradient right" is the
autograd tests' question (test_gpu_train.py, test_gpu_train_regimes.py), "is
the update right" is this file's.  tests/test_gpu_adamw.py holds the update
alone on prescribed gradients.

Forms, each at the smallest shapes it compiles for:
  * pgp_gan_forward1 + pgp_gan_step1 (train_gan fused, 8 / 16 hosts) and
    pgp_gan_step1_many (FleetTuner.train_gan, 3 cells, one inactive), with the
    gradients' outer-product structure bit for bit and their factor vectors
    against fp64 autograd;
  * train_gan_batched (pgp_gantrain.hip's backward + pgp_adamw_d);
  * backprop(fused=True), one window per call (tune1_kernel + pgp_adamw_table_d
    in the captured graph), with and without dropout, with a window without a
    positive label;
  * dp_tune_step on one rank;
  * FPETrainer.backprop, one window, from a new model with zero biases;
  * pgp_online_step at world size 1 (see test_online_step_replays for what it
    shows about the update fused into the batched GAN weight-gradient kernel,
    ``AdamFuse``, whose only caller it is).

Out of scope: GOBI's coupled-L2 Adam exposes no G
(tests/test_gpu_gobitrain.py::test_gradient_alone pins its gradient)."""
import numpy as np
import pytest
import torch

from oracle import pregan_train_oracle as TO
from preganplus_amd import train as TR
from preganplus_amd import weights as W
from tests import adamw_replay as AR

pytestmark = pytest.mark.gpu

COND = ("prototype_decoder.0.weight", "prototype_decoder.0.bias")


def snap(o):
    """P / G / m / v of a Trainer, FPETrainer or FleetTuner, flat, on the host."""
    torch.cuda.synchronize()
    return {k: getattr(o, k).cpu().numpy().reshape(-1).copy() for k in "PGmv"}


def steps_of(o):
    return np.array([t["step"] for t in o.tensors], dtype=np.float64)


def replay_step(what, o, before, steps0, steps1, lr_of, slot=0, after=None):
    """The step between two snapshots of o's buffers (slot: a fleet cell's
    offset), tensor i active iff its host step count advanced (by exactly 1).
    Returns (worst error/tolerance of P, m, v; the set of names that stepped)."""
    after = snap(o) if after is None else after
    d = np.asarray(steps1) - np.asarray(steps0)
    assert set(np.unique(d)) <= {0.0, 1.0}, (what, d)
    tensors, stepped = [], set()
    for t, di, s1 in zip(o.tensors, d, steps1):
        act = int(di) if t.get("trainable", True) else 0
        assert act == int(di), (what, t["name"], "a frozen tensor's count advanced")
        tensors.append((slot + t["offset"], t["n"], act, max(s1, 1.0), lr_of(t)))
        if act:
            stepped.add(t["name"])
            sl = slice(slot + t["offset"], slot + t["offset"] + t["n"])
            if after["G"][sl].any():     # a counted step on a non-zero gradient moves the first moment
                assert not np.array_equal(AR.bits(before["m"][sl]), AR.bits(after["m"][sl])), (what, t["name"])
    lo, hi = slot, slot + o.tensors[-1]["offset"] + o.tensors[-1]["n"]
    cut = lambda s: {k: a[lo:hi] for k, a in s.items()}
    local = [(off - slot, *rest) for off, *rest in tensors]
    b = cut(before)
    b.pop("G")
    worst = AR.assert_step(what, b, cut(after), local, lr=float("nan"), wd=o.wd, b1=o.b1, b2=o.b2, eps=o.eps)
    print(f"AdamW replay {what}: worst error/tolerance P {worst[0]:.3f} m {worst[1]:.3f} v {worst[2]:.3f}")
    return worst, stepped


def section_bits_equal(o, a, b, section, slot=0):
    for t in o.tensors:
        if t["section"] == section:
            sl = slice(slot + t["offset"], slot + t["offset"] + t["n"])
            for k in "PGmv":
                assert np.array_equal(AR.bits(a[k][sl]), AR.bits(b[k][sl])), (section, t["name"], k)


def names(o, *sections):
    return {t["name"] for t in o.tensors if t["section"] in sections and t.get("trainable", True)}


# ---------------------------------------------------------------------------
# the fused batch-1 GAN step
# ---------------------------------------------------------------------------
def gs_offsets(H):
    """TGeo<H>::GS_* of the GAN workspace row (csrc/pgp_train.hpp)."""
    gin, din = 2 * H + H * H, 2 * H * H
    x, z = 0, gin
    h = z + din
    t = h + 64
    dd = t + H * H
    return {"X": (x, gin), "Z": (z, din), "Hg": (h, 64), "T": (t, H * H), "DD": (dd, 64)}


def gan_tensor(o, section, name, G, slot=0):
    t = next(t for t in o.tensors if t["section"] == section and t["name"] == name)
    return G[slot + t["offset"]:slot + t["offset"] + t["n"]]


def ratio(got, want, rel=1e-3, abs_scale=1e-4):
    """error / tolerance of the suite's gradient comparison (test_gpu_train.close)."""
    want = np.asarray(want, dtype=np.float64).reshape(-1)
    tol = rel * np.abs(want) + abs_scale * (np.abs(want).max() + 1e-30)
    return float((np.abs(np.asarray(got, dtype=np.float64).reshape(-1) - want) / tol).max())


def check_gan_gradients(what, o, H, row, G, slot, w_pre, w_post, emb, sched, target):
    """The structure of the GAN step's gradients.  Every weight gradient is the
    outer product of its bias gradient with the layer's input from the
    forward's workspace row, each entry ONE fp32 product (bit for bit: a
    swapped index or a wrong leading dimension cannot pass); the four bias
    gradients against fp64 autograd: the Disc's BCE toward ``target`` at the
    pre-step weights on the kernel's own ns, the Gen's BCE toward [0, 1]
    through the Disc at its POST-step weights (the Disc the kernel
    differentiated through).  Returns the worst autograd error/tolerance."""
    gs = gs_offsets(H)
    part = lambda k: row[gs[k][0]:gs[k][0] + gs[k][1]]
    g = lambda sec, name: gan_tensor(o, sec, name, G, slot)
    for sec, wname, bname, vec in (("disc", "probs.0.weight", "probs.0.bias", "Z"),
                                   ("disc", "probs.2.weight", "probs.2.bias", "DD"),
                                   ("gen", "delta.2.weight", "delta.2.bias", "Hg"),
                                   ("gen", "delta.0.weight", "delta.0.bias", "X")):
        b, x = g(sec, bname), part(vec)
        want = (b[:, None] * x[None, :]).astype(np.float32)
        got = g(sec, wname).reshape(want.shape)
        assert np.array_equal(AR.bits(got), AR.bits(want)), \
            (what, wname, "not the outer product of", bname, "and", vec, int((AR.bits(got) != AR.bits(want)).sum()))
        assert b.any() and x.any(), (what, bname, vec)
    HH = H * H
    s_t = torch.tensor(np.asarray(sched, dtype=np.float64).reshape(1, H, H))
    ns_k = torch.tensor(part("Z")[HH:].astype(np.float64).reshape(1, H, H))
    e_t = torch.tensor(np.asarray(emb, dtype=np.float64).reshape(1, -1))
    bce = torch.nn.functional.binary_cross_entropy
    dw = TO.leaf_params(w_pre["disc"])
    bce(TO.disc_t(dw, s_t, ns_k)[0], torch.tensor(np.asarray(target, dtype=np.float64))).backward()
    gw, dw2 = TO.leaf_params(w_pre["gen"]), TO.leaf_params(w_post["disc"])
    bce(TO.disc_t(dw2, s_t, TO.gen_t(gw, e_t, s_t))[0], torch.tensor([0.0, 1.0], dtype=torch.float64)).backward()
    worst = 0.0
    for sec, bname, ref in (("disc", "probs.0.bias", dw), ("disc", "probs.2.bias", dw),
                            ("gen", "delta.2.bias", gw), ("gen", "delta.0.bias", gw)):
        r = ratio(g(sec, bname), ref[bname].grad.numpy())
        assert r < 1, (what, bname, r)
        worst = max(worst, r)
    return worst


def weights_of(P, o, H):
    """A master slot as reference-named fp64 arrays per section (Trainer.weights_numpy for any slot)."""
    shapes = {(sec, name): shp for sec, name, shp in W.blob_layout(H)[:-1]}
    out = {"transformer": {}, "gen": {}, "disc": {}}
    for t in o.tensors:
        out[t["section"]][t["name"]] = P[t["offset"]:t["offset"] + t["n"]].astype(np.float64).reshape(
            shapes[(t["section"], t["name"])])
    return out


@pytest.mark.parametrize("H", [8, 16])
def test_fused_gan_step_replays(H):
    tr = TR.Trainer(H, W.synth_weights(H, seed=4))
    rng = np.random.default_rng(8 + H)
    labels, worst, worst_grad = set(), np.zeros(3), 0.0
    for call in range(4):
        emb = rng.random(2 * H).astype(np.float32)
        sched = np.eye(H)[rng.integers(0, H, H)]
        scores = iter((1.0, 2.0) if call % 2 else (2.0, 1.0))
        rows = []

        def simulate(s):     # between pgp_gan_forward1 and pgp_gan_step1: the step's last forward overwrites the row
            if not rows:
                rows.append(tr.gscr.cpu().numpy().copy())
            return next(scores)

        before, steps0 = snap(tr), steps_of(tr)
        res = TR.train_gan(tr, emb, sched, simulate, fused=True)
        after = snap(tr)
        what = f"gan_step1 H={H} call {call}"
        w, stepped = replay_step(what, tr, before, steps0, steps_of(tr), lambda t: tr.lrs[t["section"]], after=after)
        assert stepped == names(tr, "gen", "disc")
        section_bits_equal(tr, before, after, "transformer")
        target = TR.bce_target(res[1], res[2])
        labels.add(tuple(target))
        n = tr.P.numel()
        worst_grad = max(worst_grad, check_gan_gradients(
            what, tr, H, rows[0], after["G"], 0, weights_of(before["P"][:n], tr, H), weights_of(after["P"][:n], tr, H),
            emb, sched, target))
        worst = np.maximum(worst, w)
    assert labels == {(0.0, 1.0), (1.0, 0.0)}
    assert {t["step"] for t in tr.tensors if t["section"] != "transformer"} == {4.0}
    print(f"gan_step1 H={H}: bias gradients vs fp64 autograd, worst error/tolerance {worst_grad:.3f}")


@pytest.mark.parametrize("H", [8, 16])
def test_fleet_gan_step_replays(H):
    M, active = 3, [True, False, True]
    ws = []
    for m in range(M):
        w = W.synth_weights(H, seed=20 + m)
        w["prototypes"] = np.random.default_rng(m).uniform(0.1, 0.9, (16, 2))
        ws.append(w)
    ft = TR.FleetTuner(H, ws)
    n = ft.slot_len
    rng = np.random.default_rng(80 + H)
    script = {0: [(1.0, 2.0), (3.0, 1.0), (2.0, 2.0), (4.0, 1.0)], 2: [(3.0, 1.0), (0.5, 2.0), (5.0, 1.0), (1.0, 1.5)]}
    lr_of = lambda t: ft.lrs[t["section"]]
    labels, worst, worst_grad = set(), np.zeros(3), 0.0
    for call in range(4):
        emb = (rng.uniform(0.1, 0.9, (M, H, 2)) * (rng.uniform(size=(M, H, 1)) < 0.5)).astype(np.float32)
        scheds = rng.uniform(0, 1, (M, H, H))
        rows = []

        def sim_of(c):
            it = iter(script[c][call])

            def f(s):
                if not rows:
                    rows.append(ft.gan_graph(False).gscr.cpu().numpy().copy())
                return next(it)
            return f

        before, steps0 = snap(ft), ft.sched.steps.copy()
        res = ft.train_gan(emb, scheds, simulate=[sim_of(c) if active[c] else None for c in range(M)], active=active)
        after = snap(ft)
        row = rows[0].reshape(M, -1)
        for c in range(M):
            what = f"gan_step1_many H={H} call {call} cell {c}"
            w, stepped = replay_step(what, ft, before, steps0[c], ft.sched.steps[c], lr_of, slot=c * n, after=after)
            section_bits_equal(ft, before, after, "transformer", slot=c * n)
            if not active[c]:
                assert not stepped and res[c] is None
                for sec in ("gen", "disc"):
                    section_bits_equal(ft, before, after, sec, slot=c * n)
                continue
            assert stepped == names(ft, "gen", "disc")
            target = TR.bce_target(res[c][1], res[c][2])
            labels.add(tuple(target))
            sl = slice(c * n, (c + 1) * n)
            worst_grad = max(worst_grad, check_gan_gradients(
                what, ft, H, row[c], after["G"], c * n, weights_of(before["P"][sl], ft, H),
                weights_of(after["P"][sl], ft, H), emb[c], scheds[c].astype(np.float32), target))
            worst = np.maximum(worst, w)
    assert labels == {(0.0, 1.0), (1.0, 0.0)}
    print(f"gan_step1_many H={H}: worst AdamW error/tolerance {worst}, bias gradients vs autograd {worst_grad:.3f}")


# ---------------------------------------------------------------------------
# the batched GAN step
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("H,B", [(16, 37), (50, 9)])
def test_batched_gan_step_replays(H, B):
    from preganplus_amd import simulate as SIM
    tr = TR.Trainer(H, W.synth_weights(H, seed=12), max_batch=B)
    sim = SIM.Simulation(H, device=tr.device)
    rng = np.random.default_rng(H + B)
    for call in range(2):
        emb = np.where(rng.uniform(size=(B, H, 1)) < 0.4, rng.uniform(size=(B, H, 2)), 0.0).astype(np.float32)
        s = np.zeros((B, H, H), np.float32)
        s[np.arange(B)[:, None], np.arange(H)[None, :], rng.integers(0, H, size=(B, H))] = 1.0
        before, steps0 = snap(tr), steps_of(tr)
        TR.train_gan_batched(tr, sim, SIM.synth_envs(B, H, seed=3 + call), emb, s)
        after = snap(tr)
        _, stepped = replay_step(f"train_gan_batched H={H} B={B} call {call}", tr, before, steps0, steps_of(tr),
                                 lambda t: tr.lrs[t["section"]], after=after)
        assert stepped == names(tr, "gen", "disc")
        section_bits_equal(tr, before, after, "transformer")


# ---------------------------------------------------------------------------
# the tuning steps
# ---------------------------------------------------------------------------
def tune_inputs(H, n, seed, positive=True):
    rng = np.random.default_rng(seed)
    wins = rng.uniform(0, 0.8, size=(n, 3, 3 * H)).astype(np.float32)
    anom = (rng.uniform(size=(n, H)) < 0.3).astype(np.int32)
    anom[:, 1] = 1
    if not positive:
        anom[:] = 0
    return wins, anom, rng.integers(0, 3, size=(n, H)).astype(np.int32)


@pytest.mark.parametrize("dropout", [0.0, 0.1])
@pytest.mark.parametrize("H", [8, 16])
def test_fused_tune_step_replays(H, dropout):
    """Three calls of one window; the second has no positive label: torch skips a parameter whose grad is None,
    so the prototype decoder's P / m / v and step counts keep their bits."""
    w = W.synth_weights(H, seed=6)
    tr = TR.Trainer(H, w, max_batch=1, dropout=dropout, dropout_seed=77)
    st = TR.TuneState(w["prototypes"])
    for call in range(3):
        wins, anom, cls = tune_inputs(H, 1, 10 * H + call, positive=call != 1)
        before, steps0 = snap(tr), steps_of(tr)
        TR.backprop(tr, st, wins, anom, cls, fused=True)
        after = snap(tr)
        _, stepped = replay_step(f"backprop fused H={H} dropout={dropout} call {call}", tr, before, steps0,
                                 steps_of(tr), lambda t: tr.lrs[t["section"]], after=after)
        want = names(tr, "transformer") - (set(COND) if call == 1 else set())
        assert stepped == want, stepped ^ want
        for sec in ("gen", "disc"):
            section_bits_equal(tr, before, after, sec)
    by = {t["name"]: t["step"] for t in tr.tensors}
    assert by[COND[0]] == by[COND[1]] == 2.0 and by["time_encoder.weight"] == 3.0


def test_dp_tune_step_replays():
    H, B = 16, 37
    w = W.synth_weights(H, seed=6)
    tr = TR.Trainer(H, w, max_batch=B)
    st = TR.TuneState(w["prototypes"])
    for call in range(2):
        wins, anom, cls = tune_inputs(H, B, 5 + call)
        before, steps0 = snap(tr), steps_of(tr)
        TR.dp_tune_step(tr, st, wins, anom, cls)
        after = snap(tr)
        _, stepped = replay_step(f"dp_tune_step H={H} B={B} call {call}", tr, before, steps0, steps_of(tr),
                                 lambda t: tr.lrs[t["section"]], after=after)
        assert stepped == names(tr, "transformer")
        for sec in ("gen", "disc"):
            section_bits_equal(tr, before, after, sec)


@pytest.mark.parametrize("H", [16, 50])
def test_fpe_step_replays(H):
    """A new FPE (torch's MultiheadAttention starts with zero biases): the moment weights' error is largest
    against |p| here.  Two calls of one window, the second without a positive label."""
    from preganplus_amd import fpetrain as FT
    fpe = dict(W.synth_fpe_weights(H, seed=3)["fpe"])
    for k in ("mha.in_proj_bias", "mha.out_proj.bias"):
        fpe[k] = np.zeros_like(fpe[k])
    ft = FT.FPETrainer(fpe, H=H)
    st = TR.TuneState(np.random.default_rng(1).uniform(0.1, 0.9, (3, 2)), 0.2)
    rng = np.random.default_rng(H)
    for call in range(2):
        wins, anom, cls = tune_inputs(H, 1, 30 * H + call, positive=call == 0)
        h0 = rng.standard_normal((1, 3)).astype(np.float32)
        before, steps0 = snap(ft), steps_of(ft)
        ft.backprop(st, wins, h0, anom, cls)
        _, stepped = replay_step(f"FPETrainer.backprop H={H} call {call}", ft, before, steps0, steps_of(ft),
                                 lambda t: ft.lr)
        want = {t["name"] for t in ft.tensors} - (set(COND) if call == 1 else set())
        assert stepped == want, stepped ^ want


# ---------------------------------------------------------------------------
# the native online step: AdamW fused into the batched GAN weight-gradient kernel
# ---------------------------------------------------------------------------
def test_online_step_replays():
    """Whatever launches pgp_online_step chooses, every section's update is inside the bound.  Which launches:
    with no collective callback (one process: ``step._cb`` is NULL, asserted) the library takes its world-size-1
    branch, where each GAN section's AdamW runs inside its weight-gradient kernel (``AdamFuse``) if
    ``fuse_adam`` (csrc/pgp_online.hip) finds one set of per-step scalars for the whole section and no table
    rows: the GAN sections have no device table (the library gives one to the transformer only), and all their
    tensors carry the same step count (asserted before each step), hence the same lr / bc1 and sqrt(bc2).  If
    those conditions failed the library would run the same update through ``adamw_kernel`` instead, which this
    test cannot tell apart: it pins the result, not the launch."""
    from tests.test_gpu_c3step import _online
    main = torch.cuda.Stream()
    with torch.cuda.stream(main):
        tr, step = _online(16, 6, native=True)
        assert not step._cb                      # NULL callback: the world-size-1 branch
        for call in range(2):
            torch.cuda.synchronize()
            for sec in ("gen", "disc"):
                assert len({t["step"] for t in tr.tensors if t["section"] == sec and t["trainable"]}) == 1
            before, steps0 = snap(tr), steps_of(tr)
            step.run()
            torch.cuda.synchronize()
            step.sync()
            _, stepped = replay_step(f"pgp_online_step H=16 E=6 call {call}", tr, before, steps0, steps_of(tr),
                                     lambda t: tr.lrs[t["section"]])
            assert names(tr, "gen", "disc") <= stepped and "time_encoder.weight" in stepped
