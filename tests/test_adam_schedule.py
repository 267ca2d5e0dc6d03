"""The AdamW host schedule (preganplus_amd/adamw.py) and every path built on it
against a scalar loop written here the way torch's single-tensor AdamW does it
(torch/optim/adamw.py: Python floats, ``beta ** step``, ``math.sqrt``):
bit-equal fp32 tables and equal final step counts.  CPU; the C-ABI's host-side
size queries only."""
import math

import numpy as np
import pytest

from preganplus_amd import adamw
from preganplus_amd import weights as W

B1, B2 = 0.9, 0.999


def reference(steps0, on, lr):
    """on [n][T] -> (table [n,T,3] fp32, the counts after the n steps)."""
    steps = [float(s) for s in steps0]
    tab = np.zeros((len(on), len(steps), 3), dtype=np.float32)
    for i, row in enumerate(on):
        for k, active in enumerate(row):
            if active:
                steps[k] += 1
            s = max(steps[k], 1)
            tab[i, k] = (float(active), np.float32(lr / (1 - B1 ** s)), np.float32(math.sqrt(1 - B2 ** s)))
    return tab, steps


def same_bits(got, want, msg=""):
    assert got.dtype == np.float32 and got.shape == want.shape, (msg, got.dtype, got.shape, want.shape)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg=str(msg))


def pattern(names, positive, cond=adamw.COND_TENSORS):
    return [[bool(p) or name not in cond for name in names] for p in positive]


def positives(rng, call, n=10):
    pos = rng.random(n) < 0.6
    if call == 0:
        pos[:3] = False            # cond tensors at step 0 (bias correction at max(step, 1))
    return pos


def fpe_lr():
    from preganplus_amd import fpetrain
    return fpetrain.FPE_LR


@pytest.mark.parametrize("start", [0, 1, 100, 12345])
@pytest.mark.parametrize("lr", [1e-4, 5e-5, 3e-5, "fpe"])
def test_schedule_matches_the_scalar_loop(lr, start):
    lr = fpe_lr() if lr == "fpe" else lr
    names = ("time_encoder.weight",) + adamw.COND_TENSORS + ("time_encoder.bias",)
    pos = positives(np.random.default_rng(start), 0)
    on = pattern(names, pos)
    steps0 = [float(start)] * len(names)
    tab, end = adamw.schedule(steps0, adamw.stepping(names, pos), lr, B1, B2)
    want, want_end = reference(steps0, on, lr)
    same_bits(tab, want, (lr, start))
    assert end.dtype == np.float64 and end.tolist() == want_end
    assert steps0 == [float(start)] * len(names)            # pure: the caller's counts are untouched
    counts = np.array([[0.0, 1.0], [start, start + 1.0]])    # scalars itself, in its argument's shape
    size, bc2 = adamw.scalars(lr, B1, B2, counts)
    s = [max(c, 1) for c in counts.ravel().tolist()]
    same_bits(size, np.array([lr / (1 - B1 ** c) for c in s], dtype=np.float32).reshape(2, 2))
    same_bits(bc2, np.array([math.sqrt(1 - B2 ** c) for c in s], dtype=np.float32).reshape(2, 2))


def test_trainer_schedule_over_consecutive_calls():
    from preganplus_amd import train as TR
    tr = TR.Trainer(16, W.synth_weights(16, seed=1), None, device="cpu", max_batch=1)
    sel = tr.trainable("transformer")
    names = [t["name"] for t in sel]
    assert set(TR.COND_TENSORS) < set(names)
    rng = np.random.default_rng(0)
    for call in range(4):
        pos = positives(rng, call)
        want, want_end = reference([t["step"] for t in sel], pattern(names, pos), tr.lrs["transformer"])
        same_bits(tr.adam_schedule_np("transformer", pos, TR.COND_TENSORS), want, call)
        assert [t["step"] for t in sel] == want_end
    assert {t["step"] for t in tr.tensors if t["section"] != "transformer"} == {0.0}


@pytest.mark.parametrize("H", [8, 16])
def test_fleet_tables_match_the_scalar_loop(H):
    from preganplus_amd import train as TR
    M, rng = 4, np.random.default_rng(H)
    fs = TR.FleetSchedule(H, M)
    fs.steps[3] = rng.integers(0, 40, len(fs.tensors))       # a cell that starts from non-zero counts
    names = [fs.tensors[i]["name"] for i in fs.sel]
    for call in range(3):
        positive = np.stack([positives(rng, call) for _ in range(M)])
        active = np.array([True, call == 1, True, True])     # cell 1 sits two calls out
        before = fs.steps.copy()
        tab = fs.tables(positive, active)
        tabD, tabG = fs.gan_tables(active)
        for m in range(M):
            if not active[m]:
                assert not tab[m].any() and not tabD[m].any() and not tabG[m].any()
                assert (fs.steps[m] == before[m]).all()
                continue
            want, end = reference(before[m, fs.sel], pattern(names, positive[m]), fs.lr)
            same_bits(tab[m], want, (call, m))
            assert fs.steps[m, fs.sel].tolist() == end
            for got, sel, sec in ((tabD, fs.sel_disc, "disc"), (tabG, fs.sel_gen, "gen")):
                want, end = reference(before[m, sel], [[True] * len(sel)], fs.lrs[sec])
                same_bits(got[m], want[0], (call, m, sec))
                assert fs.steps[m, sel].tolist() == end


def test_fpe_table_matches_the_scalar_loop():
    from preganplus_amd import fpetrain as FT
    names = list(W.fpe_shapes(16))
    assert FT.COND is adamw.COND_TENSORS and set(FT.COND) < set(names)
    tensors = [{"name": name, "step": 0.0} for name in names]
    rng = np.random.default_rng(2)
    for call in range(4):
        pos = positives(rng, call)
        want, want_end = reference([t["step"] for t in tensors], pattern(names, pos), FT.FPE_LR)
        same_bits(FT.adam_table(tensors, pos, FT.FPE_LR, B1, B2), want, call)
        assert [t["step"] for t in tensors] == want_end
