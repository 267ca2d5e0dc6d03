"""The host side of the fleet's per-cell GAN step (preganplus_amd/train.py:
FleetSchedule.gan_tables, the staging layouts of FleetTuner.train_gan) and the
cell-indexed GAN entries of the C-ABI (include/preganplus.h:
pgp_gan_forward1_many, pgp_gan_step1_many).  CPU: loads the library, makes no
GPU call — every check here runs on the host before anything is enqueued."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

from preganplus_amd import _native
from preganplus_amd import train as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -2
NEW = ("pgp_gan_forward1_many", "pgp_gan_step1_many")
_lib = _native.lib


def _header():
    with open(os.path.join(ROOT, "include", "preganplus.h")) as f:
        return f.read()


def test_header_declares_and_library_exports():
    hdr, L = _header(), _lib()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert hasattr(L, name), name
        at = hdr.index("int " + name)
        assert "PreGANPlus.py" in hdr[hdr.rindex("/*", 0, at):at], name     # cites the reference lines it stands for
    assert "#define PGP_ABI_VERSION 1" in hdr and L.pgp_abi_version() == 1   # additions only


def test_binding_argument_counts_match_the_header():
    hdr, L = _header(), _lib()
    for name, count in zip(NEW, (10, 26)):
        m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\);", hdr, re.S)
        assert len(m.group(1).split(",")) == count, name
        assert len(getattr(L, name).argtypes) == count, name


# ---- the GAN AdamW tables and count advances against Trainer.adam_schedule_np, cell by cell ----

def _lone(H, steps0):
    """A stand-in with the fields Trainer.adam_schedule_np reads (a Trainer needs a device)."""
    tensors = [dict(t, step=float(s)) for t, s in zip(TR.master_tensors(H), steps0)]
    return types.SimpleNamespace(tensors=tensors, lrs=TR.default_lrs(H), b1=0.9, b2=0.999)


@pytest.mark.parametrize("H", [8, 16])
def test_gan_tables_equal_the_lone_schedule(H):
    M, rng = 5, np.random.RandomState(H)
    fs = TR.FleetSchedule(H, M)
    nt = len(fs.tensors)
    fs.steps[4] = rng.randint(0, 40, nt)            # a cell that starts from non-zero counts
    lone = [_lone(H, fs.steps[m]) for m in range(M)]
    tr_cols = [i for i, t in enumerate(fs.tensors) if t["section"] == "transformer"]
    tr0 = fs.steps[:, tr_cols].copy()
    nD = sum(t["section"] == "disc" and t["trainable"] for t in fs.tensors)
    nG = sum(t["section"] == "gen" and t["trainable"] for t in fs.tensors)
    assert nD == 4 and nG == 4                       # Linear weight + bias, twice each (models.py:118-151)
    for call in range(3):
        active = np.array([True, True, call != 0, call == 1, True])   # cell 3 runs in one call, cell 2 skips one
        before = fs.steps.copy()
        tabD, tabG = fs.gan_tables(active)
        assert tabD.shape == (M, nD, 3) and tabG.shape == (M, nG, 3)
        assert tabD.dtype == np.float32 and tabG.dtype == np.float32
        for m in range(M):
            if not active[m]:
                assert not tabD[m].any() and not tabG[m].any() and (fs.steps[m] == before[m]).all()
                continue
            wantD = TR.Trainer.adam_schedule_np(lone[m], "disc", [True], ())
            wantG = TR.Trainer.adam_schedule_np(lone[m], "gen", [True], ())
            assert wantD.shape == (1, nD, 3) and wantG.shape == (1, nG, 3)
            assert tabD[m].tobytes() == wantD[0].tobytes(), (call, m)
            assert tabG[m].tobytes() == wantG[0].tobytes(), (call, m)
            assert fs.steps[m].tolist() == [t["step"] for t in lone[m].tensors], (call, m)
    assert (fs.steps[:, tr_cols] == tr0).all()       # the transformer's counts are not touched
    assert fs.gan_tables(None)[0].all()              # None: every cell


@pytest.mark.parametrize("H, M", [(8, 1), (16, 5), (8, 301), (16, 7), (16, 3)])
@pytest.mark.parametrize("envs", [False, True])
def test_gan_staging_offsets_are_8_byte_aligned(H, M, envs):
    from preganplus_amd import simulate as SIM
    lay, total = TR.fleet_gan_staging_layout(H, M, 4, 4, envs)
    names = ["emb", "sched", "active", "target", "tabD", "tabG"] + (["envs"] if envs else [])
    assert [p[0] for p in lay] == names              # [emb..active] goes up before graph A, [active..tabG] before B
    olay, ototal = TR.fleet_gan_output_layout(H, M, envs)
    assert [p[0] for p in olay] == ["ns", "probs", "probs_gen", "probs_after"] + (["sim"] if envs else [])
    for parts, tot in ((lay, total), (olay, ototal)):
        end = 0
        for name, dt, shp, off, nb in parts:
            assert off % 8 == 0 and off >= end, name
            assert nb == int(np.prod(shp)) * np.dtype(dt).itemsize
            end = off + nb
        assert tot % 8 == 0 and tot >= end
    shapes = {p[0]: (p[1], p[2]) for p in lay + olay}
    assert shapes["emb"] == (np.float32, (M, 2 * H)) and shapes["sched"] == (np.float32, (M, H, H))
    assert shapes["active"] == (np.int32, (M,)) and shapes["target"] == (np.float32, (M, 2))
    assert shapes["tabD"] == (np.float32, (M, 4, 3)) and shapes["ns"] == (np.float32, (M, H, H))
    if envs:
        assert shapes["envs"] == (np.float64, (M, SIM.env_len(H))) and shapes["sim"] == (np.float64, (M, 4))


# ---- the argument checks of the entries: all refused before anything is enqueued (NULL / host pointers) ----

def _sections(H):
    L = _lib()
    return L.pgp_master_offset(H, 1), L.pgp_master_offset(H, 2), L.pgp_master_len(H)   # gen, disc, end


def _fwd(H=16, M=2, ptr=None):
    return _lib().pgp_gan_forward1_many(H, M, None, ptr, ptr, ptr, ptr, ptr, ptr, None)


def _step(H=16, M=2, ptr=None, disc=None, gen=None, n_disc=None, n_gen=None, stride_d=12, stride_g=12):
    go, do, end = _sections(H) if H in (8, 16) else (0, 0, 0)
    disc = ((do, 10),) if disc is None else disc
    gen = ((go, 10),) if gen is None else gen
    arr = lambda ts: (TR._AdamTensor * max(len(ts), 1))(*[TR._AdamTensor(o, c, 1, 0.0, 0.0) for o, c in ts])
    return _lib().pgp_gan_step1_many(H, M, None, ptr, ptr, ptr, ptr, ptr, 5e-5, 5e-5, 1e-5, 0.9, 0.999, 1e-8,
                                     arr(disc), len(disc) if n_disc is None else n_disc, ptr, stride_d,
                                     arr(gen), len(gen) if n_gen is None else n_gen, ptr, stride_g,
                                     ptr, ptr, ptr, None)


@pytest.fixture
def fake():
    """A host pointer: not device memory, so a call that got past its checks could not have worked — every use
    below must be refused by a check."""
    buf = np.zeros(8, dtype=np.float64)
    yield buf.ctypes.data_as(ctypes.c_void_p)
    assert not buf.any()


@pytest.mark.parametrize("H", [32, 50, 0, -8])
def test_other_host_counts_are_unsupported(H, fake):
    for M in (2, 0):
        assert _fwd(H=H, M=M) == ERR_UNSUPPORTED
        assert _step(H=H, M=M) == ERR_UNSUPPORTED
    assert _fwd(H=H, ptr=fake) == ERR_UNSUPPORTED
    assert _step(H=H, ptr=fake) == ERR_UNSUPPORTED


def test_no_cells_is_ok_and_launches_nothing():
    for H in (8, 16):
        assert _fwd(H=H, M=0) == OK
        assert _step(H=H, M=0) == OK


@pytest.mark.parametrize("H", [8, 16])
def test_bad_arguments(H, fake):
    go, do, end = _sections(H)
    assert 0 < go < do < end
    assert _fwd(H=H, M=-1) == ERR_ARG
    assert _step(H=H, M=-1) == ERR_ARG
    assert _fwd(H=H) == ERR_ARG                        # cells and NULL arrays
    assert _step(H=H) == ERR_ARG
    for n in (-1, 49):
        assert _step(H=H, ptr=fake, n_disc=n) == ERR_ARG
        assert _step(H=H, ptr=fake, n_gen=n) == ERR_ARG
    assert _step(H=H, ptr=fake, stride_d=-1) == ERR_ARG
    assert _step(H=H, ptr=fake, stride_g=-3) == ERR_ARG
    assert _step(H=H, ptr=fake, disc=((go, 10),)) == ERR_ARG          # a disc tensor placed in the gen section
    assert _step(H=H, ptr=fake, gen=((do, 10),)) == ERR_ARG           # and the reverse
    assert _step(H=H, ptr=fake, disc=((do - 1, 10),)) == ERR_ARG      # straddling the boundary
    assert _step(H=H, ptr=fake, gen=((do - 5, 10),)) == ERR_ARG
    assert _step(H=H, ptr=fake, disc=((end - 5, 10),)) == ERR_ARG     # past the slot
    assert _step(H=H, ptr=fake, gen=((0, 10),)) == ERR_ARG            # in the transformer section
    assert _step(H=H, ptr=fake, disc=((do, -1),)) == ERR_ARG
    assert b"" != _lib().pgp_last_error()


def test_train_gan_needs_exactly_one_score_source():
    """Both or neither of simulate= / envs=: refused before anything else is touched (a stand-in has no device)."""
    ft = types.SimpleNamespace(M=2, H=16)
    sims = [lambda s: 0.0] * 2
    with pytest.raises(ValueError):
        TR.FleetTuner.train_gan(ft, None, None)
    with pytest.raises(ValueError):
        TR.FleetTuner.train_gan(ft, None, None, simulate=sims, envs=np.zeros((2, 322)))


def test_kept_tuning_errors_do_not_tie_the_tuner_into_a_cycle():
    """results() keeps the ZeroDivisionError of a cell without a positive label (the fleet plugin hands it on).
    Kept with its traceback it would reference results()'s frame and so the tuner: the tuner, its graphs and
    pinned buffers would then wait for the cyclic collector, which may run inside a later stream capture.  On a
    stand-in with the fields results() touches: reference counting alone must free it."""
    import gc
    import weakref

    class Tuner:
        pass

    def run():
        M, n, H, K = 2, 2, 8, 16
        ft = Tuner()
        ft.M, ft.H, ft.K = M, H, K
        ft.states = [TR.TuneState(np.full((K, 2), 0.5)) for _ in range(M)]
        ft.tune_errors = {}
        S = 2 * K + 3
        g = types.SimpleNamespace(n=n, score=True, state=None, o_state=2 * n * M, o_lg=2 * n * M + M * S,
                                  o_pr=2 * n * M + M * S + 2 * n * H * M)
        out = np.zeros(g.o_pr + 2 * n * H * M)
        out[g.o_state:g.o_lg] = np.stack([s.vector() for s in ft.states]).reshape(-1)
        none = np.zeros((M, n, H), dtype=np.int32)        # no positive label: accuracy_scores divides by zero
        res = TR.FleetTuner.results(ft, g, out, none, none, np.ones(M, dtype=bool))
        assert all(r[1] is None for r in res)
        assert [type(ft.tune_errors[c]) for c in range(M)] == [ZeroDivisionError] * M
        assert all(e.__traceback__ is None for e in ft.tune_errors.values())
        return weakref.ref(ft)

    was = gc.isenabled()
    gc.disable()
    try:
        assert run()() is None
    finally:
        if was:
            gc.enable()


def test_fleet_plugin_refuses_other_host_counts():
    from preganplus_amd.recovery import PreGANPlusFleetRecovery
    for H in (32, 50, 64):
        with pytest.raises(ValueError):
            PreGANPlusFleetRecovery(H, [{}], [None])
