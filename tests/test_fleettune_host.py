"""The host side of the fleet tuner (preganplus_amd/train.py: FleetSchedule,
fleet_staging_layout) and the cell-indexed entries of the C-ABI
(include/preganplus.h: pgp_tune_step1_many, pgp_adamw_table_many,
pgp_tune_forward_cells, pgp_forward1_many).  CPU: loads the library, makes no
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
NEW = ("pgp_tune_step1_many", "pgp_adamw_table_many", "pgp_tune_forward_cells", "pgp_forward1_many")
_lib = _native.lib


def test_header_declares_and_library_exports():
    with open(os.path.join(ROOT, "include", "preganplus.h")) as f:
        hdr = f.read()
    L = _native.lib()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert hasattr(L, name), name
    assert "#define PGP_ABI_VERSION 1" in hdr and L.pgp_abi_version() == 1   # additions only
    # every new entry cites the reference lines it stands for
    for name in NEW:
        at = hdr.index("int " + name)
        comment = hdr[hdr.rindex("/*", 0, at):at]
        assert "train.py" in comment or "PreGANPlus.py" in comment, name


def test_binding_argument_counts_match_the_header():
    """The ctypes argtypes lists are as long as the header's parameter lists."""
    with open(os.path.join(ROOT, "include", "preganplus.h")) as f:
        hdr = f.read()
    L = _lib()
    for name in NEW:
        m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\);", hdr, re.S)
        assert len(getattr(L, name).argtypes) == len(m.group(1).split(",")), name


# ---- the AdamW tables and count advances against Trainer.adam_schedule_np, cell by cell ----

def _lone(H, steps0):
    """A stand-in with the fields Trainer.adam_schedule_np reads (a Trainer needs a device)."""
    tensors = [dict(t, step=float(s)) for t, s in zip(TR.master_tensors(H), steps0)]
    return types.SimpleNamespace(tensors=tensors, lrs=TR.default_lrs(H), b1=0.9, b2=0.999)


@pytest.mark.parametrize("H", [8, 16])
def test_tables_equal_the_lone_schedule(H):
    M, rng = 5, np.random.RandomState(H)
    fs = TR.FleetSchedule(H, M)
    nt = len(fs.tensors)
    fs.steps[4] = rng.randint(0, 40, nt)            # a cell that starts from non-zero counts
    fs.steps[2, fs.base_col] = 7
    lone = [_lone(H, fs.steps[m]) for m in range(M)]
    for call, n in enumerate((3, 1, 10)):
        positive = rng.rand(M, n) < 0.5
        positive[1] = False                          # cell 1: no positive label, its prototype decoder lags
        active = np.array([True, True, True, call == 1, True])
        before = fs.steps.copy()
        bases = fs.drop_bases()
        tab = fs.tables(positive, active)
        assert tab.shape == (M, n, len(fs.sel), 3) and tab.dtype == np.float32
        for m in range(M):
            if not active[m]:
                assert not tab[m].any() and (fs.steps[m] == before[m]).all()
                continue
            assert bases[m] == int(before[m, fs.base_col])     # the dropout base, before the counts advance
            want = TR.Trainer.adam_schedule_np(lone[m], "transformer", positive[m], TR.COND_TENSORS)
            assert tab[m].tobytes() == want.tobytes(), (call, m)
            assert fs.steps[m].tolist() == [t["step"] for t in lone[m].tensors], (call, m)
    cond = [i for i, t in enumerate(fs.tensors) if t["name"] in TR.COND_TENSORS]
    assert len(cond) == 2 and (fs.steps[1, cond] == 0).all() and fs.steps[1, fs.base_col] == 14   # 3 + 1 + 10
    assert (fs.steps[:, [i for i, t in enumerate(fs.tensors) if t["section"] != "transformer"]]
            == before[:, [i for i, t in enumerate(fs.tensors) if t["section"] != "transformer"]]).all()


def test_master_tensors_cover_the_master_buffer():
    L = _lib()
    for H in TR.FUSED_STEP_HOSTS:
        t = TR.master_tensors(H)
        assert t[0]["offset"] == 0 and all(a["offset"] + a["n"] == b["offset"] for a, b in zip(t, t[1:]))
        assert t[-1]["offset"] + t[-1]["n"] == L.pgp_master_len(H)
        assert [x["name"] for x in t if not x["trainable"]] == ["pos_encoder.pe"]


@pytest.mark.parametrize("H, M, n, K", [(8, 1, 1, 3), (16, 5, 3, 16), (8, 300, 2, 16), (16, 7, 10, 5), (16, 3, 1, 4)])
def test_staging_offsets_are_8_byte_aligned(H, M, n, K):
    T = len(TR.FleetSchedule(H, 1).sel)
    lay, total = TR.fleet_staging_layout(H, M, n, K, T)
    assert [p[0] for p in lay] == ["W", "Y", "C", "sched", "active", "state", "rng"]
    end = 0
    for name, dt, shp, off, nb in lay:
        assert off % 8 == 0 and off >= end, name
        assert nb == int(np.prod(shp)) * np.dtype(dt).itemsize
        end = off + nb
    assert total % 8 == 0 and total >= end
    shapes = {p[0]: p[2] for p in lay}
    assert shapes["W"] == (M, n, 3, 3 * H) and shapes["sched"] == (M, n, T, 3) and shapes["state"] == (M, 2 * K + 3)
    assert shapes["active"] == (M,) and shapes["rng"] == (M, 2)


# ---- the argument checks of the entries: all refused before anything is enqueued (NULL arrays, no device) ----

def _step(H=16, K=16, M=2, n=3, step=0, p=0.0, ptr=None, rng=None):
    return _lib().pgp_tune_step1_many(H, K, M, n, step, None, ptr, ptr, ptr, ptr, ptr, ptr, 0.02, 0.995, ptr, ptr, ptr,
                                      p, rng, None)


def _adamw(M=2, slot=100, ptr=None, tensors=((0, 10),), nt=None, stride=3):
    arr = (TR._AdamTensor * max(len(tensors), 1))(*[TR._AdamTensor(o, c, 1, 0.0, 0.0) for o, c in tensors])
    return _lib().pgp_adamw_table_many(M, slot, None, ptr, ptr, ptr, ptr, 1e-4, 1e-5, 0.9, 0.999, 1e-8, arr,
                                       len(tensors) if nt is None else nt, ptr, stride, None)


def _fwd(H=16, M=2, n=3, ptr=None):
    return _lib().pgp_tune_forward_cells(H, M, n, None, ptr, ptr, ptr, ptr, None)


def _infer(H=16, K=16, M=2, ptr=None):
    return _lib().pgp_forward1_many(H, K, M, None, *([ptr] * 12), None)


@pytest.mark.parametrize("H", [32, 50, 0, -8])
def test_other_host_counts_are_unsupported(H):
    assert _step(H=H) == ERR_UNSUPPORTED
    assert _step(H=H, M=0) == ERR_UNSUPPORTED
    assert _fwd(H=H) == ERR_UNSUPPORTED
    assert _infer(H=H) == ERR_UNSUPPORTED


def test_no_cells_is_ok_and_launches_nothing():
    for H in (8, 16):
        assert _step(H=H, M=0) == OK
        assert _fwd(H=H, M=0) == OK
        assert _fwd(H=H, n=0) == OK
        assert _infer(H=H, M=0) == OK
    assert _adamw(M=0) == OK


def test_bad_arguments():
    assert _step(M=-1) == ERR_ARG
    assert _step(n=-1) == ERR_ARG
    assert _step(step=-1) == ERR_ARG
    assert _step(step=3) == ERR_ARG            # outside [0, n_steps)
    assert _step(n=0, step=0) == ERR_ARG
    assert _step(M=0, step=3) == ERR_ARG       # the step's range is checked whatever the fleet's size
    for p in (-0.1, 1.0, 1.5, float("nan")):
        assert _step(p=p) == ERR_ARG
    assert _step(K=2) == ERR_ARG               # triplet_loss needs prototypes 0-2
    assert _step() == ERR_ARG                  # cells and NULL arrays
    assert _fwd(M=-1) == ERR_ARG
    assert _fwd(n=-1) == ERR_ARG
    assert _fwd(M=65536) == ERR_ARG
    assert _fwd() == ERR_ARG
    assert _infer(M=-1) == ERR_ARG
    assert _infer(K=0) == ERR_ARG
    assert _infer(K=65) == ERR_ARG
    assert _infer() == ERR_ARG
    assert _adamw(M=-1) == ERR_ARG
    assert _adamw(slot=-1) == ERR_ARG
    assert _adamw(stride=-1) == ERR_ARG
    assert _adamw(nt=-1) == ERR_ARG
    assert _adamw(nt=49) == ERR_ARG
    assert _adamw() == ERR_ARG                 # cells and NULL arrays


def test_dropout_needs_the_rng_words():
    """p > 0 with every array but rng: refused; nothing can have been launched (the pointers are not device memory)."""
    buf = np.zeros(8, dtype=np.float64)
    fake = buf.ctypes.data_as(ctypes.c_void_p)
    assert _step(p=0.1, ptr=fake, rng=None) == ERR_ARG


def test_adamw_tensor_outside_the_slot():
    buf = np.zeros(8, dtype=np.float64)
    fake = buf.ctypes.data_as(ctypes.c_void_p)
    assert _adamw(ptr=fake, slot=100, tensors=((95, 10),)) == ERR_ARG
    assert _adamw(ptr=fake, slot=100, tensors=((-1, 10),)) == ERR_ARG
    assert _adamw(ptr=fake, slot=100, tensors=((0, -1),)) == ERR_ARG


def test_fleet_tuner_refuses_other_host_counts():
    for H in (32, 50, 64):
        with pytest.raises(ValueError):
            TR.FleetTuner(H, [{}])
    with pytest.raises(ValueError):
        TR.FleetTuner(16, [{}], dropout=1.0)
    with pytest.raises(ValueError):
        TR.FleetTuner(16, [])
    with pytest.raises(ValueError):
        TR.FleetTuner(16, [{}, {}], dropout_seeds=[1])
    with pytest.raises(ValueError):
        TR.FleetTuner(16, [{}, {}], extras=[None])
