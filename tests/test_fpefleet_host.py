"""The FPE's epoch-per-launch and fleet entries, the host side: the header
declares pgp_fpe_train_steps / pgp_fpe_train_steps_many / pgp_fpe_forward_many_cells and
pgp_fpe_job, ``FPETrainer.adam_table`` holds the rows consecutive ``adam_step`` calls would
use, and every argument error is returned before anything is enqueued.  CPU: loads the
library, makes no GPU call."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from preganplus_amd import _native
from preganplus_amd import fpetrain as FT
from preganplus_amd import weights as W
from preganplus_amd.train import _AdamTensor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -2
ENTRIES = ("pgp_fpe_train_steps", "pgp_fpe_train_steps_many", "pgp_fpe_forward_many_cells")
VP = ctypes.c_void_p


def test_header_declares_and_library_exports():
    with open(os.path.join(ROOT, "include", "preganplus.h")) as f:
        hdr = f.read()
    L = _native.lib()
    for name in ENTRIES:
        assert re.search(rf"\bint\s+{name}\s*\(", hdr), name
        assert hasattr(L, name) and name in _native.SIGNATURES, name
    body = re.search(r"typedef\s+struct\s+pgp_fpe_job\s*\{(.*?)\}\s*pgp_fpe_job\s*;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    fields = [(t, n) for t, n in re.findall(r"(long long|int)\s+(\w+)\s*;", body)]
    assert fields == [("long long", "window_off"), ("long long", "step_off"), ("int", "n"), ("int", "reserved")]
    assert [(n, FT.JOB_DTYPE[n].str) for n in FT.JOB_DTYPE.names] == [
        ("window_off", "<i8"), ("step_off", "<i8"), ("n", "<i4"), ("reserved", "<i4")]
    assert FT.JOB_DTYPE.itemsize == 24 and [FT.JOB_DTYPE.fields[n][1] for n in FT.JOB_DTYPE.names] == [0, 8, 16, 20]
    assert [len(_native.SIGNATURES[n][1]) for n in ENTRIES] == [24, 28, 12]    # tests/test_abi_table.py: the kinds
    assert "#define PGP_ABI_VERSION 1" in hdr and L.pgp_abi_version() == 1   # an addition only


def tensor_list(H=16):
    out, off = [], 0
    for name, shp in W.fpe_shapes(H).items():
        n = int(np.prod(shp))
        out.append({"name": name, "shape": shp, "offset": off, "n": n, "step": 0.0})
        off += n
    return out


def test_adam_table_is_the_rows_of_consecutive_adam_steps():
    positive = (True, False, True, True, False, False)
    lr, b1, b2 = FT.FPE_LR, 0.9, 0.999
    a, b = tensor_list(), tensor_list()
    table = FT.adam_table(a, positive, lr, b1, b2)
    assert table.dtype == np.float32 and table.shape == (6, 16, 3)
    cond = [i for i, t in enumerate(b) if t["name"] in FT.COND]
    assert len(cond) == 2
    for i, p in enumerate(positive):
        # what adam_step puts in its descriptors: the shared function's doubles through ctypes' c_float
        desc = [_AdamTensor(t["offset"], t["n"], *r) for t, r in zip(b, FT.adam_rows(b, p, lr, b1, b2))]
        row = np.array([(d.active, d.step_size, d.bc2_sqrt) for d in desc], dtype=np.float32)
        np.testing.assert_array_equal(table[i].view(np.uint32), row.view(np.uint32), err_msg=f"step {i}")
        for k in range(16):
            assert table[i, k, 0] == (1.0 if p or k not in cond else 0.0)
    assert [t["step"] for t in a] == [t["step"] for t in b]
    assert {t["step"] for k, t in enumerate(a) if k in cond} == {3.0}       # the prototype decoder fell behind
    assert {t["step"] for k, t in enumerate(a) if k not in cond} == {6.0}
    # the arithmetic itself, for one row: torch's bias corrections of steps 3 (COND) and 4 (the others)
    for k in range(16):
        st = 3.0 if k in cond else 4.0
        assert table[3, k, 1] == np.float32(lr / (1 - b1 ** st)) and table[3, k, 2] == np.float32(math.sqrt(1 - b2 ** st))
    # a skipped tensor's row repeats the scalars of its last step; its count does not advance
    np.testing.assert_array_equal(table[4, cond, 1:], table[3, cond, 1:])
    np.testing.assert_array_equal(table[5, cond, 1:], table[3, cond, 1:])


# ---------------------------------------------------------------------------
# argument errors, on sentinel-filled HOST arrays: a launch on them would fault
# ---------------------------------------------------------------------------
H, K, M, NW, NS, NT = 16, 3, 3, 8, 12, 16
LEN = 11401
HYPER = dict(update_min=0.1, decay=0.9, lr=1e-4, weight_decay=1e-5, beta1=0.9, beta2=0.999, eps=1e-8)


class Host:
    def __init__(self):
        f = lambda shape, dt: np.full(shape, -7.25 if dt != np.int32 else -9, dtype=dt)
        self.a = {"windows": f((NW, 3, 3 * H), np.float32), "y": f((NW, H), np.int32), "cls": f((NW, H), np.int32),
                  "h0": f((NS, 3), np.float32), "sched": f((NS, NT, 3), np.float32), "loss": f((NS, 2), np.float64),
                  "P": f((M, LEN), np.float32), "G": f((M, LEN), np.float32), "exp_avg": f((M, LEN), np.float32),
                  "exp_avg_sq": f((M, LEN), np.float32), "state": f((M, 2 * K + 3), np.float64),
                  "probs": f((NS, H, 2), np.float64), "protos": f((NS, H, 2), np.float64),
                  "jobs_dev": np.full(M * 24, 0x5a, dtype=np.uint8)}
        self.before = {k: v.tobytes() for k, v in self.a.items()}
        self.jobs = np.zeros(M, dtype=FT.JOB_DTYPE)
        self.jobs[:] = [(0, 0, 6, 0), (0, 6, 0, 0), (2, 6, 6, 0)]
        self.tensors = (_AdamTensor * NT)(*[_AdamTensor(t["offset"], t["n"], 1, 0.0, 0.0) for t in tensor_list()])

    def p(self, k, null=()):
        return None if k in null else self.a[k].ctypes.data_as(VP)

    def unchanged(self):
        return {k: v.tobytes() for k, v in self.a.items()} == self.before

    def steps(self, L, H_=H, K_=K, n=6, nt=NT, tensors=None, null=(), **hy):
        h = dict(HYPER, **hy)
        t = None if "tensors" in null else (tensors or self.tensors)
        return L.pgp_fpe_train_steps(
            H_, K_, n, *[self.p(k, null) for k in ("windows", "h0", "y", "cls", "P", "G", "exp_avg", "exp_avg_sq", "state")],
            h["update_min"], h["decay"], h["lr"], h["weight_decay"], h["beta1"], h["beta2"], h["eps"], t, nt,
            self.p("sched", null), self.p("loss", null), None)

    def many(self, L, H_=H, K_=K, M_=M, jobs=None, nw=NW, ns=NS, nt=NT, tensors=None, null=(), **hy):
        h = dict(HYPER, **hy)
        j = self.jobs if jobs is None else jobs
        t = None if "tensors" in null else (tensors or self.tensors)
        return L.pgp_fpe_train_steps_many(
            H_, K_, M_, None if "jobs" in null else j.ctypes.data_as(VP), nw,
            *[self.p(k, null) for k in ("windows", "y", "cls")], ns,
            *[self.p(k, null) for k in ("h0", "sched", "loss", "P", "G", "exp_avg", "exp_avg_sq", "state")],
            h["update_min"], h["decay"], h["lr"], h["weight_decay"], h["beta1"], h["beta2"], h["eps"], t, nt,
            self.p("jobs_dev", null), None)

    def forward(self, L, H_=H, M_=M, jobs=None, nw=NW, ns=NS, null=()):
        j = self.jobs if jobs is None else jobs
        return L.pgp_fpe_forward_many_cells(
            H_, M_, None if "jobs" in null else j.ctypes.data_as(VP), nw, self.p("windows", null), ns,
            *[self.p(k, null) for k in ("h0", "P", "probs", "protos", "jobs_dev")], None)


def job_table(*rows):
    j = np.zeros(len(rows), dtype=FT.JOB_DTYPE)
    j[:] = list(rows)
    return j


def test_argument_errors_enqueue_nothing():
    L = _native.lib()
    x = Host()
    every = (x.steps, x.many, x.forward)
    # host counts: before everything else, whatever the rest is
    for h in (8, 32, 0, -1, 64):
        for call in every:
            assert call(L, H_=h) == ERR_UNSUPPORTED, (h, call.__name__)
        assert x.steps(L, H_=h, n=0) == ERR_UNSUPPORTED and x.many(L, H_=h, M_=0) == ERR_UNSUPPORTED
        assert x.forward(L, H_=h, M_=0) == ERR_UNSUPPORTED
    # counts and pool sizes
    assert x.steps(L, n=-1) == ERR_ARG
    for call in (x.many, x.forward):
        assert call(L, M_=-1) == ERR_ARG and call(L, nw=-1) == ERR_ARG and call(L, ns=-1) == ERR_ARG
    # scalars of the training entries
    for call in (x.steps, x.many):
        for bad in (dict(K_=0), dict(K_=-3), dict(lr=0.0), dict(lr=-1e-4), dict(lr=float("nan")),
                    dict(weight_decay=-1e-5), dict(eps=-1e-8), dict(beta1=1.0), dict(beta1=-0.1), dict(beta2=1.0),
                    dict(beta2=1.5), dict(beta2=-0.5), dict(nt=-1), dict(nt=49)):
            assert call(L, **bad) == ERR_ARG, (call.__name__, bad)
        # a tensor outside the slot
        for off, n in ((LEN - 1, 2), (-1, 4), (0, -1), (LEN + 1, 0), (0, LEN + 1)):
            t = (_AdamTensor * NT)(*x.tensors)
            t[5] = _AdamTensor(off, n, 1, 0.0, 0.0)
            assert call(L, tensors=t) == ERR_ARG, (call.__name__, off, n)
    # jobs
    for call in (x.many, x.forward):
        for bad in ((0, 0, 6, 1), (0, 0, -1, 0), (-1, 0, 6, 0), (0, -1, 6, 0), (NW - 5, 0, 6, 0), (0, NS - 5, 6, 0),
                    (NW + 1, 0, 0, 0), (0, NS + 1, 0, 0), (2 ** 40, 0, 1, 0), (0, 2 ** 40, 1, 0)):
            assert call(L, jobs=job_table((0, 0, 6, 0), bad, (2, 6, 6, 0))) == ERR_ARG, (call.__name__, bad)
        assert call(L, null=("jobs",)) == ERR_ARG
    # a NULL array while some job has steps
    for k in ("windows", "h0", "y", "cls", "P", "G", "exp_avg", "exp_avg_sq", "state", "sched", "loss", "tensors"):
        assert x.steps(L, null=(k,)) == ERR_ARG, k
        assert x.many(L, null=(k,)) == ERR_ARG, k
    assert x.many(L, null=("jobs_dev",)) == ERR_ARG
    for k in ("windows", "h0", "P", "probs", "protos", "jobs_dev"):
        assert x.forward(L, null=(k,)) == ERR_ARG, k
    assert L.pgp_last_error()
    # nothing to do: PGP_OK, no pointer is looked at
    nothing = ("windows", "h0", "y", "cls", "P", "G", "exp_avg", "exp_avg_sq", "state", "sched", "loss", "tensors",
               "probs", "protos", "jobs_dev")
    idle = job_table((0, 0, 0, 0), (NW, NS, 0, 0), (3, 3, 0, 0))
    for h in (16, 50):
        assert x.steps(L, H_=h, n=0, null=nothing) == OK
        assert x.many(L, H_=h, M_=0, null=nothing + ("jobs",)) == OK
        assert x.forward(L, H_=h, M_=0, null=nothing + ("jobs",)) == OK
        assert x.many(L, H_=h, jobs=idle, null=nothing) == OK and x.forward(L, H_=h, jobs=idle, null=nothing) == OK
    assert x.steps(L, n=0, nt=0, null=nothing) == OK
    assert x.unchanged()
