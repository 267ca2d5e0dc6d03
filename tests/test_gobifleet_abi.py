"""The fleet entries of the C-ABI (include/preganplus.h: pgp_gobi_train_steps_many
/ _eval_many, pgp_gobi_plan_groups, ...) and the Python layer's own checks
(preganplus_amd/gobitrain.py, gobi.py).  Every check here runs on the host
before anything is enqueued.  CPU: loads the library, makes no GPU call."""
import ctypes
import os
import re

import numpy as np
import pytest

from preganplus_amd import _native
from preganplus_amd import gobi as GB
from preganplus_amd import gobitrain as GT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -2
VP = ctypes.c_void_p
NEW = ("pgp_gobi_train_steps_many", "pgp_gobi_train_eval_many", "pgp_gobi_create_many", "pgp_gobi_model_count",
       "pgp_gobi_set_model", "pgp_gobi_optimize_groups", "pgp_gobi_plan_groups")
_lib = _native.lib


def test_header_declares_and_library_exports():
    with open(os.path.join(ROOT, "include", "preganplus.h")) as f:
        hdr = f.read()
    L = _native.lib()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert hasattr(L, name), name
    assert "#define PGP_ABI_VERSION 1" in hdr and L.pgp_abi_version() == 1   # additions only
    m = re.search(r"typedef struct pgp_gobi_job \{(.*?)\} pgp_gobi_job;", hdr, re.S)
    fields = re.findall(r"\b(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    assert tuple(fields) == GT.JOB_DTYPE.names and GT.JOB_DTYPE.itemsize == 72   # the Python table is the C struct


# ---- pgp_gobi_plan_groups against a restatement ----

def plan_ref(model_of, n_models):
    """Ascending model, ascending environment id within it, four per group, -1 padding."""
    out = []
    for m in range(n_models):
        envs = [e for e, mm in enumerate(model_of) if mm == m]
        for k in range(0, len(envs), 4):
            four = envs[k:k + 4]
            out.append([m] + four + [-1] * (4 - len(four)))
    return out


def _plan(model_of, n_models, cap=None):
    mo = np.asarray(model_of, dtype=np.int32)
    cap = (len(mo) + 3) // 4 + n_models if cap is None else cap
    table = np.full((max(cap, 1), 5), -7, dtype=np.int32)
    g = _lib().pgp_gobi_plan_groups(len(mo), mo.ctypes.data_as(VP), n_models, table.ctypes.data_as(VP), cap)
    return g, table


@pytest.mark.parametrize("model_of, n_models", [
    ([], 3),                                     # E = 0
    ([0] * 9, 1),                                # one model
    ([0, 1, 2, 0, 0, 1, 2, 2, 2, 2, 2], 3),      # the issue's example
    ([0, 3, 3, 0, 3, 3, 3], 4),                  # models 1 and 2 have no environment
    (list(np.random.RandomState(5).randint(0, 7, 61)), 7),
])
def test_plan_groups(model_of, n_models):
    g, table = _plan(model_of, n_models)
    want = plan_ref(model_of, n_models)
    assert g == len(want)
    assert table[:g].tolist() == want
    assert (table[g:] == -7).all()               # nothing past the groups is written
    g2, table2 = _plan(model_of, n_models, cap=len(want))   # the exact cap is enough
    assert g2 == g and table2[:g].tolist() == want


def test_plan_groups_example():
    g, table = _plan([0, 1, 2, 0, 0, 1, 2, 2, 2, 2, 2], 3)
    assert table[:g].tolist() == [[0, 0, 3, 4, -1], [1, 1, 5, -1, -1], [2, 2, 6, 7, 8], [2, 9, 10, -1, -1]]


@pytest.mark.parametrize("model_of, n_models, cap", [
    ([0, 1, 3], 3, None),        # an index >= n_models
    ([0, -1, 1], 3, None),       # a negative index
    ([0, 1, 2, 0, 0, 1, 2, 2, 2, 2, 2], 3, 3),   # four groups, room for three
    ([0], 1, 0),
])
def test_plan_groups_bad(model_of, n_models, cap):
    g, table = _plan(model_of, n_models, cap)
    assert g == ERR_ARG
    assert (table == -7).all()   # all or nothing


# ---- pgp_gobi_train_steps_many / _eval_many: the argument checks ----

def _jobs(n_models=3, **over):
    """Three valid jobs over a pool of 10 samples and 12 steps; over: fields of job 1."""
    jobs = np.zeros(n_models, dtype=GT.JOB_DTYPE)
    for m in range(n_models):
        jobs[m] = (2 * m, 4 * m, 0, 4, 4, 1e-4, 1e-5, 0.9, 0.999, 1e-8)
    for k, val in over.items():
        jobs[1][k] = val
    return jobs


def _steps(jobs, H=16, n_models=None, pool=10, steps=12, ptr=None, jobs_null=False):
    n_models = len(jobs) if n_models is None else n_models
    j = None if jobs_null else jobs.ctypes.data_as(VP)
    return _lib().pgp_gobi_train_steps_many(H, n_models, j, pool, ptr, ptr, steps, ptr, ptr, ptr, ptr, ptr, ptr, None)


def _eval(jobs, H=16, n_models=None, pool=10, steps=12, ptr=None, jobs_null=False):
    n_models = len(jobs) if n_models is None else n_models
    j = None if jobs_null else jobs.ctypes.data_as(VP)
    return _lib().pgp_gobi_train_eval_many(H, n_models, j, pool, ptr, ptr, steps, ptr, ptr, ptr, ptr, None)


def _idle(jobs):
    jobs["n"] = 0
    return jobs


@pytest.mark.parametrize("H", [8, 50, 0])
def test_other_host_counts_are_unsupported(H):
    assert _steps(_idle(_jobs()), H=H) == ERR_UNSUPPORTED
    assert _eval(_idle(_jobs()), H=H) == ERR_UNSUPPORTED
    assert _steps(_jobs(), H=H, n_models=0) == ERR_UNSUPPORTED
    h = VP()
    w = np.zeros(61890, dtype=np.float32)
    assert _lib().pgp_gobi_create_many(H, 1, w.ctypes.data_as(VP), w.size, ctypes.byref(h)) == ERR_UNSUPPORTED
    assert not h.value


def test_no_work_is_ok_and_launches_nothing():
    """NULL pointers and no device: nothing may be touched."""
    assert _steps(_jobs(), n_models=0, jobs_null=True) == OK
    assert _eval(_jobs(), n_models=0, jobs_null=True) == OK
    assert _steps(_idle(_jobs())) == OK      # every job has n = 0
    assert _eval(_idle(_jobs())) == OK


SCALAR_RULES = [dict(n=-1), dict(n_samples=-1), dict(step0=-1), dict(lr=0.0), dict(lr=-1e-4), dict(lr=float("nan")),
                dict(weight_decay=-1e-5), dict(beta1=1.0), dict(beta1=-0.1), dict(beta2=1.0), dict(beta2=1.5),
                dict(eps=-1e-8)]
RANGE_RULES = [dict(sample_off=-1), dict(sample_off=7), dict(sample_off=11, n_samples=0), dict(n_samples=9),
               dict(order_off=-1), dict(order_off=9), dict(order_off=13, n=0), dict(n=9),
               dict(sample_off=2 ** 62, n_samples=2 ** 31 - 1), dict(order_off=2 ** 62, n=2 ** 31 - 1)]


def _refused_job_1(rc):
    """ERR_ARG, and the message names job 1: the rule refused it, not the NULL pointers."""
    assert rc == ERR_ARG
    assert b"job 1:" in _native.lib().pgp_last_error()


@pytest.mark.parametrize("over", SCALAR_RULES + RANGE_RULES)
def test_steps_many_bad_job(over):
    """One bad field in job 1 of three refuses the whole call, whether or not
    the other jobs have work (every pointer is NULL: nothing can be launched)."""
    _refused_job_1(_steps(_jobs(**over)))
    idle = _jobs(**over)
    idle["n"][[0, 2]] = 0
    _refused_job_1(_steps(idle))


@pytest.mark.parametrize("over", [dict(n=-1), dict(n_samples=-1)] + RANGE_RULES)
def test_eval_many_bad_job(over):
    _refused_job_1(_eval(_jobs(**over)))
    idle = _jobs(**over)
    idle["n"][[0, 2]] = 0
    _refused_job_1(_eval(idle))


def test_eval_many_ignores_the_optimizer_scalars():
    assert _eval(_idle(_jobs(lr=0.0, step0=-1, beta1=2.0))) == OK


def test_negative_counts_and_null_pointers():
    assert _steps(_idle(_jobs()), n_models=-1) == ERR_ARG
    assert _steps(_idle(_jobs()), pool=-1) == ERR_ARG
    assert _steps(_idle(_jobs()), steps=-1) == ERR_ARG
    assert _eval(_idle(_jobs()), n_models=-1) == ERR_ARG
    assert _eval(_idle(_jobs()), pool=-1) == ERR_ARG
    assert _eval(_idle(_jobs()), steps=-1) == ERR_ARG
    assert _steps(_jobs(), jobs_null=True) == ERR_ARG     # models but no table
    assert _eval(_jobs(), jobs_null=True) == ERR_ARG
    assert _steps(_jobs()) == ERR_ARG                     # work to do and NULL pointers: an argument error, no launch
    assert _eval(_jobs()) == ERR_ARG
    one = _idle(_jobs())
    one["n"][2] = 1                                       # a single step in the last job is work
    assert _steps(one) == ERR_ARG
    assert _eval(one) == ERR_ARG


def test_handle_entries_refuse_null():
    L = _lib()
    w = np.zeros(61890, dtype=np.float32)
    assert L.pgp_gobi_model_count(None) == 0
    assert L.pgp_gobi_set_model(None, 0, w.ctypes.data_as(VP), w.size) == ERR_ARG
    assert L.pgp_gobi_optimize_groups(None, 4, 1, None, None, None, None, None, 0, None, None) == ERR_ARG
    h = VP()
    assert L.pgp_gobi_create_many(16, 0, w.ctypes.data_as(VP), 0, ctypes.byref(h)) == ERR_ARG
    assert L.pgp_gobi_create_many(16, 2, w.ctypes.data_as(VP), w.size, ctypes.byref(h)) == ERR_ARG   # one model's floats
    assert L.pgp_gobi_create_many(16, 1, None, w.size, ctypes.byref(h)) == ERR_ARG
    assert not h.value


# ---- the Python layer's own checks (host only) ----

def _data(n):
    return np.zeros((n, 16, 18)), np.zeros((n, 2), dtype=np.float32)


def test_fleet_state_checks():
    with pytest.raises(ValueError):
        GT.fleet_state()
    with pytest.raises(ValueError):
        GT.fleet_state(weights=[GT.fresh_weights(1)], seeds=[1])
    with pytest.raises(ValueError):
        GT.fleet_state(weights=[])
    with pytest.raises(ValueError):
        GT.fleet_state(seeds=[1, 2], states=[None])
    with pytest.raises(ValueError):
        GT.fleet_state(seeds=[1, 2], hyper=[{"lr": 1e-3}])
    with pytest.raises(ValueError):
        GT.fleet_state(seeds=[1], hyper={"learning_rate": 1e-3})
    bad = GT.fresh_weights(1)
    bad["find.2.bias"] = np.zeros(64, dtype=np.float32)
    with pytest.raises(ValueError):
        GT.fleet_state(weights=[GT.fresh_weights(1), bad])
    P, m, v, steps, hy = GT.fleet_state(seeds=[16, 17], hyper=[None, {"lr": 3e-4}])
    assert P.shape == (2, 61890) and P.dtype == np.float32 and not m.any() and not v.any() and steps == [0, 0]
    assert hy[0]["lr"] == GT.LR and hy[1]["lr"] == 3e-4 and hy[1]["weight_decay"] == GT.WEIGHT_DECAY
    w16 = GT.fresh_weights(16)
    assert P[0].tobytes() == np.concatenate([w16[k].reshape(-1) for k in GB._ORDER]).tobytes()
    ck = GT.checkpoint_dict(P[1], np.ones(61890), np.ones(61890), 12, 0, [], lr=5e-4)
    _, m2, _, steps2, hy2 = GT.fleet_state(weights=[w16, w16], states=[None, ck["optimizer_state_dict"]])
    assert steps2 == [0, 12] and hy2[1]["lr"] == 5e-4 and m2[1].all() and not m2[0].any()


def test_pool_datasets_checks():
    f, t, off, size, dof = GT.pool_datasets([_data(5), _data(3)], None, 2)
    assert f.shape == (8, 16, 18) and f.dtype == np.float32 and t.shape == (8, 2)
    assert off == [0, 5] and size == [5, 3] and dof == [0, 1]
    assert GT.pool_datasets([_data(5)], None, 3)[4] == [0, 0, 0]
    assert GT.pool_datasets([_data(5), _data(3)], [1, 1, 0], 3)[4] == [1, 1, 0]
    with pytest.raises(ValueError):
        GT.pool_datasets([], None, 1)
    with pytest.raises(ValueError):
        GT.pool_datasets([_data(5), _data(3)], None, 3)          # which model trains on which?
    with pytest.raises(ValueError):
        GT.pool_datasets([_data(5), _data(3)], [0, 1], 3)        # dataset_of's length
    with pytest.raises(ValueError):
        GT.pool_datasets([_data(5), _data(3)], [0, 2], 2)        # dataset_of's range
    with pytest.raises(ValueError):
        GT.pool_datasets([(np.zeros((5, 16, 17)), np.zeros((5, 2)))], None, 1)
    with pytest.raises(ValueError):
        GT.pool_datasets([(np.zeros((5, 16, 18)), np.zeros((4, 2)))], None, 1)


def test_fleet_jobs_checks():
    hy = GT.fleet_state(seeds=[1, 2, 3])[4]
    jobs, pool = GT.fleet_jobs([[0, 4, 1], [], [2, 2]], [0, 0, 5], [5, 5, 3], [0, 7, 0], hy)
    assert pool.dtype == np.int32 and pool.tolist() == [0, 4, 1, 2, 2]
    assert jobs["order_off"].tolist() == [0, 3, 3] and jobs["n"].tolist() == [3, 0, 2]
    assert jobs["sample_off"].tolist() == [0, 0, 5] and jobs["step0"].tolist() == [0, 7, 0]
    assert jobs["lr"].tolist() == [GT.LR] * 3
    with pytest.raises(ValueError):
        GT.fleet_jobs([[0], [1]], [0, 0, 5], [5, 5, 3], [0, 0, 0], hy)
    with pytest.raises(IndexError):
        GT.fleet_jobs([[0], [1], [3]], [0, 0, 5], [5, 5, 3], [0, 0, 0], hy)   # model 2's dataset has 3 samples
    with pytest.raises(IndexError):
        GT.fleet_jobs([[-1], [1], [0]], [0, 0, 5], [5, 5, 3], [0, 0, 0], hy)


def test_model_of_checks():
    assert GB.check_model_of([0, 2, 1], 3, 3).dtype == np.int32
    assert GB.check_model_of([], 0, 1).shape == (0,)
    with pytest.raises(ValueError):
        GB.check_model_of([0, 1], 3, 3)              # length
    with pytest.raises(ValueError):
        GB.check_model_of([[0, 1, 2]], 3, 3)         # shape
    with pytest.raises(ValueError):
        GB.check_model_of([0, 3, 1], 3, 3)           # range
    with pytest.raises(ValueError):
        GB.check_model_of([0, -1, 1], 3, 3)
    with pytest.raises(ValueError):
        GB.check_model_of([0.0, 1.0, 2.0], 3, 3)     # not integers
