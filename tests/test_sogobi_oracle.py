"""Second-order GOBI on the CPU: the restatements of so_opt() that the GPU tests
compare against (tests/sogobi_ref.py) held to the reference's own run
(tests/golden/sogobi_h16.npz, made by tests/golden/make_golden_sogobi.py), the
sign packing and the Philox host statement, SOGOBIScheduler's host side, and
every argument error of pgp_gobi_so_optimize / _groups (nothing is enqueued)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import sogobi_ref as S
from oracle import gobi_oracle as GO
from preganplus_amd import _native
from preganplus_amd import gobi as GB

OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -2


def test_fp32_restatement_is_the_reference_bit_for_bit():
    """restate() in fp32 on the recorded probes: results and iterations of all 240
    environments and the first step's g, hv and pre-projection x, bit for bit."""
    f = S.fixture()
    sd, _ = GO.load(S.WEIGHTS)
    assert len(f["inits"]) == 240 and f["steps"].sum() == len(np.load(S.GOLD_SO)["sign_words"])
    for e in range(240):
        taps = []
        res, it = S.restate(sd, f["inits"][e], S.unpack_signs(f["signs"][e]), torch.float32, taps=taps)
        assert it == f["iterations"][e] and len(taps) == f["steps"][e], e
        assert np.array_equal(res.numpy(), f["results"][e]), e
        for k, name in enumerate(("g", "hv", "pre")):
            assert np.array_equal(taps[0][k].numpy(), f[name][e]), (e, name)


def test_fp64_restatement_reaches_the_same_schedules():
    """The fp64 trajectory on the same probes ends in the reference's fp32
    schedule with its iteration count in every environment (240 of 240), and its
    batched forward-over-reverse equals autograd's g and hv."""
    f, T = S.fixture(), S.fixture_trajectory()
    assert np.array_equal(T.result, f["results"].astype(np.float64))
    assert np.array_equal(T.iterations, f["iterations"])
    sd, _ = GO.load(S.WEIGHTS)
    for e in (0, 57, 239):
        taps = []
        res, it = S.restate(sd, f["inits"][e], S.unpack_signs(f["signs"][e]), torch.float64, taps=taps)
        assert it == T.iterations[e] and np.array_equal(res.numpy(), T.result[e])
        for s in range(3):
            for k, mine in enumerate((T.g, T.hv, T.pre)):
                ref = taps[s][k].numpy()
                assert np.abs(mine[s][e] - ref).max() <= 1e-12 * np.abs(ref).max(), (e, s, k)


def test_reference_own_error_at_step_1():
    """What the GPU tolerances rest on: the reference's fp32 g and hv at step 1
    (the fixture's taps) against fp64, max-normalised per environment, the worst
    of the 240: 1.05e-6 and 1.98e-6.  The GPU tests allow 4 times REF_ERR_*."""
    f, T = S.fixture(), S.fixture_trajectory()
    eg, eh = S.max_normalised(f["g"], T.g[0]).max(), S.max_normalised(f["hv"], T.hv[0]).max()
    print(f"reference fp32 vs fp64 at step 1: g {eg:.3e}  hv {eh:.3e}")
    assert 0.9 * S.REF_ERR_G <= eg <= S.REF_ERR_G
    assert 0.9 * S.REF_ERR_HV <= eh <= S.REF_ERR_HV
    assert S.TOL_G == 4 * S.REF_ERR_G and S.TOL_HV == 4 * S.REF_ERR_HV


def test_robust_shares_of_the_fixture():
    """The shares the GPU tests require of the fp64 trajectories at 4 x the
    reference's error: robust rows at step 1 (>= 90 %) and environments robust
    at every row of every step (>= 40 %); in all of the latter the reference's
    fp32 run is the fp64 one."""
    f, T = S.fixture(), S.fixture_trajectory()
    rows, envs = int(T.robust_rows1.sum()), int(T.qualifies.sum())
    print(f"robust rows at step 1: {rows} of 3840; qualifying environments: {envs} of 240")
    assert rows >= 0.9 * 3840 and envs >= 0.4 * 240


def test_sign_packing_and_philox_round_trip():
    rng = np.random.Generator(np.random.PCG64(3))
    v = 2.0 * rng.integers(0, 2, size=(5, 7, 16, 18)) - 1.0
    w = GB.pack_signs(v)
    assert w.dtype == np.uint32 and w.shape == (5, 7, 9)
    assert np.array_equal(GB.unpack_signs(w), v) and np.array_equal(S.unpack_signs(w), v)
    one = np.full((16, 18), -1.0)
    one[1, 15] = 1.0                      # entry k = 33: bit 1 of word 1
    assert GB.pack_signs(one).tolist() == [0, 2, 0, 0, 0, 0, 0, 0, 0]
    # Philox4x32-10 known answer (Random123 kat_vectors): counter 0, key 0
    assert int(GB._philox4x32_10_word0(0, 0, 0, 0)) == 0x6627E8D5
    s = GB.so_signs([0, 1, 2 ** 40 + 5, 2 ** 64 - 1], 200)
    assert s.dtype == np.uint32 and s.shape == (4, 200, 9)
    assert int(s[0, 0, 0]) == 0x6627E8D5                       # word 0, step 0, key 0
    assert np.array_equal(GB.so_signs([2 ** 40 + 5], 50)[0], s[2, :50])   # an environment's own seed alone
    assert len({s[i].tobytes() for i in range(4)}) == 4
    bits = GB.unpack_signs(s)
    assert abs(bits.mean()) < 0.01                              # 230k fair draws: |mean| ~ 0.002
    assert np.array_equal(GB.pack_signs(bits), s)


def test_sogobi_scheduler_host_side():
    """SOGOBIScheduler on a duck-typed environment with the optimiser stubbed:
    the init matrix is SOGOBI.py:19-33's, each call hands the optimiser a fresh
    seed of its own counter, result_cache is the result's allocation and the
    decision list is SOGOBI.py:35-39's over it."""

    class StubOpt:
        def __init__(self):
            self.seen = []

        def optimize_so(self, init, seeds=None, **kw):
            assert not kw and init.shape == (1, 16, 18)
            self.seen.append((np.array(init[0]), int(np.asarray(seeds)[0])))
            res = np.array(init, dtype=np.float32)
            res[0, :, 2:] = np.roll(res[0, :, 2:], 1, axis=1)   # every container moves one host on
            return torch.tensor(res), None, None

    sch = GB.SOGOBIScheduler.__new__(GB.SOGOBIScheduler)
    GB.Scheduler.__init__(sch)
    sch.opt, sch.max_container_ips, sch.hosts, sch.result_cache, sch.seed, sch.calls = StubOpt(), 4000.0, 16, None, 7, 0
    rng = np.random.Generator(np.random.PCG64(11))
    for trial in range(3):
        env = S.duck_env(rng, sch.max_container_ips)
        sch.setEnvironment(env)
        np.random.seed(trial)
        dec = sch.placement([])
        np.random.seed(trial)
        init, prev = sch.init_matrix()
        seen, seed = sch.opt.seen[-1]
        assert np.array_equal(seen, init) and seed == sch.call_seed(trial) == (7 << 32) + trial
        for c, cont in enumerate(env.containerlist):
            assert init[c, 0] == env.hostlist[c].getCPU() / 100
            assert init[c, 1] == (cont.getApparentIPS() / sch.max_container_ips if cont else 0)
            assert init[c, 2:].sum() == 1 and (cont is None or cont.h == -1 or init[c, 2 + cont.h] == 1)
        res = init.astype(np.float32)
        res[:, 2:] = np.roll(res[:, 2:], 1, axis=1)
        assert np.array_equal(sch.result_cache, res[:, 2:])
        assert dec == GO.decision(res, prev) and sch.selection() == []
        assert all(prev[cid] != h for cid, h in dec) and {cid for cid, _ in dec} == set(prev)
    assert GB.SOGOBIScheduler.run_SOGOBI is GB.GOBIScheduler.run_GOBI


def test_argument_errors_enqueue_nothing():
    """Every argument error of the two entries, on host pointers and without a
    handle: each returns before anything is enqueued (no device is touched)."""
    if not os.path.exists(_native.LIB_PATH):
        pytest.skip("the HIP library is not built")
    L = _native.lib()
    a = (ctypes.c_float * 8)()
    p = ctypes.cast(a, ctypes.c_void_p)

    def so(n_env=4, init=p, result=p, its=p, fit=p, max_iters=0, signs=None, sign_steps=0, seeds=None, g=None):
        rc = L.pgp_gobi_so_optimize(g, n_env, init, result, its, fit, max_iters, signs, sign_steps, seeds, None, None)
        return rc, L.pgp_gobi_last_error().decode()

    def sog(n_env=4, n_groups=1, groups=p, init=p, result=p, its=p, fit=p, max_iters=0, signs=None, sign_steps=0,
            seeds=None, g=None):
        rc = L.pgp_gobi_so_optimize_groups(g, n_env, n_groups, groups, init, result, its, fit, max_iters, signs,
                                           sign_steps, seeds, None, None)
        return rc, L.pgp_gobi_last_error().decode()

    for f in (so, sog):
        assert f(n_env=0, init=None, result=None, its=None, fit=None)[0] == OK      # nothing to do
        rc, msg = f(n_env=-1, seeds=p)
        assert rc == ERR_ARG and "negative" in msg
        for k in ("init", "result", "its", "fit"):
            rc, msg = f(seeds=p, **{k: None})
            assert rc == ERR_ARG and "NULL input/output" in msg, k
        for kw in ({}, {"signs": p, "seeds": p, "sign_steps": 200}):                # neither, both
            rc, msg = f(**kw)
            assert rc == ERR_ARG and "not both" in msg
        for kw in ({"sign_steps": 199}, {"sign_steps": 2, "max_iters": 3}, {"sign_steps": 0, "max_iters": 201}):
            rc, msg = f(signs=p, **kw)
            assert rc == ERR_ARG and "sign_steps" in msg, kw
        for kw in ({"signs": p, "sign_steps": 200}, {"signs": p, "sign_steps": 3, "max_iters": 3}, {"seeds": p}):
            rc, msg = f(**kw)                                                       # valid but for the handle
            assert rc == ERR_ARG and "NULL optimiser" in msg, kw
    assert sog(n_groups=-1, seeds=p)[0] == ERR_ARG
    rc, msg = sog(groups=None, seeds=p)
    assert rc == ERR_ARG and "group table" in msg
    assert sog(n_groups=0, groups=None, init=None, seeds=None)[0] == ERR_ARG        # the arrays are still checked
    # 16 hosts only: no handle of another host count can exist
    h = ctypes.c_void_p()
    w = np.zeros(8, np.float32)
    assert L.pgp_gobi_create(50, w.ctypes.data_as(ctypes.c_void_p), w.size, ctypes.byref(h)) == ERR_UNSUPPORTED
    assert not h.value


def test_python_layer_checks():
    """optimize_so's own checks come before the library call (a stub handle, no device)."""
    o = GB.GOBIOptimizer.__new__(GB.GOBIOptimizer)
    o.device = torch.device("cpu")
    x = np.zeros((2, 16, 18), np.float32)
    with pytest.raises(ValueError, match="not both"):
        o.optimize_so(x)
    with pytest.raises(ValueError, match="not both"):
        o.optimize_so(x, signs=np.zeros((2, 200, 9), np.uint32), seeds=[1, 2])
    with pytest.raises(ValueError, match="signs must be"):
        o.optimize_so(x, signs=np.zeros((2, 200, 8), np.uint32))
    with pytest.raises(ValueError, match="seeds must be"):
        o.optimize_so(x, seeds=[1, 2, 3])
    with pytest.raises(ValueError, match="init must be"):
        o.optimize_so(np.zeros((2, 16, 17), np.float32), seeds=[1, 2])


_LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "preganplus_amd", "_lib",
                    "libpreganplus.so")


@pytest.mark.skipif(not os.path.exists(_LIB) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"),
                    reason="built library / llvm-objdump absent")
@pytest.mark.parametrize("kernel", ["gobi_so_kernel", "gobi_so_groups_kernel"])
def test_so_kernels_dpp_sources_clear_of_valu_writes(kernel):
    """The second-order kernels reuse pgp_gobi.hpp's inline-asm row_newbcast
    chains, outside the compiler's hazard check: in the built kernel no VALU
    write of a DPP source sits within the 2 wait states the hardware needs
    (tools/dpp_hazard_check.py, as test_roofline_isa.py holds gobi_kernel)."""
    import re
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(_LIB)), "..", "tools"))
    import dpp_hazard_check
    import isa_count
    asm = isa_count._disasm(_LIB, kernel)
    m = re.search(rf"^[0-9a-f]+ <_ZN3pgp12_GLOBAL__N_1\d+{kernel}E[^>]*>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", asm, re.S | re.M)
    assert m is not None, f"{kernel} not found in the built library"
    n, found = dpp_hazard_check.check_insts(dpp_hazard_check.parse(m.group(1).split("\n")))
    assert n > 100, f"only {n} DPP instructions: the row_newbcast chains are gone?"
    assert not found, found[:5]
