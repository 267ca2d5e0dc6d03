"""The PreGAN fleet forward, the host side: the header declares
pgp_fpe_forward1 / pgp_fpe_forward1_many, every argument error is returned before anything is
enqueued, and the Python front ends refuse what the kernel is not built for.  CPU: loads the
library, makes no GPU call."""
import ctypes
import os
import re

import numpy as np
import pytest

from preganplus_amd import _native
from preganplus_amd import weights as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -2
ENTRIES = ("pgp_fpe_forward1", "pgp_fpe_forward1_many")
VP = ctypes.c_void_p
H, K, M = 16, 3, 3
INPUTS = ("windows", "h0", "sched", "P_fpe", "P_master", "prototypes")
OUTPUTS = ("scores", "protos", "cls", "any_anom", "probs", "keep_orig", "final_target", "gen_target")


def test_header_declares_and_library_exports():
    with open(os.path.join(ROOT, "include", "preganplus.h")) as f:
        hdr = f.read()
    L = _native.lib()
    for name in ENTRIES:
        assert re.search(rf"\bint\s+{name}\s*\(", hdr), name
        assert hasattr(L, name) and name in _native.SIGNATURES, name
    assert [len(_native.SIGNATURES[n][1]) for n in ENTRIES] == [17, 20]
    assert "#define PGP_ABI_VERSION 1" in hdr and L.pgp_abi_version() == 1   # an addition only
    assert L.pgp_fpe_param_len(H) == 11401 and L.pgp_master_len(H) > L.pgp_master_offset(H, 2) > \
        L.pgp_master_offset(H, 1) > 0


class Host:
    """Sentinel-filled HOST arrays: a launch on them would fault."""

    def __init__(self):
        L = _native.lib()
        f = lambda shape, dt: np.full(shape, -7.25 if dt != np.int32 else -9, dtype=dt)
        f32, i32 = np.float32, np.int32
        self.a = {"windows": f((M, 3, 3 * H), f32), "h0": f((M, 3), f32), "sched": f((M, H, H), f32),
                  "P_fpe": f((M, int(L.pgp_fpe_param_len(H))), f32), "P_master": f((M, int(L.pgp_master_len(H))), f32),
                  "prototypes": f((M, 2 * K + 3), np.float64), "active": np.ones(M, dtype=i32),
                  "scores": f((M, H, 2), f32), "protos": f((M, H, 2), f32), "cls": f((M, H), i32),
                  "any_anom": f((M,), i32), "probs": f((M, 2), f32), "keep_orig": f((M,), i32),
                  "final_target": f((M, H), i32), "gen_target": f((M, H), i32)}
        self.before = {k: v.tobytes() for k, v in self.a.items()}

    def p(self, k, null=()):
        return None if k in null else self.a[k].ctypes.data_as(VP)

    def unchanged(self):
        return {k: v.tobytes() for k, v in self.a.items()} == self.before

    def one(self, L, H_=H, K_=K, null=()):
        return L.pgp_fpe_forward1(H_, K_, *[self.p(k, null) for k in INPUTS + OUTPUTS], None)

    def many(self, L, H_=H, K_=K, M_=M, stride=2 * K + 3, null=()):
        ins = [self.p(k, null) for k in ("active",) + INPUTS]
        return L.pgp_fpe_forward1_many(H_, K_, M_, *ins, stride, *[self.p(k, null) for k in OUTPUTS], None)


def test_argument_errors_enqueue_nothing():
    L = _native.lib()
    x = Host()
    # host counts: before everything else, whatever the rest is (8: the GAN kernels alone; 50: the FPE's alone)
    for h in (8, 50, 32, 0, -1, 64):
        assert x.one(L, H_=h) == ERR_UNSUPPORTED and x.many(L, H_=h) == ERR_UNSUPPORTED, h
        assert x.many(L, H_=h, M_=0) == ERR_UNSUPPORTED and x.many(L, H_=h, M_=-1) == ERR_UNSUPPORTED, h
    assert x.many(L, M_=-1) == ERR_ARG
    for k in (0, -1, 65, 1000):
        assert x.one(L, K_=k) == ERR_ARG and x.many(L, K_=k) == ERR_ARG, k
        assert x.many(L, K_=k, M_=0) == ERR_ARG, k
    for stride in (2 * K - 1, 0, -6):
        assert x.many(L, stride=stride) == ERR_ARG, stride
        assert x.many(L, stride=stride, M_=0) == ERR_ARG, stride
    for k in INPUTS + OUTPUTS:
        assert x.one(L, null=(k,)) == ERR_ARG, k
        assert x.many(L, null=(k,)) == ERR_ARG, k
    assert L.pgp_last_error()
    # nothing to do: PGP_OK, no pointer is looked at
    assert x.many(L, M_=0) == OK and x.many(L, M_=0, null=INPUTS + OUTPUTS + ("active",)) == OK
    assert x.many(L, M_=0, K_=1, stride=2) == OK and x.many(L, M_=0, K_=64, stride=128) == OK
    assert x.unchanged()


@pytest.mark.parametrize("hosts", [8, 50])
def test_python_front_ends_refuse_other_host_counts(hosts):
    from preganplus_amd.recovery import PreGANFleetRecovery, PreGANRecovery
    w = W.synth_fpe_weights(16, seed=11)
    with pytest.raises(ValueError, match="16"):
        PreGANFleetRecovery(hosts, [w, w], [{}, {}])
    with pytest.raises(ValueError, match="16"):
        PreGANFleetRecovery(hosts, [w], training=True)
    with pytest.raises(ValueError, match="16"):
        PreGANRecovery(hosts, "", training=True, weights=w, extra={}, master_forward=True)
    with pytest.raises(ValueError, match="16"):
        PreGANRecovery(hosts, "", weights=w, extra={}, master_forward=True)


def test_fleet_refuses_mismatched_lists():
    from preganplus_amd.recovery import PreGANFleetRecovery
    w = W.synth_fpe_weights(16, seed=11)
    with pytest.raises(ValueError, match="extras"):
        PreGANFleetRecovery(16, [w, w], [{}])
    with pytest.raises(ValueError, match="extras"):
        PreGANFleetRecovery(16, [w], [{}, {}, {}])
    with pytest.raises(ValueError, match="at least one"):
        PreGANFleetRecovery(16, [])
    w4 = dict(w, prototypes=np.zeros((4, 2)))
    with pytest.raises(ValueError, match="prototypes"):
        PreGANFleetRecovery(16, [w, w4])
