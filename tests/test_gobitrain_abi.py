"""The C-ABI of the surrogate's training (include/preganplus.h,
csrc/pgp_gobitrain.hip through pgp_capi.hip): declared, exported, and its
argument checks, which run on the host before any launch.  CPU: loads the
library, makes no GPU call."""
import os
import re

import pytest

from preganplus_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -2
_lib = _native.lib


def _steps(L, H=16, N=4, n=0, step0=0, lr=1e-4, wd=1e-5, b1=0.9, b2=0.999, eps=1e-8, ptr=None):
    return L.pgp_gobi_train_steps(H, N, n, ptr, ptr, ptr, ptr, ptr, ptr, step0, lr, wd, b1, b2, eps, ptr, None)


def test_header_declares_and_library_exports():
    with open(os.path.join(ROOT, "include", "preganplus.h")) as f:
        hdr = f.read()
    L = _native.lib()
    for name in ("pgp_gobi_train_steps", "pgp_gobi_train_eval"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert hasattr(L, name), name
    assert "#define PGP_ABI_VERSION 1" in hdr and L.pgp_abi_version() == 1   # additions only


@pytest.mark.parametrize("H", [8, 50, 0])
def test_other_host_counts_are_unsupported(H):
    L = _lib()
    assert _steps(L, H=H) == ERR_UNSUPPORTED
    assert L.pgp_gobi_train_eval(H, 4, 0, None, None, None, None, None, None) == ERR_UNSUPPORTED


@pytest.mark.parametrize("kw", [dict(n=-1), dict(N=-1), dict(step0=-1), dict(lr=0.0), dict(lr=-1e-4),
                                dict(lr=float("nan")), dict(wd=-1e-5), dict(b1=1.0), dict(b1=-0.1), dict(b2=1.0),
                                dict(b2=1.5), dict(eps=-1e-8), dict(n=3)])
def test_bad_arguments(kw):
    """(n = 3 with NULL pointers: a NULL argument, not a launch.)"""
    assert _steps(_lib(), **kw) == ERR_ARG


def test_empty_call_is_ok_and_launches_nothing():
    L = _lib()
    assert _steps(L, n=0) == OK   # NULL pointers and no device: nothing may be touched
    assert L.pgp_gobi_train_eval(16, 4, 0, None, None, None, None, None, None) == OK
    assert L.pgp_gobi_train_eval(16, 4, -1, None, None, None, None, None, None) == ERR_ARG
    assert L.pgp_gobi_train_eval(16, 4, 2, None, None, None, None, None, None) == ERR_ARG
