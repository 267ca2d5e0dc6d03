"""The offline FPE training entry points report the host counts they are
compiled for (csrc/pgp_fpetrain.hip: 16 and 50).  CPU: loads the library, makes
no GPU call."""
import numpy as np

from preganplus_amd import _native
from preganplus_amd import weights as W


def _param_len(n):
    return int(_native.lib().pgp_fpe_param_len(n))


def test_fpe_param_len_50_hosts():
    assert _param_len(50) == 93137
    assert _param_len(50) == sum(int(np.prod(s)) for s in W.fpe_shapes(50).values())


def test_fpe_param_len_16_hosts():
    assert _param_len(16) == 11401
    assert _param_len(16) == sum(int(np.prod(s)) for s in W.fpe_shapes(16).values())


def test_fpe_param_len_other_hosts():
    assert _param_len(32) == 0
