"""Conditions on the reference side of tests/test_gpu_parity_hosts.py (CPU).

The GPU tests that use ``branch_weights`` compare decisions exactly outside
their derived fp32 band and leave out windows whose anomaly flags differ in
band.  These conditions, on the fp64 oracle alone, are what keeps a kernel
fault from hiding behind those exclusions: both gates really open and close,
several classes occur, and few decisions sit in band."""
import numpy as np
import pytest

from oracle import pregan_oracle as O
from preganplus_amd import weights as W
from tests import decision_bounds as DB
from tests.branch_weights import N_WINDOWS, branch_weights, inputs

HOSTS = [8, 16, 32, 50, 64]
IN_BAND_CAP = {"anomaly": 0.10, "class": 0.02, "keep": 0.02, "gen": 0.02}


@pytest.mark.parametrize("H", HOSTS)
def test_branch_weights_reference_conditions(H):
    w, x, s, ref = branch_weights(H)
    assert x.shape == (N_WINDOWS, 3, 3 * H) and s.shape == (N_WINDOWS, H, H)
    # inputs and the two shifted biases are fp32-representable
    for a in (x, s, w["transformer"]["anomaly_decoder.0.bias"], w["disc"]["probs.2.bias"]):
        assert np.array_equal(a, np.asarray(a, np.float32).astype(np.float64))
    # every (any, keep) cell is populated
    for a in (False, True):
        for k in (False, True):
            cell = int(((ref["any"] == a) & (ref["keep"] == k)).sum())
            assert cell >= 40, (a, k, cell)
    assert len(np.unique(ref["cls"][ref["cls"] >= 0])) >= 2
    # the smallest batches of the launch-boundary sweep see both branches too
    assert 0 < ref["any"][:16].sum() < 16
    # few decisions within what fp32 can move: the oracle against itself in fp32
    got = O.forward(w, x, s, dtype=np.float32)
    st = DB.compare(got, ref, w, s)
    assert not DB.violations(st), st
    for kind, cap in IN_BAND_CAP.items():
        assert st[kind]["n"] > 0
        assert st[kind]["in_band"] <= cap * st[kind]["n"], (kind, st[kind])


@pytest.mark.parametrize("H", HOSTS)
def test_plain_synth_weights_flags_do_not_depend_on_the_input(H):
    """Why the shifts are needed: on the unshifted seeded weights every window
    flags the same hosts (and at least one), so ``any`` is constant."""
    x, s = inputs(H)
    r = O.forward(W.synth_weights(H, 7), x, s)
    assert (r["anom"] == r["anom"][0]).all()
    assert r["any"].all()


def test_branch_weights_are_cached_and_leave_synth_weights_alone():
    a = branch_weights(8)
    assert branch_weights(8) is a
    plain = W.synth_weights(8, 7)
    assert not np.array_equal(a[0]["transformer"]["anomaly_decoder.0.bias"],
                              plain["transformer"]["anomaly_decoder.0.bias"])
    assert np.array_equal(a[0]["gen"]["delta.0.weight"], plain["gen"]["delta.0.weight"])
