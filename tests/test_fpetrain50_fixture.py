"""Pin the oracle's fp64 restatement of PreGAN's offline FPE training at 50
hosts (oracle.pregan_train_oracle: fpe_t, custom_loss, fpe_backprop, AdamW)
against the reference's own modules (tests/golden/make_golden_fpetrain50.py:
the reference FPE_16 class at n_hosts = 50), before any GPU test relies on it.
Tolerances: those of the 16-host test
(test_train_oracle_golden.test_fpe_offline_training_matches_reference) and, for
the gradients, of test_tuning_step_matches_reference."""
import numpy as np
import pytest
import torch

from oracle import pregan_oracle as O
from oracle import pregan_train_oracle as TO
from tests import fpetrain50_common as C


def test_fpe50_fixture_data():
    """The windows and labels are load_dataset's of the recorded series; the
    label mix the GPU tests rely on."""
    from preganplus_amd import train as TR
    z, _, zs, init, _ = C.fixture()
    wins, anom, cls = TR.load_dataset(z["series"])
    np.testing.assert_allclose(wins, z["wins"], rtol=0, atol=1e-15)
    assert np.array_equal(anom, z["anom"]) and np.array_equal(cls, z["cls"])
    npos = z["anom"].sum(1)
    assert (npos == 0).sum() >= 2 and (npos > 0).sum() >= 15
    assert set(np.unique(z["cls"][z["anom"] > 0])) == {0, 1, 2}
    many, idle, other = (int(i) for i in zs["index"])
    assert npos[idle] == 0 and npos[many] == npos.max() and 0 < npos[other] < npos[many]
    assert sum(int(np.prod(v.shape)) for v in init.values()) == 93137


@pytest.mark.parametrize("j", [0, 1, 2])
def test_fpe50_step_gradients_match_reference(j):
    """One step from the initial weights (many positives / idle / other):
    losses, the gradient of every parameter, the state after the step."""
    z, _, zs, init, protos = C.fixture()
    i = int(zs["index"][j])
    fw = TO.leaf_params(init, skip=())
    st = TO.TuneState(protos, float(zs["factor"]))
    st.num_zero, st.num_ones = int(zs["num_zero"]), int(zs["num_ones"])
    probs, pr = TO.fpe_t(fw, torch.tensor(z["wins"][i:i + 1]), torch.tensor(zs[f"s{j}/h0"][None]))
    aloss, tloss = TO.custom_loss(probs[0], pr[0], z["anom"][i], z["cls"][i], st)
    (aloss + tloss).backward()
    np.testing.assert_allclose([float(aloss), float(tloss)], zs[f"s{j}/loss"], rtol=1e-10, atol=1e-12)
    for k, q in fw.items():
        assert (q.grad is not None) == bool(zs[f"s{j}/has_grad/{k}"]), k
        got = np.zeros(q.shape) if q.grad is None else q.grad.numpy()
        C.recorded(zs, f"s{j}/g/{k}", got, C.close(1e-8, 1e-12), sum_rel=1e-8, key=k)
    np.testing.assert_allclose(np.stack([p.numpy() for p in st.protos]), zs[f"s{j}/prototypes"], rtol=1e-12)
    assert st.factor == pytest.approx(float(zs[f"s{j}/state"][0]), rel=1e-14)
    assert (st.num_zero, st.num_ones) == tuple(zs[f"s{j}/state"][1:])


def test_fpe50_offline_training_matches_reference():
    """Two epochs over the 24 windows with the recorded GRU states: loss,
    factor, counters, parameters, AdamW moments and step counts, prototypes
    after each epoch, and accuracy()'s scores from the same forwards."""
    from preganplus_amd import train as TR
    z, zo, _, init, protos = C.fixture()
    fw = TO.leaf_params(init, skip=())
    opt = TO.AdamW(fw, 1e-4)
    st = TO.TuneState(protos, 0.2)
    wins, anom, cls = z["wins"], z["anom"], z["cls"]
    for ep in range(2):
        losses = TO.fpe_backprop(fw, opt, st, wins, z[f"ep{ep}/h0_backprop"], anom, cls)
        loss = np.mean([a for a, _ in losses]) + np.mean([t for _, t in losses])
        assert loss == pytest.approx(float(z[f"ep{ep}/loss"]), rel=1e-12)
        assert st.factor + O.PROTO_UPDATE_MIN == pytest.approx(float(z[f"ep{ep}/factor"]), rel=1e-14)
        assert (st.num_zero, st.num_ones) == (z[f"ep{ep}/num_zero"], z[f"ep{ep}/num_ones"])
        for k, q in fw.items():
            C.recorded(z, f"ep{ep}/p/{k}", q.detach().numpy(), C.close(1e-10, 1e-13), sum_rel=1e-10, key=k)
            C.recorded(zo, f"ep{ep}/m/{k}", opt.m[k].numpy(), C.close(1e-9, 1e-14), sum_rel=1e-9, key=k)
            assert opt.step[k] == float(z[f"ep{ep}/step/{k}"])
        np.testing.assert_allclose(np.stack([p.numpy() for p in st.protos]), z[f"ep{ep}/prototypes"], rtol=1e-12)
        with torch.no_grad():
            probs, pr = TO.fpe_t(fw, torch.tensor(wins), torch.tensor(z[f"ep{ep}/h0_accuracy"]))
        asc, csc = TR.accuracy_scores(probs.numpy(), pr.numpy(), anom, cls, np.stack([p.numpy() for p in st.protos]))
        assert asc == pytest.approx(float(z[f"ep{ep}/ascore"]), rel=1e-12)
        assert csc == pytest.approx(float(z[f"ep{ep}/cscore"]), rel=1e-12)
