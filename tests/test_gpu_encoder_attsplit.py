"""K2's attention-split form (pgp_encoder_split form 1, encoder_asplit_kernel<50>:
layer 1's q|k, v and out_proj on split-bf16 planes of which the last ones are
read from global memory) against the fp64 oracle, the fp32 form (0) and the
split feed-forward form (2).  H = 50 only; marked gpu."""
import numpy as np
import pytest
import torch

from oracle import pregan_oracle as O
from preganplus_amd import weights as W
from tests.parity_utils import RTOL, assert_parity
from tests.test_gpu_parity import c2, run

pytestmark = pytest.mark.gpu

H = 50
DECISIONS = ("cls", "any", "keep", "final_target", "gen_target")
_cache = {}


def model(seed=4):
    from preganplus_amd.model import DecisionModel
    if ("m", seed) not in _cache:
        _cache[("m", seed)] = (DecisionModel(H, W.synth_weights(H, seed=seed)), W.synth_weights(H, seed=seed))
    return _cache[("m", seed)]


def run_form(m, form, x, s, latent=True):
    m.encoder_split(form)
    try:
        return run(m, x, s, latent=latent)
    finally:
        m.encoder_split(1)


def big():
    """B = 1,333: 84 blocks x 50 hosts = 4,200 units, about two per wave with
    uneven ranges on a 256-CU device (one 8-wave workgroup per CU)."""
    if "big" not in _cache:
        rng = np.random.Generator(np.random.PCG64(911))
        x, s = c2(rng, 1333, H, dense=9)
        m, w = model()
        _cache["big"] = (x, s, {f: run_form(m, f, x, s) for f in (0, 1, 2)})
    return _cache["big"]


def test_three_forms_vs_oracle_ragged_batch():
    rng = np.random.Generator(np.random.PCG64(350))
    m, w = model()
    x, s = c2(rng, 517, H, dense=9)
    ref = O.forward(w, x, s)
    ref["sched32"] = s.astype(np.float32)
    out = {f: run_form(m, f, x, s) for f in (0, 1, 2)}
    for f in (0, 1, 2):
        assert_parity(out[f], ref, w, s)
    for k in ("latent", "logits", "protos"):
        n = ref[k].shape[0]
        e1 = np.abs(out[1][k][:n].astype(np.float64) - ref[k]).max()
        e0 = np.abs(out[0][k][:n].astype(np.float64) - ref[k]).max()
        print(f"{k}: worst error form 1 {e1:.3e}, form 0 {e0:.3e}")
        assert e1 <= 2 * e0 + 1e-7, (k, e1, e0)
    for k in DECISIONS:
        assert np.array_equal(out[1][k], out[0][k]) and np.array_equal(out[1][k], out[2][k]), k
    # the forms really ran
    assert not np.array_equal(out[1]["latent"], out[2]["latent"])
    assert not np.array_equal(out[1]["latent"], out[0]["latent"])


def test_several_units_per_wave():
    x, s, out = big()
    m, w = model()
    for k in DECISIONS:
        assert np.array_equal(out[1][k], out[0][k]), k
    np.testing.assert_allclose(out[1]["latent"], out[0]["latent"], rtol=RTOL, atol=1e-4)
    ref = O.forward(w, x[:256], s[:256])
    ref["sched32"] = s[:256].astype(np.float32)
    got = {k: (v[:256] if v is not None else None) for k, v in out[1].items()}
    assert_parity(got, ref, w, s[:256])


@pytest.mark.parametrize("form", [1, 2])
def test_latent_independent_of_the_batch(form):
    """A window's latent does not depend on the launch it arrives in (its block,
    its lane, its unit's place in a wave's range): bit for bit."""
    x, s, out = big()
    m, _ = model()
    for lo, hi in ((0, 16), (656, 693), (1317, 1333)):
        alone = run_form(m, form, x[lo:hi], s[lo:hi])
        assert np.array_equal(alone["latent"], out[form]["latent"][lo:hi]), (form, lo, hi)


def test_smallest_batch():
    rng = np.random.Generator(np.random.PCG64(5))
    m, w = model()
    x, s = c2(rng, 5, H)
    ref = O.forward(w, x, s)
    ref["sched32"] = s.astype(np.float32)
    assert_parity(run_form(m, 1, x, s), ref, w, s)


def test_weight_update_rederives_the_image():
    """A device repack and a host load of perturbed master weights give the same
    bits under form 1 (its image is re-derived by both), other bits than the
    unperturbed model, and the form switch is stateless."""
    from preganplus_amd import train as TR
    from preganplus_amd.model import DecisionModel
    rng = np.random.default_rng(50)
    w = W.synth_weights(H, seed=H)
    tr = TR.Trainer(H, w, max_batch=1)
    tr.P.add_(torch.randn_like(tr.P) * 1e-2)
    protos = rng.uniform(0, 1, (H, 2))
    host, dev, base = DecisionModel(H, w), DecisionModel(H, w), DecisionModel(H, w)
    host.load_master(tr.P, protos)
    dev.repack_master(tr.P, torch.tensor(protos, dtype=torch.float64, device=tr.device), protos)
    B = 48
    x = rng.uniform(0, 1, (B, 3, 3 * H))
    s = rng.uniform(0, 1, (B, H, H))
    a, b, c = (run_form(mm, 1, x, s) for mm in (host, dev, base))
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert not np.array_equal(a["latent"], c["latent"])
    assert not np.array_equal(a["logits"], c["logits"])
    two = run_form(dev, 2, x, s)
    again = run_form(dev, 1, x, s)
    assert not np.array_equal(two["latent"], b["latent"])
    for k in b:
        assert np.array_equal(again[k], b[k]), k
