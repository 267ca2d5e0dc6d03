"""CPU checks of the dropout restatement the GPU tests compare against
(tests/dropout_ref.py): the Philox known-answer vectors, unit masks == the
oracle's forward, and the restatement's own fp32-vs-fp64 error against the
project's tolerances (so the GPU comparison needs no waiver)."""
import numpy as np
import pytest
import torch

from oracle import pregan_train_oracle as TO
from preganplus_amd import weights as W
from tests import dropout_ref as DR


@pytest.mark.parametrize("ctr,key,want", [
    ([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
    ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0],
     [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]),
])
def test_philox_known_answers(ctr, key, want):
    got = DR.philox4x32_10(np.array(ctr, dtype=np.uint64), np.array(key, dtype=np.uint64))
    assert [int(v) for v in got] == want


def test_mask_geometry_and_indexing():
    """Site counts as the issue's table; an element's bit is word e & 3 of the
    block (e >> 2, site, n_lo, n_hi) under key (seed_lo, seed_hi)."""
    assert sum(DR.site_counts(16)) == 10560 and sum(DR.site_counts(8)) == 4320
    H, p, seed, step = 8, 0.5, (5 << 32) | 9, (1 << 32) + 5
    keep = DR.keep_masks(H, p, seed, step)
    off = np.concatenate([[0], np.cumsum(DR.site_counts(H))])
    for site, e in [(0, 0), (0, 191), (1, 7), (3, 1535), (8, 190)]:
        w = DR.philox4x32_10(np.array([e >> 2, site, 5, 1], dtype=np.uint64), np.array([9, 5], dtype=np.uint64))
        assert keep[off[site] + e] == (int(w[e & 3]) >= 1 << 31), (site, e)
    assert DR.keep_masks(H, 0.0, seed, step).all()
    assert DR.drop_threshold(0.5) == 1 << 31 and DR.drop_threshold(0.1) == int(float(np.float32(0.1)) * 2.0 ** 32)


@pytest.mark.parametrize("H", [8, 16])
def test_unit_masks_equal_the_oracle(H):
    w = W.synth_weights(H, seed=3)
    tw = TO.leaf_params(w["transformer"])
    x = torch.tensor(np.random.default_rng(1).uniform(0, 0.8, size=(2, 3, 3 * H)))
    got = DR.encode_drop_t(tw, x, DR.unit_masks(), 1.0)
    assert torch.equal(got, TO.encode_t(tw, x))
    # and all-ones keep bytes through split_masks
    one = DR.split_masks(np.ones(sum(DR.site_counts(H)), np.uint8), H)
    assert torch.equal(DR.encode_drop_t(tw, x[:1], one, 1.0), TO.encode_t(tw, x[:1]))


@pytest.mark.parametrize("H", [8, 16])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_restatement_fp32_is_well_inside_the_tolerances(H, p):
    """encode_drop_t in fp32 against fp64, the masks the kernel would draw:
    gradients within 0.1 of `1e-3 |want| + 1e-4 max|want|` (key-bias slice
    excluded), logits within 0.1 of `1e-4 |want| + 1e-5 max|want|`."""
    w = W.synth_weights(H, seed=3)
    scale = DR.keep_scale(p)
    worst_g = worst_l = 0.0
    for seed in range(6):
        x, y, mult, tgt = DR.spiky_case(H, seed)
        keep = DR.keep_masks(H, p, seed + 11, seed)
        a, lga, _ = DR.autograd_drop(w, x, y, mult, tgt, DR.split_masks(keep, H, torch.float64), scale, torch.float64)
        b, lgb, _ = DR.autograd_drop(w, x, y, mult, tgt, DR.split_masks(keep, H, torch.float32), scale, torch.float32)
        for k in a:
            if a[k].grad is None:
                continue
            want = DR.drop_key_bias(k, a[k].grad.numpy(), H)
            got = DR.drop_key_bias(k, b[k].grad.double().numpy(), H)
            worst_g = max(worst_g, DR.ratio_to_tolerance(got, want, 1e-3, 1e-4))
        worst_l = max(worst_l, DR.ratio_to_tolerance(lgb, lga, 1e-4, 1e-5))
    print(f"H={H} p={p}: worst gradient error / tolerance {worst_g:.4f}, logits {worst_l:.4f}")
    assert worst_g <= 0.1 and worst_l <= 0.1


def test_chosen_seeds_drop_counts_within_5_sigma():
    """The seeds the GPU mask test uses: |drops - 1056| <= 154 over one step at
    H = 16, p = 0.1 (sigma = sqrt(10560 * 0.1 * 0.9) = 30.8)."""
    for seed in DR.TEST_SEEDS:
        for base, step in DR.TEST_STEPS:
            drops = int((DR.keep_masks(16, 0.1, seed, base + step) == 0).sum())
            assert abs(drops - 1056) <= 154, (seed, base + step, drops)
