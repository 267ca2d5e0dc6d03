"""K2b's split-bf16 form at H = 50 contracts the latent in dense 32-k blocks:
the (host, step) chunks of two hosts form one stream of 6 x 13 = 78 k-steps cut
into 10 blocks of 8 with 2 zero slots (pgp_decoder.hip DecB), so a block takes its k-steps from
one or two neighbouring chunks and the weight planes are laid out in the same
order.  These tests pin the k-order (every latent element reaches the row it
belongs to, exactly), ragged and tile-inactive batches, batch independence,
and the bookkeeping of the built kernel.

A repack of the master re-derives the plane image through the same launch as a
weight load; tests/test_gpu_repack.py::test_device_repack_equals_host_pack[50]
pins that for this decoder (the split form is H = 50's default: a stale image
would give other logits than the freshly loaded model's)."""
import os
import sys

import numpy as np
import pytest

from oracle import pregan_oracle as O
from preganplus_amd import roofline as R
from preganplus_amd import weights as W
from tests.parity_utils import assert_parity

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "preganplus_amd", "_lib", "libpreganplus.so")
H = 50

# probe positions: hosts = first / second of a body, the next body, the last
# body; steps = first / last; channels c = 4 s + g: k-steps 0, 7 | 8, 11, the
# loose k-step 12 (c = 48, 49).  With the chunk index 3 (h % 2) + w inside a
# body the stream positions 13 chunk + s touch every block boundary the probed
# chunks have, the first position (behind the zero slots in front of the stream)
# and the last, 77
PROBE_H, PROBE_W, PROBE_C = (0, 1, 2, 49), (0, 2), (0, 31, 32, 47, 48, 49)


def _inputs(n, seed):
    from tests.test_gpu_parity import c2
    return c2(np.random.Generator(np.random.PCG64(seed)), n, H, dense=min(5, n))


@pytest.mark.gpu
def test_k_order_probe():
    """Decoder weights zero except one 1.0 per logit row, at column (h, w, c) of
    the latent; the last layer's norm2 is the identity (gamma 1, beta 0: the
    packer folds it into the decoder).  Then that logit is the latent element
    itself, bit for bit: 1.0 splits as (1, 0, 0) and x0 + x1 + x2 reassembles x
    exactly in mfma_bf6's order (x2 + x1 is the exact residual x - x0); every
    other product is an exact zero.  A k-step that met another k-step's plane,
    or a zero-filled slot, gives 0 or another element.  All 48 positions sit on
    distinct logit rows of one model; the fp32 form passes the same probe."""
    from preganplus_amd.model import DecisionModel
    from tests.test_gpu_parity import run
    w = W.synth_weights(H, seed=11)
    t = w["transformer"]
    t["transformer_encoder.layers.1.norm2.weight"][:] = 1.0
    t["transformer_encoder.layers.1.norm2.bias"][:] = 0.0
    for k in ("anomaly_decoder.0", "prototype_decoder.0"):
        t[k + ".weight"][:] = 0.0
        t[k + ".bias"][:] = 0.0
    pos = [(h, s, c) for h in PROBE_H for s in PROBE_W for c in PROBE_C]
    assert len(pos) <= 2 * H
    cols = [h * 3 * H + s * H + c for h, s, c in pos]
    for n, col in enumerate(cols):
        t["anomaly_decoder.0.weight"][n, col] = 1.0
    x, s = _inputs(16, 500)
    m = DecisionModel(H, w)
    for split in (True, False):
        m.decoder_split(split)
        got = run(m, x, s, latent=True)
        lat = got["latent"][:, cols]
        assert np.abs(lat).min() > 0        # a probe that reads 0 would prove nothing
        rows = got["logits"].reshape(16, 2 * H)
        bad = [(pos[n], float(rows[b, n]), float(lat[b, n])) for b, n in
               zip(*np.nonzero(rows[:, :len(pos)].view(np.uint32) != lat.view(np.uint32)))]
        assert not bad, (split, bad[:8])
        assert not rows[:, len(pos):].any()  # rows without a tap stay exactly 0
        assert np.array_equal(got["protos"], np.full_like(got["protos"], 0.5))
    m.decoder_split(True)


@pytest.fixture(scope="module")
def ragged():
    """261 windows and their fp64 oracle, computed once; the smaller batches are prefixes."""
    from preganplus_amd.model import DecisionModel
    w = W.synth_weights(H, seed=12)
    x, s = _inputs(261, 501)
    ref = O.forward(w, x, s)
    return w, x, s, ref, DecisionModel(H, w)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [5, 37, 261])
def test_ragged_and_tile_inactive_batches(ragged, B):
    """B = 5: wave 0's second window tile is past the batch (it then reads tile
    0's latent and stores nothing); B = 37: a ragged third tile; B = 261: a
    second workgroup with one tile of 5 windows.  Against the fp64 oracle."""
    from tests.test_gpu_parity import run
    w, x, s, ref, m = ragged
    r = {k: (v[:B] if isinstance(v, np.ndarray) and v.shape[:1] == (261,) else v) for k, v in ref.items()}
    r["sched32"] = s[:B].astype(np.float32)
    got = run(m, x[:B], s[:B], latent=True)
    assert_parity(got, r, w, s[:B])


@pytest.mark.gpu
def test_batch_independence():
    """The first 37 windows give the same bits alone and inside 517 windows
    (other workgroup count, other tiles beside them in the wave)."""
    from preganplus_amd.model import DecisionModel
    from tests.test_gpu_parity import run
    w = W.synth_weights(H, seed=13)
    x, s = _inputs(517, 502)
    m = DecisionModel(H, w)
    big, small = run(m, x, s), run(m, x[:37], s[:37])
    for k in ("logits", "protos", "cls"):
        assert np.array_equal(big[k][:37].view(np.uint32), small[k].view(np.uint32)), k


@pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"),
                    reason="built library / llvm-objdump absent")
def test_built_kernel_bookkeeping():
    """The bf16 MFMAs of decoder_split_kernel<50, 2> as built (one body of the
    `#pragma unroll 1` loop, a wave's 2 window tiles) are what
    roofline.decoder_split_flops_per_window counts: 25 bodies x 10 blocks x 13
    tiles x 6 per window tile; and the kernel holds its registers: no spilled
    VGPR or SGPR and no scratch in the built code object's metadata."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_count
    per_body = isa_count.decoder_split_count(H, 2)
    bodies, tw = 25, 2
    per_tile = per_body * bodies // tw
    assert per_tile == 25 * 10 * 13 * 6
    assert R.decoder_split_flops_per_window(H) == per_tile * 16 * 16 * 32 * 2 // 16
    assert R.decoder_split_flops_per_window(32) == 96 * 8 * 6 * 16 * 16 * 32 * 2 // 16  # H = 32: one block per chunk, 8 tiles
    res = [v for k, v in isa_count.kernel_resources("decoder_split_kernel").items() if f"ILi{H}ELi2E" in k]
    assert len(res) == 1, res
    assert res[0]["vgpr_spill_count"] == 0 and res[0]["sgpr_spill_count"] == 0, res
    assert res[0]["private_segment_fixed_size"] == 0, res
    assert res[0]["vgpr_count"] <= 256, res  # two waves per SIMD
