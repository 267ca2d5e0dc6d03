"""GPU parity at every compiled host count, on weights whose decisions depend
on the input (tests/branch_weights.py; its reference-side conditions are
asserted on the CPU in tests/test_branch_weights.py): the HIP path (through the
C-ABI) vs the fp64 oracle at the launch boundaries of K1 / K2 / K2b / K3, the
stage-split calls, K3's 16-wave fp32 form and the edge inputs at 8, 32 and 64
hosts.  Tolerance as everywhere (tests/parity_utils.py): continuous outputs
rtol 1e-4, decisions exact outside their derived fp32 band.  Marked gpu: runs
on the MI355X box only."""
import json

import numpy as np
import pytest
import torch

from oracle import pregan_oracle as O
from preganplus_amd import weights as W
from tests.branch_weights import N_WINDOWS, branch_weights
from tests.parity_utils import assert_parity
from tests.test_gpu_parity import _c2_torch, get_model, run

pytestmark = pytest.mark.gpu

# the edges of the grids: one block of 16 windows per K1 workgroup (and per
# wave everywhere); four waves, 64 windows, per K2 (H >= 32) and small-batch K3
# workgroup; 16 waves, 256 windows, per fp32 K2b workgroup
SWEEP_B = [1, 15, 16, 17, 63, 64, 65, 255, 256, 257, N_WINDOWS]


def _census_line(tag, st):
    kinds = {k: {f: v[f] for f in ("n", "in_band", "mismatch")} for k, v in st.items()
             if k in ("anomaly", "any", "class", "keep", "final", "gen")}
    print("CENSUS", tag, json.dumps({"windows": st["windows"], "windows_excluded": st["windows_excluded"], **kinds}))


@pytest.mark.parametrize("H", [8, 16, 32, 50, 64])
def test_launch_boundary_sweep(H):
    """The first B windows of branch_weights(H) for every B in SWEEP_B: within
    tolerance of the oracle, every decision as the oracle's outside its band,
    and every output bitwise the first B rows of the 293-window run (a window
    does not depend on its batch, on how many waves of its workgroup are busy,
    or on which workgroup it lands in).  Both values of ``any`` and ``keep``
    occur in the GPU's own outputs."""
    w, x, s, ref = branch_weights(H)
    m = get_model(H, w, f"branch{H}")
    full = run(m, x, s, latent=True)
    st = assert_parity(full, ref, w, s)
    _census_line(f"sweep H={H} B={N_WINDOWS}", st)
    for B in SWEEP_B[:-1]:
        got = run(m, x[:B], s[:B], latent=True)
        for k in full:
            assert got[k].shape[0] == B and np.array_equal(got[k], full[k][:B]), (k, B)
        r = {k: v[:B] for k, v in ref.items()}
        assert_parity(got, r, w, s[:B])
    assert 0 < full["any"].sum() < N_WINDOWS and 0 < full["keep"].sum() < N_WINDOWS
    # no more windows left out of the downstream kinds than the reference-side
    # cap on in-band anomaly flags allows
    assert st["windows"] == N_WINDOWS and st["windows_excluded"] <= 0.10 * N_WINDOWS, st


@pytest.mark.parametrize("H", [8, 32, 64])
def test_stage_split_equals_fused_call(H):
    """Stages 0-3 called one by one on a preallocated output, 65 windows (a
    second K2 / K3 workgroup at 32 and 64 hosts): bitwise the fused call."""
    w, x, s, _ = branch_weights(H)
    m = get_model(H, w, f"branch{H}")
    a = run(m, x[:65], s[:65], latent=True)
    b = run(m, x[:65], s[:65], latent=True, stage_split=True)
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert 0 < a["any"].sum() < 65


@pytest.mark.parametrize("H", [8, 32, 64])
def test_k3_fp32_16_wave_form(H):
    """K3's fp32 kernel in its 16-wave form (pgp_gan.hip: from 4,096 blocks of 16
    windows up; the only K3 at these host counts) on 65,557 windows: 4,098
    blocks, 257 workgroups, the last with two busy waves and a five-window
    tail.  First and last 64 windows against the oracle; windows at the start,
    middle and ragged tail bitwise the same when run alone (the 4-wave form: a
    wave owns its 16 windows in both, only the dealing of the weight DMA over
    the waves differs); probs / keep / any consistent over the whole launch."""
    from preganplus_amd.model import to_numpy
    B = 65557
    w = branch_weights(H)[0]
    m = get_model(H, w, f"branch{H}")
    x, s = _c2_torch(B, H, seed=4100 + H)
    g = torch.Generator(device="cuda").manual_seed(H)
    s[-256:] = torch.rand((256, H, H), generator=g, device="cuda")
    full = to_numpy(m.forward(x, s))
    torch.cuda.synchronize()
    for lo, hi in ((0, 64), (B // 2 - 7, B // 2 + 50), (B - 45, B)):
        part = to_numpy(m.forward(x[lo:hi].contiguous(), s[lo:hi].contiguous()))
        torch.cuda.synchronize()
        for k in part:
            assert np.array_equal(full[k][lo:hi], part[k]), (k, lo, hi)
    idx = np.r_[0:64, B - 64:B]
    xs = x[idx].cpu().numpy().astype(np.float64)
    ss = s[idx].cpu().numpy().astype(np.float64)
    del x, s, m
    torch.cuda.empty_cache()
    assert np.isfinite(full["logits"]).all() and np.isfinite(full["probs"]).all()
    np.testing.assert_allclose(full["probs"].sum(axis=1), 1.0, rtol=0, atol=2e-6)
    assert np.array_equal(full["keep"], full["probs"][:, 0] > full["probs"][:, 1])
    anom = full["logits"][..., 1] > full["logits"][..., 0]
    assert np.array_equal(full["any"], anom.any(axis=1))
    assert np.array_equal(full["cls"] < 0, ~anom)
    assert 0 < full["any"].sum() < B and 0 < full["keep"].sum() < B
    ref = O.forward(w, xs, ss)
    ref["sched32"] = ss.astype(np.float32)
    st = assert_parity({k: v[idx] for k, v in full.items()}, ref, w, ss)
    _census_line(f"k3-16wave H={H} B={B} (first and last 64)", st)


@pytest.mark.parametrize("H", [8, 32, 64])
def test_edge_inputs(H):
    """test_edge_inputs_h16's windows and schedules at width 3 H, on the plain
    seeded weights: constant / zero / extreme windows; all-zero and tied
    schedules."""
    w = W.synth_weights(H, seed=7)
    x = np.zeros((8, 3, 3 * H))
    x[1] = 1.0                      # constant rows
    x[2] = 50.0                     # far outside the training range
    x[3, :, ::3] = 1.0              # cpu saturated everywhere
    x[4] = np.linspace(0, 2, 9 * H).reshape(3, 3 * H)
    x[5, 2] = 1.3
    x[6] = 1e-6
    x[7, 0] = 0.9
    s = np.zeros((8, H, H))         # all-zero rows -> argmax 0
    s[1, :, 3] = s[1, :, 5] = 1.0   # ties -> first index
    s[2] = np.eye(H)
    s[3] = 0.5
    s[4:] = np.eye(H)[::-1]
    ref = O.forward(w, x, s)
    ref["sched32"] = s.astype(np.float32)
    assert all(np.isfinite(ref[k]).all() for k in ("logits", "protos", "probs", "new_sched"))
    m = get_model(H, w, f"syn{H}")
    got = run(m, x, s)
    st = assert_parity(got, ref, w, s)
    _census_line(f"edge H={H}", st)
    assert got["final_target"][0].tolist() == [0] * H
    assert got["final_target"][1].tolist() == [3] * H
    for k in ("logits", "protos", "probs"):
        assert np.isfinite(got[k]).all(), k
