"""The attention-split form of K2 (encoder_asplit_kernel<50>, pgp_encoder.hip
EncA) as BUILT: its MFMA counts are the ones roofline.py reports work with, they
relate to the split feed-forward form's as the change says (layer 1's 468 fp32
attention MFMAs gone, 12 tiles x 2 blocks x 6 products x 3 steps bf16 ones in
their place), and its LDS image fits the CU.  CPU-only (disassembly of the built
library, the library's own geometry export)."""
import ctypes
import os
import sys

import pytest

from preganplus_amd import roofline as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "preganplus_amd", "_lib", "libpreganplus.so")

needs_lib = pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"),
                               reason="built library / llvm-objdump absent")


@needs_lib
def test_attention_split_mfma_counts_match_built_library():
    import isa_count
    got = isa_count.encoder_asplit_counts(tuple(R.ENC_ASPLIT_MFMA_PER_HOST))
    old = isa_count.encoder_split_counts(tuple(R.ENC_ASPLIT_MFMA_PER_HOST))
    for H, want in R.ENC_ASPLIT_MFMA_PER_HOST.items():
        assert got[H][:2] == want, (H, got[H], want)
        assert got[H][0] == old[H][0] - 468
        assert got[H][1] == old[H][1] + 12 * 2 * 6 * 3
    # bench.py's executed-work fields describe the default form
    f32, bf = R.encoder_split_executed_flops_per_window(50)
    assert (f32, bf) == (48 * 2048 * 50 / 16, 936 * 16 * 16 * 32 * 2 * 50 / 16)
    assert R.ENC_SPLIT_MFMA_PER_HOST[50] == (516, 504)


@needs_lib
def test_attention_split_lds_geometry():
    """Layer 1's attention is 24 plane triples (q|k 12, v 6, out_proj 6); the
    LDS-resident ones with the feed-forward planes, the tables and the staging
    slots stay within the CU's 160 KiB, and the kernel's resource report agrees
    with the constants."""
    from preganplus_amd import _native
    L = _native.lib()
    c, lds, res, strm = (ctypes.c_int() for _ in range(4))
    assert L.pgp_encoder_form_info(50, ctypes.byref(c), ctypes.byref(lds), ctypes.byref(res), ctypes.byref(strm)) == 0
    assert c.value == 1
    assert res.value + strm.value == 24 and res.value in (16, 17)
    assert 0 < lds.value <= 163840
    # 42 + 42 feed-forward groups and 3 per resident triple, 1 KiB each, at least
    assert lds.value >= (84 + 3 * res.value) * 1024
    for H in (8, 16, 32, 64):
        assert L.pgp_encoder_form_info(H, ctypes.byref(c), ctypes.byref(lds), ctypes.byref(res), ctypes.byref(strm)) == 0
        assert (c.value, lds.value, res.value, strm.value) == (0, 0, 0, 0)


def _kernel_metadata(needle):
    """The code object metadata (llvm-readelf --notes) of the built library's
    gfx950 kernel whose name contains `needle`, as {field: text}."""
    import glob
    import re
    import shutil
    import subprocess
    import tempfile
    bindir = "/opt/rocm/lib/llvm/bin"
    with tempfile.TemporaryDirectory() as td:
        shutil.copy(LIB, os.path.join(td, "lib.so"))
        subprocess.run([f"{bindir}/llvm-objdump", "--offloading", "lib.so"], cwd=td, check=True, capture_output=True)
        for co in sorted(glob.glob(os.path.join(td, "lib.so.*gfx950"))):
            notes = subprocess.run([f"{bindir}/llvm-readelf", "--notes", co], check=True, capture_output=True,
                                   text=True).stdout
            for item in re.split(r"\n  - (?=\.)", notes):
                f = dict(re.findall(r"^\s*(\.\w+):\s*(\S+)\s*$", item, re.M))
                if needle in f.get(".name", ""):
                    return f
    return None


@needs_lib
def test_attention_split_kernel_has_no_spills():
    """0 spilled VGPRs, no scratch, 512 threads per block launchable (2 waves per
    SIMD within the 512 registers of a SIMD lane) and the LDS within the CU's,
    from the code object's metadata."""
    f = _kernel_metadata("encoder_asplit_kernelILi50")
    assert f is not None
    assert int(f[".vgpr_spill_count"]) == 0 and int(f[".sgpr_spill_count"]) == 0
    assert int(f[".private_segment_fixed_size"]) == 0
    assert int(f[".vgpr_count"]) <= 256          # arch + accumulation registers of one wave
    assert int(f[".max_flat_workgroup_size"]) >= 512
    assert int(f[".group_segment_fixed_size"]) <= 163840
