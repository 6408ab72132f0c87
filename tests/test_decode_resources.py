"""The frame decode's kernels (ws_decode_gpu.hip) exist in the built gfx950 library and neither
spill registers nor use a private segment (CPU test, no GPU): the gather's per-lane compose path
sits beside its streaming path in one kernel, and a spill there would put scratch traffic into
every chunk (tests/test_kernel_resources.py tells what that cost the frame assembly)."""

import os

import pytest

from tests.test_kernel_resources import LIB, READELF, kernel_resources

DECODE_KERNELS = ["decode_offsets(", "decode_gather("]


@pytest.fixture(scope="module")
def resources():
    if not os.path.exists(LIB):
        pytest.skip("libnetc_ws_gpu.so not built (make)")
    if not os.path.exists(READELF):
        pytest.skip("llvm-readelf not found")
    return kernel_resources()


@pytest.mark.parametrize("kernel", DECODE_KERNELS)
def test_decode_kernel_exists_and_does_not_spill(resources, kernel):
    found = {k: v for k, v in resources.items() if "netc_gpu::" in k and kernel in k}
    assert len(found) == 1, f"expected one kernel {kernel}*, found {sorted(found)}"
    for k, (vgprs, spills, scratch) in found.items():
        assert spills == 0 and scratch == 0, f"{k}: {vgprs} VGPRs, {spills} spilled, {scratch} B scratch per lane"
        assert vgprs <= 128, f"{k}: {vgprs} VGPRs leave fewer than 4 wavefronts per SIMD"
