"""What hipcc makes of csrc/conv_wino.hip, from the kernel metadata alone (no GPU): the file is compiled to gfx950 assembly with the
build recipe's flags in a temporary directory (tools/wino_isa_counts.py does the same for its instruction counts), once as the product
library compiles it and once as the dev library does (-DHPS_DEV_BUILD; the file is part of both).  Either way it must hold exactly the
two conv_wino_kernel instantiations that ship -- the 16 x 16-block form and its quad sibling; the earlier forms live in
csrc/conv_wino_dev.hip -- and each of them must

  * use no scratch (.private_segment_fixed_size = 0): a spilled register is reloaded behind s_waitcnt vmcnt(0), which also drains the
    LDS-DMA pieces in flight (see pk_off in the kernel);
  * fit 256 registers (.vgpr_count <= 256): the kernel runs two waves per SIMD, and a SIMD has 512.
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import wino_isa_counts as W  # noqa: E402


def _metadata(dev):
    asm = W.compile_asm(dev=dev, source="conv_wino.hip")
    meta = {k: v for k, v in W.metadata(asm).items() if "conv_wino" in k and "kernel" in k}
    assert len(meta) == 2 and all("conv_wino_kernel" in k for k in meta), sorted(meta)     # no dev-only kernel in this file
    assert sorted(W.kernels(asm)) == sorted(meta)             # ... and the tool's instruction counts see the same two
    return meta


@pytest.fixture(scope="module")
def product_metadata():
    return _metadata(dev=False)


def test_wino_kernels_use_no_scratch(product_metadata):
    for name, m in product_metadata.items():
        assert m["private_segment_fixed_size"] == 0, (name, m)
        assert m.get("vgpr_spill_count", 0) == 0, (name, m)


def test_wino_kernels_fit_two_waves_per_simd(product_metadata):
    for name, m in product_metadata.items():
        assert m["vgpr_count"] <= 256, (name, m)


def test_wino_kernels_the_same_in_the_dev_library(product_metadata):
    dev = _metadata(dev=True)
    assert dev == product_metadata                            # same names, registers and (no) scratch: -DHPS_DEV_BUILD adds only the K-slice override
    for name, m in dev.items():
        assert m["private_segment_fixed_size"] == 0 and m.get("vgpr_spill_count", 0) == 0 and m["vgpr_count"] <= 256, (name, m)
