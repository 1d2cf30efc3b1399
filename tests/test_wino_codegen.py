"""What hipcc makes of csrc/conv_wino.hip, from the kernel metadata alone (no GPU): the file is compiled to gfx950 assembly with the
build recipe's flags in a temporary directory (tools/wino_isa_counts.py does the same for its instruction counts), and every
conv_wino_kernel instantiation of the product library must

  * use no scratch (.private_segment_fixed_size = 0): a spilled register is reloaded behind s_waitcnt vmcnt(0), which also drains the
    LDS-DMA pieces in flight (see pk_off in the kernel);
  * fit 256 registers (.vgpr_count <= 256): the eight-wave forms run two waves per SIMD, and a SIMD has 512.
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import wino_isa_counts as W  # noqa: E402


@pytest.fixture(scope="module")
def product_metadata():
    meta = {k: v for k, v in W.metadata(W.compile_asm(dev=False)).items() if "conv_wino_kernel" in k}
    assert len(meta) >= 2, sorted(meta)                       # the 16 x 16-block form and its quad sibling
    return meta


def test_wino_kernels_use_no_scratch(product_metadata):
    for name, m in product_metadata.items():
        assert m["private_segment_fixed_size"] == 0, (name, m)
        assert m.get("vgpr_spill_count", 0) == 0, (name, m)


def test_wino_kernels_fit_two_waves_per_simd(product_metadata):
    for name, m in product_metadata.items():
        assert m["vgpr_count"] <= 256, (name, m)
