"""What hipcc makes of csrc/stem_wino.hip and csrc/stem_wino_dev.hip, from the kernel metadata alone (no GPU): the files are compiled to
gfx950 assembly with the build recipe's flags, as tests/test_wino_codegen.py does for the Winograd layers.

csrc/stem_wino.hip is part of both libraries and must hold, with the product flags and with the dev flags (-DHPS_DEV_BUILD), exactly the
three stem_wino_kernel instantiations that ship -- <POOL, NCHW> = <false, false>, <true, false>, <true, true> -- with the same metadata
and no profiling form; csrc/stem_wino_dev.hip holds the thirteen stem_wino_ablate_kernel instantiations.  Every one of them must

  * use no scratch (.private_segment_fixed_size = 0, no spilled VGPR): an ablation's time must never be a spill's time;
  * fit 256 registers (.vgpr_count <= 256): eight waves per workgroup, one workgroup per CU, so two waves per SIMD of 512 registers.
"""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import wino_isa_counts as W  # noqa: E402


def _stem_metadata(dev, source):
    meta = W.metadata(W.compile_asm(dev=dev, source=source))
    return {k: v for k, v in meta.items() if "stem_wino" in k}


def _form(name):
    """(AB or None, POOL, NCHW) from a mangled kernel name: ...kernelI[Li<AB>E]Lb<POOL>ELb<NCHW>EEE..."""
    return re.search(r"kernelI(?:Li(\d+)E)?Lb([01])ELb([01])EEE", name).groups()


def _assert_no_scratch_two_waves(meta):
    for name, m in meta.items():
        assert m["private_segment_fixed_size"] == 0, (name, m)
        assert m.get("vgpr_spill_count", 0) == 0, (name, m)
        assert m["vgpr_count"] <= 256, (name, m)


@pytest.fixture(scope="module")
def product_metadata():
    return _stem_metadata(dev=False, source="stem_wino.hip")


def test_stem_file_holds_the_three_product_kernels(product_metadata):
    assert len(product_metadata) == 3, sorted(product_metadata)
    assert all("stem_wino_kernel" in k and "ablate" not in k for k in product_metadata), sorted(product_metadata)
    # <POOL, NCHW> as mangled template arguments: the three forms that have an entry point
    assert sorted(_form(k) for k in product_metadata) == [(None, "0", "0"), (None, "1", "0"), (None, "1", "1")]


def test_stem_kernels_use_no_scratch_and_fit_two_waves_per_simd(product_metadata):
    _assert_no_scratch_two_waves(product_metadata)


def test_stem_file_is_the_same_in_the_dev_library(product_metadata):
    dev = _stem_metadata(dev=True, source="stem_wino.hip")
    assert not any("ablate" in k for k in dev), sorted(dev)
    assert dev == product_metadata                            # same three names, registers and (no) scratch: the file knows no dev build


def test_dev_file_holds_the_thirteen_ablations_without_scratch():
    meta = _stem_metadata(dev=True, source="stem_wino_dev.hip")
    assert len(meta) == 13 and all("stem_wino_ablate_kernel" in k for k in meta), sorted(meta)
    forms = sorted((int(ab), pool, nchw) for ab, pool, nchw in map(_form, meta))
    assert forms == [(ab, "0", "0") for ab in range(1, 8)] + [(ab, "1", "1") for ab in range(8, 14)]
    _assert_no_scratch_two_waves(meta)
