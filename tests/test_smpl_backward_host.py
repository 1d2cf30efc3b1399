"""CPU: the SMPL backward entry points exist, and the float64 oracle gradient the GPU tests measure against is itself right
(central differences along random directions)."""
import ctypes

import pytest
import torch

import smpl_grad_scenario as SC
from hierarchicalprobabilistic3dhuman_amd import _capi, build as hps_build

NEW_SYMBOLS = ("hps_smpl_lbs_backward", "hps_smpl_blend_backward", "hps_smpl_pose_prep_backward")


def test_backward_entry_points_are_exported():
    lib = ctypes.CDLL(hps_build.build(force=False, verbose=False))
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), "libhps.so does not export %s" % name
        assert name in _capi.EXPORTED_SYMBOLS


def test_backward_workspaces_and_argument_validation_need_no_gpu():
    q = _capi.query_workspace
    assert q(_capi.WS_SMPL_LBS_BWD, 3, 6890, 24) == 54 * 3 * (24 * 12 + 8 * 3) * 4  # 54 chunks of 128 vertices; 24 joints x 12, 8 rows x 3 for g_transl
    assert q(_capi.WS_SMPL_BLEND_BWD, 3, 224, 20736) == 41 * 224 * 128 * 4        # 41 slices of 512 columns
    lib = _capi.load()
    assert lib.hps_smpl_blend_backward(None, None, None, None, 1, 224, 128, 20736, 20736, None) == -1
    assert b"null pointer" in lib.hps_last_error()
    assert lib.hps_smpl_lbs_backward(None, 0, None, None, None, 4, 24, None, None, 0, None, None, None, None, None, None, 1, 1, None) == -1
    assert lib.hps_smpl_pose_prep_backward(None, None, 0, None, 10, None, None, None, None, 24, None, None, 0, None, 128, None, None,
                                           None, 1, None) == -1


# (M, pose2rot, transl, zero_row): both pose routes, with and without transl, one all-zero rotation-vector mesh
FD_CASES = [(3, False, True, None), (3, True, True, 1), (2, True, False, None), (2, False, False, None)]


@pytest.mark.parametrize("key", FD_CASES, ids=lambda k: "M%d-%s-%s-zero%s" % (k[0], "aa" if k[1] else "rotmat", "transl" if k[2] else "notransl", k[3]))
def test_float64_oracle_gradient_agrees_with_central_differences(key):
    c = SC.case(*key)
    g64, _ = SC.reference(key)
    x0 = {k: c[k].double() for k in SC.INPUTS if c[k] is not None}
    gen = torch.Generator().manual_seed(5)
    h = 1e-5
    for trial in range(3):
        d = {k: torch.randn(v.shape, generator=gen, dtype=torch.float64) for k, v in x0.items()}
        with torch.no_grad():
            lp = SC.forward_loss(c, torch.float64, {k: x0[k] + h * d[k] for k in x0})
            lm = SC.forward_loss(c, torch.float64, {k: x0[k] - h * d[k] for k in x0})
        fd = float(lp - lm) / (2 * h)
        an = float(sum((g64[k] * d[k]).sum() for k in x0))
        rel = abs(fd - an) / abs(an)
        print("direction %d: central difference %.12e  autograd %.12e  relative error %.2e" % (trial, fd, an, rel))
        assert rel <= 1e-7
