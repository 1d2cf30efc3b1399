"""CPU: the head backward entry points exist, and the pinned float64 autograd the GPU tests measure against (head_grad_scenario) is
itself right: central differences in float64, signs pinned to the unperturbed factors, along random unit directions over features
and weights.  The same for the restated rot6d_to_rotmat."""
import ctypes
import os

import pytest
import torch

import head_grad_scenario as HS
from hierarchicalprobabilistic3dhuman_amd import _capi

NEW_SYMBOLS = ("hps_head_forward_refine", "hps_head_pose_levels_backward", "hps_head_trunk_backward", "hps_rot6d_to_rotmat_backward")
# tests/test_smpl_backward_host.py's tolerance.  There it is relative to the directional derivative; here the direction is a unit
# vector over ~1.6 million entries, the directional derivative is a small multiple of max|g| or far less, and the tolerance is
# stated relative to max|g| over all gradient tensors.
FD_TOL = 1e-7
H = 1e-4            # head, unit directions over ~1.6 million entries: truncation ~ h^2 |f'''| / 6, rounding ~ 1e-16 |loss| / h
H_ROT = 1e-6        # rot6d, unit directions over 6 n entries (third derivatives ~ |a|^-3 are not small): rounding ~ 1e-10 |loss|


def test_backward_entry_points_are_exported():
    if not os.path.exists(_capi.LIB_PATH):
        pytest.skip("libhps.so is not built")
    lib = ctypes.CDLL(_capi.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), "libhps.so does not export %s" % name
        assert name in _capi.EXPORTED_SYMBOLS


def test_backward_workspaces_and_argument_validation_need_no_gpu():
    if not os.path.exists(_capi.LIB_PATH):
        pytest.skip("libhps.so is not built")
    q = _capi.query_workspace
    assert q(_capi.WS_HEAD_LEVELS_BWD, 3, 7000, 23) == 3 * (2 * 7000 + 23 * (128 + 128 + 9)) * 4
    assert q(_capi.WS_HEAD_TRUNK_BWD, 3, 512 + 512 + 256, 29) == 3 * (1280 + 2 * 29) * 4
    lib = _capi.load()
    assert lib.hps_rot6d_to_rotmat_backward(None, None, None, 1, None) == -1
    assert b"null pointer" in lib.hps_last_error()
    assert lib.hps_head_trunk_backward(*([None, 512] + [None] * 20 + [1, 512, 512, 10, 6, 3, 256, None])) == -1
    assert lib.hps_head_forward_refine(*([None, 512] + [None] * 9 + [8] + [None] * 6 + [1.0] + [None] * 13 + [1, 512, 512, 29, 256, 128, 23, None])) == -1
    assert lib.hps_head_pose_levels_backward(*([None, 256, 128, None, None, 8] + [None] * 21 + [1, 23, 7000, None])) == -1


@pytest.mark.parametrize("recipe,B", [("spread", 1), ("spread", 3), ("spread", 130), ("default", 3)])
def test_gap_filter_keeps_enough_rows_and_the_spread_recipe_has_improper_matrices(recipe, B):
    feats, kept, n = HS.features(recipe, B)                       # asserts the gap condition on the rows used and the kept share
    print("%s B=%d: %d of %d candidate rows kept" % (recipe, B, kept, n))
    assert feats.shape == (B, 512) and 4 * kept >= n
    sd64 = {k: v.double() for k, v in HS.state(recipe).items()}
    with torch.no_grad():
        out = HS.head(sd64, feats.double())
    assert float(HS.min_gap(out["pose_S"]).min()) >= HS.MIN_GAP
    share = HS.improper_share(out)
    print("share of matrices with det U det V = -1: %.3f" % share)
    if recipe == "default":
        assert share == 0.0
    elif B >= 3:
        assert share >= 0.05                                      # the proper fix (:144-150) is exercised with both signs


@pytest.mark.parametrize("recipe", ["spread", "default"])
def test_pinned_float64_gradient_agrees_with_central_differences(recipe):
    B = 3
    feats, _, _ = HS.features(recipe, B)
    sd, cot = HS.state(recipe), HS.cotangents(B)
    sd64 = {k: v.double() for k, v in sd.items()}
    names = HS.param_names(sd)
    with torch.no_grad():
        pin32 = HS.head(sd, feats)["pose_U"]                      # on the CPU the pinned run is the fp32 restatement
        U0 = HS.head(sd64, feats.double(), pin32)["pose_U"]       # the unperturbed float64 factors, with those signs
    g64, g32 = HS.reference(("host", recipe, B), sd, feats, pin32, cot)
    gmax = max(float(v.abs().max()) for v in g64.values())
    for k in g64:                                                 # figures of the reference's own fp32 error
        scale = float(g64[k].abs().max())
        if k == "feats" or k.startswith(("fc1.", "fc_embed.")) or k.startswith("fc_pose.10.0"):
            print("%-22s cpu32 error / (2^-23 max|g64|) = %.1f" % (k, float((g32[k] - g64[k]).abs().max()) / (2.0 ** -23 * scale)))

    def loss(f, s):
        with torch.no_grad():
            out = HS.head(s, f, U0)
        return float(sum((cot[k].double() * out[k]).sum() for k in cot))

    gen = torch.Generator().manual_seed(5)
    for trial in range(4):
        d = {k: torch.randn(v.shape, generator=gen, dtype=torch.float64) for k, v in g64.items()}
        norm = sum(float((v * v).sum()) for v in d.values()) ** 0.5
        d = {k: v / norm for k, v in d.items()}
        sp, sm = dict(sd64), dict(sd64)
        for k in names:
            sp[k], sm[k] = sd64[k] + H * d[k], sd64[k] - H * d[k]
        fd = (loss(feats.double() + H * d["feats"], sp) - loss(feats.double() - H * d["feats"], sm)) / (2 * H)
        an = float(sum((g64[k] * d[k]).sum() for k in g64))
        err = abs(fd - an) / gmax
        print("direction %d: central difference %.12e  autograd %.12e  |difference| / max|g| = %.2e" % (trial, fd, an, err))
        assert err <= FD_TOL


@pytest.mark.parametrize("n", [1, 3, 130])
def test_rot6d_float64_gradient_agrees_with_central_differences(n):
    x, cot = HS.rot6d_case(n)
    g64, _ = HS.rot6d_reference(n)
    gmax = float(g64.abs().max())
    gen = torch.Generator().manual_seed(6)
    for trial in range(3):
        d = torch.randn(n, 6, generator=gen, dtype=torch.float64)
        d = d / d.norm()
        f = lambda v: float((HS.rot6d(v) * cot.double()).sum())
        fd = (f(x.double() + H_ROT * d) - f(x.double() - H_ROT * d)) / (2 * H_ROT)
        an = float((g64 * d).sum())
        print("direction %d: central difference %.12e  autograd %.12e  |difference| / max|g| = %.2e" % (trial, fd, an, abs(fd - an) / gmax))
        assert abs(fd - an) / gmax <= FD_TOL
    # at n == 3 the cross product must still run along dim 1 (the reference's torch.cross without dim does not)
    R = HS.rot6d(x.double())
    assert float((torch.matmul(R.transpose(-1, -2), R) - torch.eye(3, dtype=torch.float64)).abs().max()) <= 1e-12
