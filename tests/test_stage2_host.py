"""CPU: the references the stage-2 GPU tests measure against (stage2_scenario) are themselves right, and the inputs chosen for the GPU
tests hide nothing: the two restatements of the reparameterised sampler have the same derivative, the float64 gradient of the
true-noise form agrees with central differences, and every host-noise case meets the conditions on its inputs."""
import ctypes
import os

import pytest
import torch

import head_grad_scenario as HS
import stage2_scenario as S2
from hierarchicalprobabilistic3dhuman_amd import _capi

NEW_SYMBOLS = ("hps_mf_sample_keep_quat", "hps_mf_sample_backward", "hps_head_pose_levels_backward_factors")
FORMS_TOL = 1e-10       # forms (a) and (b) in float64 on float64 quaternions: the same derivative up to float64 rounding
FD_TOL = 1e-7           # tests/test_head_backward_host.py's rule: |central difference - autograd| / max|g| along unit directions
H = 1e-4


def test_stage2_entry_points_are_exported_and_validate_on_the_host():
    if not os.path.exists(_capi.LIB_PATH):
        pytest.skip("libhps.so is not built")
    lib = ctypes.CDLL(_capi.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), "libhps.so does not export %s" % name
        assert name in _capi.EXPORTED_SYMBOLS
    lib = _capi.load()
    assert lib.hps_version() == 502
    fake = ctypes.c_void_p(16)
    assert lib.hps_mf_sample_backward(None, None, None, None, None, None, None, None, 23, 23, 8, 1.5, None, None, None, None) == -1
    assert b"null pointer" in lib.hps_last_error()
    assert lib.hps_mf_sample_backward(fake, fake, fake, None, None, None, fake, fake, 24, 23, 8, 1.5, fake, fake, fake, None) == -1
    assert lib.hps_mf_sample_backward(fake, fake, fake, None, None, None, fake, fake, 23, 23, 0, 1.5, fake, fake, fake, None) == -1
    assert lib.hps_mf_sample_backward(fake, fake, fake, None, None, None, fake, fake, 23, 23, 8, 1.5, None, None, None, None) == 0     # nothing wanted
    assert lib.hps_mf_sample_backward(fake, fake, fake, fake, None, None, fake, fake, 23, 23, 8, 1.5, fake, fake, fake, None) == -1
    assert b"float64 factors" in lib.hps_last_error()
    # the quaternions are what the entry point is for
    assert lib.hps_mf_sample_keep_quat(fake, fake, fake, 23, 23, 8, 64, 1.5, 1.0, None, None, None, 0, 0, 4, fake, None, fake, None) == -1
    assert lib.hps_mf_sample_keep_quat(fake, fake, fake, 23, 23, 8, 4, 1.5, 1.0, None, None, None, 0, 0, 4, fake, fake, fake, None) == -1
    assert lib.hps_head_pose_levels_backward_factors(*([None, 256, 128, None, None, 8] + [None] * 23 + [1, 23, 7000, None])) == -1


def test_switch_is_off_by_default_and_survives_copies_and_reloads():
    import copy
    import pickle
    net = HS.make_net("default")
    assert net.differentiable_factors is False
    state = net.device_state()
    net.set_differentiable_factors(True)
    assert net.differentiable_factors is True and net.device_state() is state       # nothing derived depends on it
    for clone in (copy.deepcopy(net), pickle.loads(pickle.dumps(net)), net.to("cpu"), net.float()):
        assert clone.differentiable_factors is True
    net.load_state_dict(HS.make_net("spread").state_dict())
    assert net.differentiable_factors is True
    net.set_differentiable_factors(False)
    assert net.differentiable_factors is False


def test_orthographic_projection_and_flip():
    from hierarchicalprobabilistic3dhuman_amd import cam_utils
    g = torch.Generator().manual_seed(3)
    pts, cam = torch.randn(4, 17, 3, generator=g), torch.randn(4, 3, generator=g)
    got = cam_utils.orthographic_project_torch(pts, cam)
    want = torch.stack([cam[:, 0:1] * (pts[:, :, 0] + cam[:, 1:2]), cam[:, 0:1] * (pts[:, :, 1] + cam[:, 2:3])], dim=-1)
    assert got.shape == (4, 17, 2) and torch.equal(got, want)
    flipped = cam_utils.flip_about_x(pts)
    assert torch.equal(flipped, torch.stack([pts[..., 0], -pts[..., 1], -pts[..., 2]], dim=-1))


@pytest.mark.parametrize("recipe,B,N,seed,fseed", S2.CASES)
def test_conditions_on_the_chosen_inputs(recipe, B, N, seed, fseed):
    """The GPU cases hide nothing: the gap filter holds (HS.features asserts it), the fp32 and float64 restatements take the same
    accept decisions with every evaluated proposal at least 1e-5 from the threshold, and the fp32 restatement's own worst-tensor
    gradient error stays below 256 x 2^-23 max|g|."""
    _, kept, n = HS.features(recipe, B, fseed)
    assert 4 * kept >= n
    c = S2.host_case(recipe, B, N, seed, fseed)
    flips = int((c["info64"]["keep"] != c["info32"]["keep"]).sum())
    print("%s B=%d N=%d: %d flipped decisions, margins float64 %.2e fp32 %.2e" % (recipe, B, N, flips, c["info64"]["margin"], c["info32"]["margin"]))
    assert flips == 0 and c["info64"]["margin"] >= S2.MIN_MARGIN
    q = c["q64"].float()                                              # what a device would hand back: fp32 quaternions
    g_R = S2.cot_R(B, N)
    g64 = S2.head_vjp(c["sd32"], c["feats"], c["pin"], torch.float64, S2.sampler_loss("b", g_R, q=q))
    g32 = S2.head_vjp(c["sd32"], c["feats"], c["pin"], torch.float32, S2.sampler_loss("b", g_R, q=q))
    worst = S2.worst_ratio(g32, g64)
    print("fp32 restatement's own worst-tensor error: %.1f x 2^-23 max|g|" % worst)
    assert all(float(v.abs().max()) > 0.0 for k, v in g64.items() if k == "feats" or k.startswith("fc_pose."))
    assert worst < S2.FP32_CAP


@pytest.mark.parametrize("recipe,B,N,seed,fseed", S2.CASES[:2])
def test_forms_agree(recipe, B, N, seed, fseed):
    """Forms (a) and (b) have the same gradients with respect to the features and every head parameter: 1e-10 relative to each
    tensor's max|g| on float64 quaternions taken from (a); with the quaternions rounded to fp32 the difference is that rounding."""
    c = S2.host_case(recipe, B, N, seed, fseed)
    g_R = S2.cot_R(B, N)
    ga = S2.head_vjp(c["sd32"], c["feats"], c["pin"], torch.float64, S2.sampler_loss("a", g_R, N=N, eps=c["eps"], w=c["w"]))
    gb = S2.head_vjp(c["sd32"], c["feats"], c["pin"], torch.float64, S2.sampler_loss("b", g_R, q=c["q64"]))
    gr = S2.head_vjp(c["sd32"], c["feats"], c["pin"], torch.float64, S2.sampler_loss("b", g_R, q=c["q64"].float()))
    worst = worst_rounded = 0.0
    for k in ga:
        scale = float(ga[k].abs().max())
        if scale == 0.0:
            assert float(gb[k].abs().max()) == 0.0, k
            continue
        worst = max(worst, float((ga[k] - gb[k]).abs().max()) / scale)
        worst_rounded = max(worst_rounded, float((ga[k] - gr[k]).abs().max()) / scale)
    print("forms (a) - (b): %.2e relative; with fp32-rounded quaternions %.2e" % (worst, worst_rounded))
    assert worst <= FORMS_TOL


def test_true_noise_float64_gradient_agrees_with_central_differences():
    c = S2.host_case(*S2.CASES[0])
    B, N = S2.CASES[0][1:3]
    g_R = S2.cot_R(B, N).double()
    sd64 = {k: v.double() for k, v in c["sd32"].items()}
    names = HS.param_names(sd64)
    g64 = S2.head_vjp(c["sd32"], c["feats"], c["pin"], torch.float64, S2.sampler_loss("a", g_R, N=N, eps=c["eps"], w=c["w"]))
    gmax = max(float(v.abs().max()) for v in g64.values())
    with torch.no_grad():
        U0 = HS.head(sd64, c["feats"].double(), c["pin"])["pose_U"]    # the unperturbed float64 factors, with the pinned signs

    def loss(f, s):
        with torch.no_grad():
            out = HS.head(s, f, U0)
            R, _, info = S2.sample_true(out["pose_U"], out["pose_S"], out["pose_V"], c["eps"], c["w"], N)
        assert torch.equal(info["keep"], c["info64"]["keep"]), "the step crossed an accept threshold: not a difference of one branch"
        return float((g_R * R).sum())

    gen = torch.Generator().manual_seed(8)
    for trial in range(3):
        d = {k: torch.randn(v.shape, generator=gen, dtype=torch.float64) for k, v in g64.items()}
        norm = sum(float((v * v).sum()) for v in d.values()) ** 0.5
        d = {k: v / norm for k, v in d.items()}
        sp, sm = dict(sd64), dict(sd64)
        for k in names:
            sp[k], sm[k] = sd64[k] + H * d[k], sd64[k] - H * d[k]
        fd = (loss(c["feats"].double() + H * d["feats"], sp) - loss(c["feats"].double() - H * d["feats"], sm)) / (2 * H)
        an = float(sum((g64[k] * d[k]).sum() for k in g64))
        err = abs(fd - an) / gmax
        print("direction %d: central difference %.12e  autograd %.12e  |difference| / max|g| = %.2e" % (trial, fd, an, err))
        assert err <= FD_TOL
