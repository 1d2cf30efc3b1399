"""GPU: SMPL.forward under autograd -- the device backward (hps_smpl_lbs_backward, hps_smpl_blend_backward,
hps_smpl_pose_prep_backward) against torch autograd through the float64 CPU oracle.

Accuracy rule, for every gradient tensor (smpl_grad_scenario.check):
    max|g_dev - g64| <= 4 * max(max|g_cpu32 - g64|, 2^-23 max|g64|)
Shapes: M = 1, 3 and 130 (one full and one partial 128-mesh tile); V = 6890 ends in a partial 64-vertex panel and a partial 128-vertex
chunk of the skinning backward, 20 736 padded columns end in a half slice of the blend backward.
"""
import pytest
import torch

import mf_loss_scenario as LS
import smpl_grad_scenario as SC
from hierarchicalprobabilistic3dhuman_amd.matrix_fisher_loss import PoseMFShapeGaussianLoss
from hierarchicalprobabilistic3dhuman_amd.smpl_official import SMPL

pytestmark = pytest.mark.gpu


def _run(smpl, c, dev, use_gV=True, use_gJ=True, wrt=SC.INPUTS):
    """One forward + backward on the device: (leaves, output)."""
    x = {k: c[k].to(dev) for k in SC.INPUTS if c[k] is not None}
    for k in wrt:
        if k in x:
            x[k].requires_grad_(True)
    out = smpl(betas=x["betas"], body_pose=x["body_pose"], global_orient=x["global_orient"], transl=x.get("transl"),
               pose2rot=c["pose2rot"])
    outs, cots = [], []
    if use_gV:
        outs.append(out.vertices); cots.append(c["gV"].to(dev))
    if use_gJ:
        outs.append(out.joints); cots.append(c["gJ"].to(dev))
    torch.autograd.backward(outs, cots)
    return x, out


def _check_all(x, key, use_gV=True, use_gJ=True):
    g64, g32 = SC.reference(key, use_gV, use_gJ)
    for k in g64:
        assert x[k].grad is not None and x[k].grad.shape == x[k].shape and x[k].grad.dtype == x[k].dtype
        assert bool(torch.isfinite(x[k].grad).all())
        SC.check(k, x[k].grad, g64[k], g32[k])


# (M, pose2rot, transl, zero_row)
CASES = [(1, False, False, None), (1, True, True, 0), (3, False, True, None), (3, True, False, None), (3, True, True, 1),
         (130, False, False, None), (130, True, True, 5)]


@pytest.mark.parametrize("key", CASES, ids=lambda k: "M%d-%s-%s-zero%s" % (k[0], "aa" if k[1] else "rotmat", "transl" if k[2] else "notransl", k[3]))
def test_gradients_match_the_float64_oracle(dev, smpl_gpu, key):
    x, _ = _run(smpl_gpu, SC.case(*key), dev)
    _check_all(x, key)


def test_betas_given_as_one_row_are_summed_over_the_meshes(dev, smpl_gpu):
    key = (3, False, False, None, 1)
    x, _ = _run(smpl_gpu, SC.case(*key), dev)
    assert x["betas"].grad.shape == (1, SC.NB)
    _check_all(x, key)


@pytest.mark.parametrize("only", SC.INPUTS)
def test_gradient_for_one_input_only(dev, smpl_gpu, only):
    key = (3, True, True, None)
    x, _ = _run(smpl_gpu, SC.case(*key), dev, wrt=(only,))
    g64, g32 = SC.reference(key)
    for k in x:
        if k == only:
            SC.check(k, x[k].grad, g64[k], g32[k])
        else:
            assert x[k].grad is None


@pytest.mark.parametrize("M", [3, 130])
@pytest.mark.parametrize("use_gV,use_gJ,route", [(True, False, "dense"), (False, True, "picked"), (True, True, "dense")])
def test_cotangent_on_vertices_joints_or_both(dev, smpl_gpu, M, use_gV, use_gJ, route):
    key = (M, False, True, None)
    smpl_gpu.keep_intermediates = True
    try:
        x, _ = _run(smpl_gpu, SC.case(*key), dev, use_gV, use_gJ)
        assert smpl_gpu._last_backward["route"] == route
    finally:
        smpl_gpu.keep_intermediates = False
    _check_all(x, key, use_gV, use_gJ)


def test_unfused_mesh_route(dev, smpl_assets):
    smpl = SMPL(smpl_assets[0]).to(dev)
    smpl.fused_mesh = False
    key = (3, True, True, 1)
    x, _ = _run(smpl, SC.case(*key), dev)
    _check_all(x, key)


def test_forward_bits_under_grad_equal_the_no_grad_call(dev, smpl_gpu):
    c = SC.case(3, True, True, None)
    x, out = _run(smpl_gpu, c, dev)
    assert out.vertices.grad_fn is not None and out.joints.grad_fn is not None
    with torch.no_grad():
        ref = smpl_gpu(betas=x["betas"], body_pose=x["body_pose"], global_orient=x["global_orient"], transl=x["transl"],
                       pose2rot=True)
    assert ref.vertices.grad_fn is None
    assert torch.equal(out.vertices, ref.vertices) and torch.equal(out.joints, ref.joints)


def test_backward_is_bitwise_repeatable(dev, smpl_gpu):
    c = SC.case(130, True, True, 5)
    runs = [_run(smpl_gpu, c, dev)[0] for _ in range(2)]
    for k in runs[0]:
        assert torch.equal(runs[0][k].grad, runs[1][k].grad)


@pytest.mark.parametrize("use_gV", [True, False])
def test_a_mesh_gets_the_same_bits_alone_as_in_a_batch(dev, smpl_gpu, use_gV):
    c = SC.case(130, True, True, 5)
    x, _ = _run(smpl_gpu, c, dev, use_gV=use_gV)
    one = {k: (v[7:8] if torch.is_tensor(v) else v) for k, v in c.items()}
    one["M"] = 1
    x1, _ = _run(smpl_gpu, one, dev, use_gV=use_gV)
    for k in x:
        assert torch.equal(x[k].grad[7:8], x1[k].grad), k


def test_forward_and_backward_never_wait_for_the_host(dev, smpl_gpu):
    c = SC.case(3, True, True, 1)
    x = {k: c[k].to(dev).requires_grad_(True) for k in SC.INPUTS}
    gV, gJ = c["gV"].to(dev), c["gJ"].to(dev)
    one = torch.ones((), device=dev)
    for picked in (False, True):       # both routes; the picked route's constants are built inside the guarded region
        smpl = smpl_gpu
        torch.cuda.synchronize()
        prev = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        try:
            with pytest.raises(RuntimeError):              # the mode is live on this build: a synchronising call is refused
                torch.nonzero(one)
            out = smpl(betas=x["betas"], body_pose=x["body_pose"], global_orient=x["global_orient"], transl=x["transl"], pose2rot=True)
            if picked:
                torch.autograd.backward([out.joints], [gJ])
            else:
                torch.autograd.backward([out.vertices, out.joints], [gV, gJ])
        finally:
            torch.cuda.set_sync_debug_mode(prev)
        torch.cuda.synchronize()
    assert all(v.grad is not None for v in x.values())


def test_chain_with_the_device_loss(dev, smpl_gpu):
    """PoseMFShapeGaussianLoss on verts / joints3D taken from SMPL(pose, betas): pose.grad and betas.grad against the float64 oracle
    chain (the loss's 3D terms restated: weight * mean squared error, losses/matrix_fisher_loss.py:289-292, :298-299)."""
    case = "s2_mean_ns9"
    pred, target = LS.loss_inputs(case)
    B = pred["verts"].shape[0]
    c = SC.case(B, False, False, None, None, 3)
    gen = torch.Generator().manual_seed(77)
    target["verts"] = torch.randn(B, 6890, 3, generator=gen) * 0.3
    target["joints3D"] = torch.randn(B, LS.P3D, 3, generator=gen) * 0.3
    pred["verts"] = torch.zeros(B, 6890, 3)
    pred["joints3D"] = torch.zeros(B, LS.P3D, 3)
    cfg = LS.loss_config(case)
    w_v, w_j = cfg.WEIGHTS.VERTS3D, cfg.WEIGHTS.JOINTS3D
    sel = slice(90 - LS.P3D, 90)           # regressed joints: their gradient reaches the mesh through the regressor

    def oracle(dtype):
        x = SC.leaves(c, dtype)            # (no transl in this case: the three inputs)
        out = SC.O.smpl_forward(SC.params(dtype), betas=x["betas"], body_pose=x["body_pose"], global_orient=x["global_orient"],
                                pose2rot=False)
        loss = w_v * ((out["vertices"] - target["verts"].to(dtype)) ** 2).mean() + \
            w_j * ((out["joints"][:, sel] - target["joints3D"].to(dtype)) ** 2).mean()
        loss.backward()
        return {k: v.grad.double() for k, v in x.items()}

    g64, g32 = oracle(torch.float64), oracle(torch.float32)
    target_dict, pred_dict, _ = LS.make_dicts(pred, target, device=dev)
    x = {k: c[k].to(dev).requires_grad_(True) for k in ("global_orient", "body_pose", "betas")}
    out = smpl_gpu(betas=x["betas"], body_pose=x["body_pose"], global_orient=x["global_orient"], pose2rot=False)
    pred_dict["verts"], pred_dict["joints3D"] = out.vertices, out.joints[:, sel]
    total = PoseMFShapeGaussianLoss(cfg, LS.IMG_WH)(target_dict, pred_dict)
    total.backward()
    for k in x:
        SC.check(k, x[k].grad, g64[k], g32[k])


def test_private_hook_with_a_grad_requiring_input_raises(dev, smpl_gpu):
    c = SC.case(3, True, True, None)
    betas = c["betas"].to(dev).requires_grad_(True)
    with pytest.raises(ValueError):
        smpl_gpu(betas=betas, body_pose=c["body_pose"].to(dev), global_orient=c["global_orient"].to(dev), _defer_joints=lambda args: None)
    with torch.no_grad():                  # ... and is untouched where nothing is differentiated
        smpl_gpu(betas=betas, body_pose=c["body_pose"].to(dev), global_orient=c["global_orient"].to(dev), _after_mesh=lambda ev: None)
