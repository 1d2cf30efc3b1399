"""GPU: PoseMFShapeGaussianNet.forward and rot6d_to_rotmat under autograd (csrc/head_backward.hip) against the pinned float64
reference of head_grad_scenario, by the project's accuracy rule (smpl_grad_scenario.bound / check): per tensor
max|g_dev - g64| <= 4 max(max|g32 - g64|, 2^-23 max|g64|)."""
import copy

import pytest
import torch

import head_grad_scenario as HS
from hierarchicalprobabilistic3dhuman_amd import configs, rigid_transform_utils as rtu
from hierarchicalprobabilistic3dhuman_amd.matrix_fisher_loss import PoseMFShapeGaussianLoss

pytestmark = pytest.mark.gpu

_NETS = {}


def net_of(recipe, dev):
    """The recipe's net on the device, shared by the tests (they restore every switch they touch and never step its parameters)."""
    if recipe not in _NETS:
        _NETS[recipe] = HS.make_net(recipe).to(dev)
    return _NETS[recipe]


def outputs(out):
    pose_F, pose_U, pose_S, pose_V, mode, shape_dist, glob, cam = out
    return dict(pose_F=pose_F, pose_U=pose_U, pose_S=pose_S, pose_V=pose_V, mode=mode, loc=shape_dist.loc, scale=shape_dist.scale,
                glob=glob, cam=cam)


def device_grads(net, feats, cot, feats_grad=True):
    """(gradients dict over "feats" and the parameter names, the forward's outputs) of sum_k <cot[k], out[k]> on the device."""
    net.zero_grad(set_to_none=True)
    f = feats.detach().clone().requires_grad_(feats_grad)
    out = outputs(net(None, input_feats=f))
    loss = sum((cot[k].to(f.device) * out[k]).sum() for k in cot)
    loss.backward()
    grads = {k: p.grad for k, p in net.named_parameters() if k.startswith(HS.HEAD_PREFIXES)}
    grads["feats"] = f.grad
    return grads, out


def check_all(tag, grads, g64, g32):
    worst = {}
    for k in g64:
        if k not in grads:                                        # a leaf this case does not differentiate
            continue
        if float(g64[k].abs().max()) == 0.0:                      # nothing reaches this tensor: None or exact zeros, no ratio to print
            assert grads[k] is None or float(grads[k].abs().max()) == 0.0, k
            continue
        assert grads[k] is not None, (k, "no gradient on the device")
        group = "feats" if k == "feats" else k.split(".")[0]
        worst[group] = max(worst.get(group, 0.0), HS.check("%s %s" % (tag, k), grads[k], g64[k], g32[k]))
    print("%s worst error per group in 2^-23 max|g64|: %s" % (tag, {k: round(v, 1) for k, v in worst.items()}))


def test_route_grad_fn_and_forward_bits(dev):
    """Fails without the feature: under grad mode the outputs carry a grad_fn (pose_U / pose_V do not require grad) and equal the
    no_grad call bit for bit; under no_grad nothing has a grad_fn."""
    net = net_of("spread", dev)
    feats = HS.features("spread", 3)[0].to(dev)
    with torch.no_grad():
        plain = outputs(net(None, input_feats=feats))
    assert all(v.grad_fn is None and not v.requires_grad for v in plain.values())
    for mode_switch in (False, True):
        net.set_latency_mode(mode_switch)
        try:
            with torch.no_grad():
                want = outputs(net(None, input_feats=feats))
            got = outputs(net(None, input_feats=feats))
        finally:
            net.set_latency_mode(False)
        for k in HS.OUTPUTS:
            assert got[k].grad_fn is not None, k
        assert not got["pose_U"].requires_grad and not got["pose_V"].requires_grad
        for k in want:
            assert torch.equal(got[k], want[k]), (k, mode_switch)
    net.svd_mode = "host"
    try:
        with torch.no_grad():
            want = outputs(net(None, input_feats=feats))
        got = outputs(net(None, input_feats=feats))
    finally:
        net.svd_mode = "device"
    assert all(torch.equal(got[k], want[k]) for k in want) and got["mode"].grad_fn is not None


@pytest.mark.parametrize("recipe,B", [("spread", 1), ("spread", 3), ("spread", 130), ("default", 3)])
def test_all_gradients_against_the_pinned_float64_reference(dev, recipe, B):
    """Every parameter gradient and the feature gradient with standard-normal cotangents on all seven differentiable outputs;
    B = 130 crosses the batch tiles of the level kernels (4 images) and ends in a partial tile."""
    net = net_of(recipe, dev)
    feats, cot = HS.features(recipe, B)[0], HS.cotangents(B)
    grads, out = device_grads(net, feats.to(dev), cot)
    g64, g32 = HS.reference(("dev", recipe, B, "all"), HS.state(recipe), feats, out["pose_U"], cot)
    assert all(grads[k] is not None for k in g64)
    check_all("%s B=%d" % (recipe, B), grads, g64, g32)


@pytest.mark.parametrize("which", [("mode",), ("pose_F", "pose_S"), ("loc", "scale", "glob", "cam")], ids=lambda w: "+".join(w))
def test_partial_cotangents(dev, which):
    net, B = net_of("spread", dev), 3
    feats = HS.features("spread", B)[0]
    cot = {k: HS.cotangents(B)[k] for k in which}
    grads, out = device_grads(net, feats.to(dev), cot)
    g64, g32 = HS.reference(("dev", "spread", B, which), HS.state("spread"), feats, out["pose_U"], cot)
    check_all("cotangents on %s" % "+".join(which), grads, g64, g32)
    if "mode" not in which and "pose_F" not in which:
        for k, g in grads.items():
            if k.startswith("fc_pose."):
                assert g is None or float(g.abs().max()) == 0.0, k


def test_frozen_parameters_and_frozen_features(dev):
    net, B = copy.deepcopy(net_of("spread", dev)), 3
    feats, cot = HS.features("spread", B)[0], HS.cotangents(B)
    for p in net.parameters():
        p.requires_grad_(False)
    grads, out = device_grads(net, feats.to(dev), cot)
    g64, g32 = HS.reference(("dev", "spread", B, "all"), HS.state("spread"), feats, out["pose_U"], cot)
    assert all(v is None for k, v in grads.items() if k != "feats")
    HS.check("frozen parameters: feats", grads["feats"], g64["feats"], g32["feats"])
    for p in net.parameters():
        p.requires_grad_(True)
    grads, _ = device_grads(net, feats.to(dev), cot, feats_grad=False)
    assert grads.pop("feats") is None
    check_all("frozen features", grads, g64, g32)


@pytest.mark.parametrize("switch,B", [("latency", 1), ("host", 3)])
def test_latency_mode_and_host_svd_mode(dev, switch, B):
    net = copy.deepcopy(net_of("spread", dev))
    if switch == "latency":
        net.set_latency_mode(True)
    else:
        net.svd_mode = "host"
    feats, cot = HS.features("spread", B)[0], HS.cotangents(B)
    grads, out = device_grads(net, feats.to(dev), cot)
    g64, g32 = HS.reference(("dev", "spread", B, "all", switch), HS.state("spread"), feats, out["pose_U"], cot)
    check_all("%s B=%d" % (switch, B), grads, g64, g32)


def test_backward_is_repeatable_and_images_are_independent(dev):
    net, B = net_of("spread", dev), 130
    feats, cot = HS.features("spread", B)[0].to(dev), HS.cotangents(B)
    a, _ = device_grads(net, feats, cot)
    a = {k: v.clone() for k, v in a.items()}
    b, _ = device_grads(net, feats, cot)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    for i in (0, 67, 129):                                        # first and last image, one in the middle of a batch tile
        one, _ = device_grads(net, feats[i:i + 1], {k: v[i:i + 1] for k, v in cot.items()})
        assert torch.equal(one["feats"][0], a["feats"][i]), i


@pytest.mark.parametrize("n", [1, 3, 130])
def test_rot6d_to_rotmat_gradient_and_forward_bits(dev, n):
    x, cot = HS.rot6d_case(n)
    g64, g32 = HS.rot6d_reference(n)
    with torch.no_grad():
        want = rtu.rot6d_to_rotmat(x.to(dev))
    xd = x.to(dev).requires_grad_(True)
    got = rtu.rot6d_to_rotmat(xd)
    assert got.grad_fn is not None and want.grad_fn is None and torch.equal(got, want)
    (got * cot.to(dev)).sum().backward()
    HS.check("rot6d n=%d" % n, xd.grad, g64, g32)


def test_loss_smpl_rot6d_chain_reaches_every_head_parameter(dev, smpl_gpu):
    """PoseMFShapeGaussianLoss (STAGE1) on the head's outputs, SMPL on the mode and loc, rot6d_to_rotmat on glob: .backward() leaves
    a gradient on every head parameter, equal by the rule to the reference VJP fed with the output cotangents the device chain
    produced."""
    net, B = net_of("spread", dev), 3
    feats = HS.features("spread", B)[0]
    net.zero_grad(set_to_none=True)
    out = outputs(net(None, input_feats=feats.to(dev)))
    for k in HS.OUTPUTS:
        out[k].retain_grad()
    glob_rotmats = rtu.rot6d_to_rotmat(out["glob"])
    smpl_out = smpl_gpu(body_pose=out["mode"], global_orient=glob_rotmats.unsqueeze(1), betas=out["loc"], pose2rot=False)
    g = torch.Generator().manual_seed(21)
    target = {"pose_params_rotmats": rtu.batch_rodrigues((torch.randn(B * 23, 3, generator=g) * 0.3).to(dev)).view(B, 23, 3, 3),
              "shape_params": torch.randn(B, 10, generator=g).to(dev),
              "joints2D": (torch.rand(B, 17, 2, generator=g) * 256).to(dev),
              "joints2D_vis": torch.ones(B, 17, dtype=torch.bool, device=dev),
              "glob_rotmats": rtu.batch_rodrigues((torch.randn(B, 3, generator=g) * 0.3).to(dev)),
              "verts": torch.randn(B, 6890, 3, generator=g).to(dev), "joints3D": torch.randn(B, 14, 3, generator=g).to(dev)}
    cam = out["cam"]
    joints_coco = smpl_out.joints[:, :17]
    joints2D = (joints_coco[:, :, :2] * cam[:, None, :1] + cam[:, None, 1:]).unsqueeze(1)         # (B, 1 sample, 17, 2)
    from torch.distributions import Normal
    pred = {"pose_params_F": out["pose_F"], "pose_params_U": out["pose_U"], "pose_params_S": out["pose_S"],
            "pose_params_V": out["pose_V"], "shape_params": Normal(out["loc"], out["scale"], validate_args=False),
            "joints2D": joints2D, "glob_rotmats": glob_rotmats, "verts": smpl_out.vertices, "joints3D": smpl_out.joints[:, :14]}
    criterion = PoseMFShapeGaussianLoss(loss_config=configs.get_cfg_defaults().LOSS.STAGE1, img_wh=256)
    loss = criterion(target, pred)
    loss.backward()
    cot = {k: out[k].grad for k in HS.OUTPUTS if out[k].grad is not None}
    assert {"pose_F", "pose_S", "mode", "loc", "glob", "cam"} <= set(cot)
    grads = {k: p.grad for k, p in net.named_parameters() if k.startswith(HS.HEAD_PREFIXES)}
    assert all(v is not None for v in grads.values())
    g64, g32 = HS.reference(("dev", "spread", B, "chain"), HS.state("spread"), feats, out["pose_U"], cot)
    check_all("chain", grads, g64, g32)


def test_parameters_stepped_in_place_are_not_stale(dev):
    net, B = copy.deepcopy(net_of("spread", dev)), 3
    feats, cot = HS.features("spread", B)[0].to(dev), HS.cotangents(B)
    head_params = [p for k, p in net.named_parameters() if k.startswith(HS.HEAD_PREFIXES)]
    opt = torch.optim.SGD(head_params, lr=1e-3)
    device_grads(net, feats, cot)
    opt.step()
    fresh = HS.make_net("spread").to(dev)
    fresh.load_state_dict(net.state_dict())
    with torch.no_grad():
        want = outputs(fresh(None, input_feats=feats))
        plain = outputs(net(None, input_feats=feats))
    grad_mode = outputs(net(None, input_feats=feats))
    for k in want:
        assert torch.equal(plain[k], want[k]) and torch.equal(grad_mode[k], want[k]), k
    # a module that never took the differentiable route does not look at its parameters again
    never = copy.deepcopy(fresh)
    with torch.no_grad():
        never(None, input_feats=feats)
        state = never.device_state()
        never.fc1.bias.add_(1.0)
        never(None, input_feats=feats)
    assert never.device_state() is state and not never._track_versions
