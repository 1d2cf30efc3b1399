"""GPU: the stage-2 training step (train/train_poseMF_shapeGaussian_net.py:292-320) on the device -- the reparameterised matrix-Fisher
sampler under autograd (hps_mf_sample_keep_quat / hps_mf_sample_backward, csrc/mf_sample.hip) and pose_U / pose_V as differentiable
head outputs (hps_head_pose_levels_backward_factors) -- against float64 autograd of stage2_scenario's pinned form (b), by the project's
accuracy rule (smpl_grad_scenario.bound / check): per tensor max|g_dev - g64| <= 4 max(max|g32 - g64|, 2^-23 max|g64|).  The reference is
pinned on the device's pose_U signs and on the device's own accepted quaternions."""
import copy

import pytest
import torch

import head_grad_scenario as HS
import smpl_grad_scenario as SC
import stage2_scenario as S2
from hierarchicalprobabilistic3dhuman_amd import _capi, cam_utils, configs, rigid_transform_utils as rtu, sampling_utils as su
from hierarchicalprobabilistic3dhuman_amd.label_conversions import ALL_JOINTS_TO_COCO_MAP, ALL_JOINTS_TO_H36M_MAP, H36M_TO_J14
from hierarchicalprobabilistic3dhuman_amd.matrix_fisher_loss import PoseMFShapeGaussianLoss, matrix_fisher_nll

pytestmark = pytest.mark.gpu

_NETS = {}
NS = 8                          # LOSS.NUM_SAMPLES of the reference's configuration
J14 = [ALL_JOINTS_TO_H36M_MAP[i] for i in H36M_TO_J14]


def net_of(recipe, dev, factors=True):
    """The recipe's net on the device with the switch set, shared by the tests (they never step its parameters)."""
    key = (recipe, factors)
    if key not in _NETS:
        net = HS.make_net(recipe).to(dev)
        net.set_differentiable_factors(factors)
        _NETS[key] = net
    return _NETS[key]


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
        if k not in grads:
            continue
        if float(g64[k].abs().max()) == 0.0:
            assert grads[k] is None or float(grads[k].abs().max()) == 0.0, k
            continue
        assert grads[k] is not None, (k, "no gradient on the device")
        group = "feats" if k == "feats" else k.split(".")[0]
        worst[group] = max(worst.get(group, 0.0), HS.check("%s %s" % (tag, k), grads[k], g64[k], g32[k]))
    print("%s worst error per group in 2^-23 max|g64|: %s" % (tag, {k: round(v, 1) for k, v in worst.items()}))


_FACTORS = {}


def factors(dev, B):
    """pose_U, pose_S, pose_V (detached, on the device) of the spread recipe's head on B feature rows: about one matrix in eight is
    improper."""
    if B not in _FACTORS:
        with torch.no_grad():
            out = outputs(net_of("spread", dev)(None, input_feats=HS.features("spread", B)[0].to(dev)))
        _FACTORS[B] = tuple(out[k].detach().clone() for k in ("pose_U", "pose_S", "pose_V"))
    return _FACTORS[B]


def sample_with_quat(U, S, V, N, **kw):
    """(R, the quaternions the differentiable route saved for its backward)."""
    R = su.pose_matrix_fisher_sampling_torch(U, S, V, N, **kw)
    assert R.grad_fn is not None
    return R, R.grad_fn.saved_tensors[3]


# ---- the route ----
def test_route_factors_require_grad_and_samples_keep_their_bits(dev):
    """Fails without the feature: with the switch on pose_U / pose_V require grad, the sampled rotations carry a grad_fn and equal the
    no_grad call bit for bit on both noise routes and in latency mode; with the switch off everything is as before; out= / seed_dev=
    are refused on the differentiable route."""
    net = copy.deepcopy(net_of("spread", dev, factors=False))
    feats = HS.features("spread", 3)[0].to(dev)
    cot = HS.cotangents(3)
    off_grads, off = device_grads(net, feats, cot)
    off_grads = {k: v.clone() for k, v in off_grads.items()}
    assert not off["pose_U"].requires_grad and not off["pose_V"].requires_grad
    R_off = su.pose_matrix_fisher_sampling_torch(off["pose_U"], off["pose_S"].detach(), off["pose_V"], NS, seed=4)
    assert R_off.grad_fn is None                                   # nothing requires grad: the route of every earlier release
    net.set_differentiable_factors(True)
    for latency in (False, True):
        net.set_latency_mode(latency)
        try:
            with torch.no_grad():
                want = outputs(net(None, input_feats=feats))
            got = outputs(net(None, input_feats=feats.clone().requires_grad_(True)))
        finally:
            net.set_latency_mode(False)
        assert got["pose_U"].requires_grad and got["pose_V"].requires_grad and got["pose_U"].grad_fn is not None
        for k in want:
            assert torch.equal(got[k], want[k]), (k, latency)
        for on_cpu in (False, True):
            torch.manual_seed(31)
            with torch.no_grad():
                R_want = su.pose_matrix_fisher_sampling_torch(got["pose_U"], got["pose_S"], got["pose_V"], NS, sample_on_cpu=on_cpu, seed=9)
            torch.manual_seed(31)
            R_got = su.pose_matrix_fisher_sampling_torch(got["pose_U"], got["pose_S"], got["pose_V"], NS, sample_on_cpu=on_cpu, seed=9)
            assert R_got.grad_fn is not None and R_want.grad_fn is None and torch.equal(R_got, R_want), (latency, on_cpu)
    su.check_sampling()
    with pytest.raises(ValueError):
        su.pose_matrix_fisher_sampling_torch(got["pose_U"], got["pose_S"], got["pose_V"], NS, out=torch.empty(3, NS, 23, 3, 3, device=dev))
    with pytest.raises(ValueError):
        su.pose_matrix_fisher_sampling_torch(got["pose_U"], got["pose_S"], got["pose_V"], NS,
                                             seed_dev=torch.zeros(2, dtype=torch.int64, device=dev))
    # the switch off again: outputs and gradients bit for bit those of before
    net.set_differentiable_factors(False)
    again_grads, again = device_grads(net, feats, cot)
    for k in off:
        assert torch.equal(again[k], off[k]), k
    for k in off_grads:
        assert torch.equal(again_grads[k], off_grads[k]), k


# ---- the sampler's backward alone ----
def sampler_grads(U, S, V, N, g_R, need=(True, True, True), **kw):
    leaves = [t.detach().clone().requires_grad_(n) for t, n in zip((U, S, V), need)]
    R, quat = sample_with_quat(*leaves, N, **kw)
    R.backward(g_R)
    return dict(zip(("pose_U", "pose_S", "pose_V"), [l.grad for l in leaves])), quat, R


@pytest.mark.parametrize("B,N,on_cpu", [(1, 1, False), (3, 8, True), (130, 8, False), (5, 3, False), (1, 40, False), (3, 70, True),
                                        (3, 129, False), (130, 1, False)])
def test_sampler_backward_against_the_pinned_float64_reference(dev, B, N, on_cpu):
    """All three gradients with a random g_R.  N = 1, 3, 8: several calls share a wavefront (64, 16, 8 of them; B = 130 ends in a
    partial wavefront); N = 40: one wavefront per call; N = 70: a lane takes two samples; N = 129: two wavefronts per call (the forward's
    multi-wavefront path too)."""
    U, S, V = factors(dev, B)
    g_R = S2.cot_R(B, N)
    torch.manual_seed(40 + N)
    grads, quat, R = sampler_grads(U, S, V, N, g_R.to(dev), sample_on_cpu=on_cpu, seed=77 + N)
    su.check_sampling()
    assert float((quat.norm(dim=-1) - 1.0).abs().max()) <= 4 * SC.EPS32
    # the saved quaternions are the ones of the rotations: form (b) on them gives R
    with torch.no_grad():
        R64 = S2.sample_pinned(U.cpu().double(), S.cpu().double(), V.cpu().double(), quat.cpu())
    assert float((R.detach().cpu().double() - R64).abs().max()) <= 16 * SC.EPS32
    g64 = S2.factor_vjp(U, S, V, quat, g_R, torch.float64)
    g32 = S2.factor_vjp(U, S, V, quat, g_R, torch.float32)
    for k in g64:
        S2.check("B=%d N=%d %s" % (B, N, k), grads[k], g64[k], g32[k])


def backward_call(U, S, V, quat, g_R, want=(True, True, True)):
    """hps_mf_sample_backward itself on contiguous fp32 device tensors."""
    B, N, nj = quat.shape[:3]
    outs = [torch.full_like(t, float("nan")) if w else None for t, w in zip((U, S, V), want)]
    P = _capi.ptr
    _capi.call("hps_mf_sample_backward", P(U), P(S), P(V), None, None, None, P(quat), P(g_R), B * nj, nj, N, S2.B_ACG, P(outs[0]), P(outs[1]), P(outs[2]),
               _capi.stream())
    return outs


@pytest.mark.parametrize("N", [8, 70, 129])
def test_sum_over_the_samples_equals_single_sample_calls(dev, N):
    """The N-sample launch against N launches of one sample added in float64: the N + 1 results are each rounded to fp32 once, so the
    difference is at most 2^-24 (sum_n |g_n| + |g|) per element."""
    B = 3
    U, S, V = factors(dev, B)
    g_R = S2.cot_R(B, N).to(dev)
    _, quat, _ = sampler_grads(U, S, V, N, g_R, seed=5)
    total = backward_call(U, S, V, quat, g_R)
    acc = [torch.zeros_like(t, dtype=torch.float64) for t in total]
    mag = [t.double().abs() for t in total]
    for n in range(N):
        one = backward_call(U, S, V, quat[:, n:n + 1].contiguous(), g_R[:, n:n + 1].contiguous())
        for a, m, o in zip(acc, mag, one):
            a += o.double()
            m += o.double().abs()
    for name, t, a, m in zip(("g_U", "g_S", "g_V"), total, acc, mag):
        excess = float(((t.double() - a).abs() - 2.0 ** -24 * m).max())
        print("N=%d %s: max|launch - sum of single-sample launches| = %.3e" % (N, name, float((t.double() - a).abs().max())))
        assert excess <= 0.0, (name, excess)


def test_sampler_backward_is_repeatable_independent_of_B_and_skips_unwanted_outputs(dev):
    B, N = 130, 8
    U, S, V = factors(dev, B)
    g_R = S2.cot_R(B, N).to(dev)
    a, quat, _ = sampler_grads(U, S, V, N, g_R, seed=6)
    b, quat_b, _ = sampler_grads(U, S, V, N, g_R, seed=6)
    assert torch.equal(quat, quat_b)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    for i in (0, 67, 129):
        one = backward_call(U[i:i + 1].contiguous(), S[i:i + 1].contiguous(), V[i:i + 1].contiguous(), quat[i:i + 1].contiguous(),
                            g_R[i:i + 1].contiguous())
        for k, o in zip(("pose_U", "pose_S", "pose_V"), one):
            assert torch.equal(o[0], a[k][i]), (k, i)
    # the same for the layout with one workgroup per call
    N2 = 70
    g2 = S2.cot_R(3, N2).to(dev)
    U3, S3, V3 = factors(dev, 3)
    c, quat3, _ = sampler_grads(U3, S3, V3, N2, g2, seed=6)
    one = backward_call(U3[2:3].contiguous(), S3[2:3].contiguous(), V3[2:3].contiguous(), quat3[2:3].contiguous(), g2[2:3].contiguous())
    for k, o in zip(("pose_U", "pose_S", "pose_V"), one):
        assert torch.equal(o[0], c[k][2]), k
    # a cotangent nobody needs is not computed into a tensor: autograd hands back None, the entry point leaves NULL outputs alone
    only_s, _, _ = sampler_grads(U, S, V, N, g_R, need=(False, True, False), seed=6)
    assert only_s["pose_U"] is None and only_s["pose_V"] is None and torch.equal(only_s["pose_S"], a["pose_S"])
    gU, gS, gV = backward_call(U, S, V, quat, g_R, want=(True, False, True))
    assert gS is None and torch.equal(gU, a["pose_U"]) and torch.equal(gV, a["pose_V"])


@pytest.mark.parametrize("N,n_hot", [(8, 5), (70, 69), (129, 64)])
def test_cotangent_on_one_sample_only(dev, N, n_hot):
    """g_R zero except on sample n_hot of image 1: the launch gives that sample's single-sample result bit for bit (exact zeros are
    added), and zero for the other images."""
    B = 3
    U, S, V = factors(dev, B)
    g_R = torch.zeros(B, N, 23, 3, 3, device=dev)
    g_R[1, n_hot] = S2.cot_R(B, N)[1, n_hot].to(dev)
    _, quat, _ = sampler_grads(U, S, V, N, g_R, seed=8)
    full = backward_call(U, S, V, quat, g_R)
    one = backward_call(U, S, V, quat[:, n_hot:n_hot + 1].contiguous(), g_R[:, n_hot:n_hot + 1].contiguous())
    for f, o in zip(full, one):
        assert torch.equal(f, o)
        assert float(f[0].abs().max()) == 0.0 and float(f[2].abs().max()) == 0.0 and float(f[1].abs().max()) > 0.0


def test_nan_rotations_of_a_failed_call_give_nan_gradients(dev):
    """Non-finite concentrations: the forward's calls fail (NaN rotations, check_sampling raises), the backward's gradients of those
    calls are NaN and the other calls' are finite."""
    U, S, V = (t.clone() for t in factors(dev, 3))
    S[1, 4] = float("nan")
    g_R = S2.cot_R(3, NS).to(dev)
    grads, quat, R = sampler_grads(U, S, V, NS, g_R, seed=3)
    with pytest.raises(_capi.HpsError):
        su.check_sampling()
    assert bool(torch.isnan(R[1, :, 4]).all()) and bool(torch.isnan(quat[1, :, 4]).all())
    for k in grads:
        assert bool(torch.isnan(grads[k][1, 4]).all()), k
        rest = grads[k].clone()
        rest[1, 4] = 0.0
        assert bool(torch.isfinite(rest).all()), k


# ---- the head with cotangents on the raw factors ----
@pytest.mark.parametrize("recipe,B,which", [("spread", 1, "factors"), ("spread", 3, "factors"), ("spread", 130, "all"), ("spread", 3, "all"),
                                            ("default", 3, "all"), ("default", 3, "factors")])
def test_head_gradients_with_cotangents_on_the_raw_factors(dev, recipe, B, which):
    """Standard-normal cotangents on pose_U / pose_V alone ("factors") and together with the seven other outputs ("all"); B = 130
    crosses the batch tiles of the level kernels and ends in a partial tile."""
    net = net_of(recipe, dev)
    feats = HS.features(recipe, B)[0]
    cot = dict(S2.cot_factors(B))
    if which == "all":
        cot.update(HS.cotangents(B))
    grads, out = device_grads(net, feats.to(dev), cot)
    g64, g32 = HS.reference(("stage2", recipe, B, which), HS.state(recipe), feats, out["pose_U"], cot)
    assert all(grads[k] is not None for k in g64)
    check_all("%s B=%d %s" % (recipe, B, which), grads, g64, g32)


def test_head_factor_cotangents_in_host_svd_mode_and_with_frozen_leaves(dev):
    B = 3
    feats = HS.features("spread", B)[0]
    cot = dict(S2.cot_factors(B), **HS.cotangents(B))
    net = copy.deepcopy(net_of("spread", dev))
    net.svd_mode = "host"
    grads, out = device_grads(net, feats.to(dev), cot)
    g64, g32 = HS.reference(("stage2", "spread", B, "all", "host"), HS.state("spread"), feats, out["pose_U"], cot)
    check_all("host SVD", grads, g64, g32)
    net.svd_mode = "device"
    for p in net.parameters():
        p.requires_grad_(False)
    grads, out = device_grads(net, feats.to(dev), cot)
    g64, g32 = HS.reference(("stage2", "spread", B, "all"), HS.state("spread"), feats, out["pose_U"], cot)
    assert all(v is None for k, v in grads.items() if k != "feats")
    HS.check("frozen parameters: feats", grads["feats"], g64["feats"], g32["feats"])
    for p in net.parameters():
        p.requires_grad_(True)
    grads, _ = device_grads(net, feats.to(dev), cot, feats_grad=False)
    assert grads.pop("feats") is None
    check_all("frozen features", grads, g64, g32)


@pytest.mark.parametrize("recipe,B,N,seed,fseed", S2.CASES)
def test_sampler_through_the_head(dev, recipe, B, N, seed, fseed):
    """features -> head -> sampler with a random cotangent on R, the host-noise cases whose conditions tests/test_stage2_host.py
    asserts: every head-parameter gradient and the feature gradient against form (b) on the device's quaternions."""
    net = net_of(recipe, dev)
    feats = HS.features(recipe, B, fseed)[0]
    g_R = S2.cot_R(B, N)
    net.zero_grad(set_to_none=True)
    f = feats.to(dev).requires_grad_(True)
    out = outputs(net(None, input_feats=f))
    torch.manual_seed(seed)
    R, quat = sample_with_quat(out["pose_U"], out["pose_S"], out["pose_V"], N, sample_on_cpu=True)
    # the device took the accept decisions of the float64 restatement on the same noise (fp32 quaternions of the same proposals)
    assert float((quat.cpu().double() - S2.host_case(recipe, B, N, seed, fseed)["q64"]).abs().max()) <= 64 * SC.EPS32
    calls, real = [], _capi.call
    _capi.call = lambda name, *args: (calls.append(name), real(name, *args))[1]
    try:
        R.backward(g_R.to(dev))
    finally:
        _capi.call = real
    # the sampler's backward differentiates at the float64 factors of the head's float64 pass, which the head's backward then reuses
    assert calls.count("hps_head_forward_refine") == 1 and calls.index("hps_head_forward_refine") < calls.index("hps_mf_sample_backward")
    grads = {k: p.grad for k, p in net.named_parameters() if k.startswith(HS.HEAD_PREFIXES)}
    grads["feats"] = f.grad
    loss_fn = S2.sampler_loss("b", g_R, q=quat)
    g64 = S2.head_vjp(HS.state(recipe), feats, out["pose_U"], torch.float64, loss_fn)
    g32 = S2.head_vjp(HS.state(recipe), feats, out["pose_U"], torch.float32, loss_fn)
    check_all("%s B=%d N=%d" % (recipe, B, N), grads, g64, g32)


# ---- the stage-2 chain ----
def stage2_targets(B, dev="cpu"):
    g = torch.Generator().manual_seed(21)
    vis = torch.rand(B, 17, generator=g) < 0.75
    return {"pose_params_rotmats": HS.rot6d(torch.randn(B * 23, 6, generator=g)).view(B, 23, 3, 3).to(dev),
            "shape_params": torch.randn(B, 10, generator=g).to(dev),
            "joints2D": (torch.rand(B, 17, 2, generator=g) * 256).to(dev),
            "joints2D_vis": vis.to(dev),
            "glob_rotmats": HS.rot6d(torch.randn(B, 6, generator=g)).to(dev),
            "verts": (torch.randn(B, 6890, 3, generator=g) * 0.3).to(dev), "joints3D": (torch.randn(B, 14, 3, generator=g) * 0.3).to(dev)}


def stage2_loss(net, smpl, out, target, criterion, on_cpu, seed, shape_seed, pin_shape_noise=True):
    """The reference's stage-2 step (:262-346) on the device from the head's outputs.  Returns the loss and what the test pins the
    reference on: the saved quaternions and the shape noise (None with pin_shape_noise=False: no second draw, no comparison on the
    host -- tests/dev/stage2_step_time.py)."""
    from torch.distributions import Normal
    dev, B = out["pose_F"].device, out["pose_F"].shape[0]
    glob_rotmats = rtu.rot6d_to_rotmat(out["glob"])
    mode_out = smpl(body_pose=out["mode"], global_orient=glob_rotmats.unsqueeze(1), betas=out["loc"], pose2rot=False)
    project = lambda joints, cam: cam_utils.orthographic_project_torch(cam_utils.flip_about_x(joints[:, ALL_JOINTS_TO_COCO_MAP]), cam)
    j2d_mode = project(mode_out.joints, out["cam"])
    torch.manual_seed(seed)
    R, quat = sample_with_quat(out["pose_U"], out["pose_S"], out["pose_V"], NS, sample_on_cpu=on_cpu, seed=seed)
    dist = Normal(out["loc"], out["scale"], validate_args=False)
    shape_eps = None
    if pin_shape_noise:
        torch.cuda.manual_seed(shape_seed)
        shape_eps = torch.empty(NS, B, 10, device=dev).normal_()      # the draw Normal.rsample makes: the same numbers after the same seed
        torch.cuda.manual_seed(shape_seed)
    betas = dist.rsample([NS])
    if pin_shape_noise:
        assert torch.equal(betas.detach(), out["loc"].detach() + shape_eps * out["scale"].detach()), "the test's pin of the shape noise"
    betas = betas.transpose(0, 1)                                     # (B, NS, 10)
    joints = smpl(body_pose=R.reshape(-1, 23, 3, 3), global_orient=glob_rotmats[:, None].expand(-1, NS, -1, -1).reshape(-1, 1, 3, 3),
                  betas=betas.reshape(-1, 10), pose2rot=False).joints
    j2d_samples = project(joints, out["cam"][:, None].expand(-1, NS, -1).reshape(-1, 3)).reshape(B, NS, 17, 2)
    pred = {"pose_params_F": out["pose_F"], "pose_params_U": out["pose_U"], "pose_params_S": out["pose_S"],
            "pose_params_V": out["pose_V"], "shape_params": dist, "joints2D": torch.cat([j2d_mode[:, None], j2d_samples], dim=1),
            "glob_rotmats": glob_rotmats, "verts": mode_out.vertices, "joints3D": mode_out.joints[:, J14]}
    return criterion(target, pred), quat, shape_eps


def stage2_reference_loss(out, target, cfg, quat, shape_eps, c_F, c_S):
    """The same chain in torch in the dtype of ``out`` (HS.head's dict): rot6d, SMPL (oracle.ref_cpu.smpl_forward), sampler form (b) on
    the device's quaternions, the flip and the projection, and the loss restated term by term (losses/matrix_fisher_loss.py:265-299,
    REDUCTION 'mean') -- except the pose NLL, for which no torch restatement exists (its normalising constant; the device kernel has
    its own float64 tests, tests/test_gpu_mf_loss.py): its cotangents on pose_F / pose_S, taken from the device function on detached
    leaves, enter as the linear term <c_F, pose_F> + <c_S, pose_S>."""
    dtype = out["pose_F"].dtype
    B = out["pose_F"].shape[0]
    T = lambda k: target[k].cpu().to(dtype)
    w = cfg.WEIGHTS
    glob_rotmats = HS.rot6d(out["glob"])
    params = SC.params(dtype)
    mode_out = SC.O.smpl_forward(params, betas=out["loc"], body_pose=out["mode"], global_orient=glob_rotmats.unsqueeze(1), pose2rot=False)
    flip = torch.tensor([1.0, -1.0, -1.0], dtype=dtype)
    project = lambda joints, cam: cam[:, None, 0:1] * ((joints[:, ALL_JOINTS_TO_COCO_MAP] * flip)[:, :, :2] + cam[:, None, 1:])
    j2d_mode = project(mode_out["joints"], out["cam"])
    R = S2.sample_pinned(out["pose_U"], out["pose_S"], out["pose_V"], quat.cpu())
    betas = (out["loc"] + shape_eps.cpu().to(dtype) * out["scale"]).transpose(0, 1)
    s_out = SC.O.smpl_forward(params, betas=betas.reshape(-1, 10), body_pose=R.reshape(-1, 23, 3, 3),
                              global_orient=glob_rotmats[:, None].expand(-1, NS, -1, -1).reshape(-1, 1, 3, 3), pose2rot=False)
    j2d_samples = project(s_out["joints"], out["cam"][:, None].expand(-1, NS, -1).reshape(-1, 3)).reshape(B, NS, 17, 2)
    j2d = torch.cat([j2d_mode[:, None], j2d_samples], dim=1)
    vis = target["joints2D_vis"].cpu()[:, None, :].expand(-1, NS + 1, -1)
    t_j2d = (2.0 * T("joints2D") / 256.0 - 1.0)[:, None].expand(-1, NS + 1, -1, -1)
    mse = lambda a, b: ((a - b) ** 2).mean()
    shape_nll = -torch.distributions.Normal(out["loc"], out["scale"], validate_args=False).log_prob(T("shape_params")).sum(dim=1).mean()
    return ((c_F.cpu().to(dtype) * out["pose_F"]).sum() + (c_S.cpu().to(dtype) * out["pose_S"]).sum()
            + w.SHAPE * shape_nll + w.JOINTS2D * mse(j2d[vis], t_j2d[vis]) + w.GLOB_ROTMATS * mse(glob_rotmats, T("glob_rotmats"))
            + w.VERTS3D * mse(mode_out["vertices"], T("verts")) + w.JOINTS3D * mse(mode_out["joints"][:, J14], T("joints3D")))


@pytest.mark.parametrize("on_cpu", [True, False], ids=["host_noise", "philox"])
def test_stage2_chain_against_float64_autograd(dev, smpl_gpu, on_cpu):
    """features -> head -> rot6d_to_rotmat -> mode mesh and 8 sample meshes (joints only) through SMPL, rsample for the shapes, flip,
    orthographic_project_torch, PoseMFShapeGaussianLoss with the reference's STAGE2 weights on 'means+samples': every head-parameter
    gradient and the feature gradient against float64 autograd of stage2_reference_loss."""
    net, B = net_of("spread", dev), 3
    feats = HS.features("spread", B)[0]
    cfg = configs.get_cfg_defaults().LOSS.STAGE2
    criterion = PoseMFShapeGaussianLoss(loss_config=cfg, img_wh=256)
    target = stage2_targets(B, dev)
    net.zero_grad(set_to_none=True)
    f = feats.to(dev).requires_grad_(True)
    out = outputs(net(None, input_feats=f))
    loss, quat, shape_eps = stage2_loss(net, smpl_gpu, out, target, criterion, on_cpu, 17, 23)
    loss.backward()
    su.check_sampling()
    grads = {k: p.grad for k, p in net.named_parameters() if k.startswith(HS.HEAD_PREFIXES)}
    grads["feats"] = f.grad
    assert all(v is not None and bool(torch.isfinite(v).all()) for v in grads.values())
    # the pose term's cotangents from the device function on detached leaves (weight x mean over the B x 23 rows)
    F_leaf, S_leaf = out["pose_F"].detach().clone().requires_grad_(True), out["pose_S"].detach().clone().requires_grad_(True)
    (cfg.WEIGHTS.POSE * matrix_fisher_nll(F_leaf, out["pose_U"].detach(), S_leaf, out["pose_V"].detach(), target["pose_params_rotmats"],
                                          overreg=cfg.MF_OVERREG).mean()).backward()
    loss_fn = lambda o: stage2_reference_loss(o, target, cfg, quat, shape_eps, F_leaf.grad, S_leaf.grad)
    g64 = S2.head_vjp(HS.state("spread"), feats, out["pose_U"], torch.float64, loss_fn)
    g32 = S2.head_vjp(HS.state("spread"), feats, out["pose_U"], torch.float32, loss_fn)
    check_all("stage-2 chain %s" % ("host noise" if on_cpu else "philox"), grads, g64, g32)


def test_stage2_training_step_from_an_image_batch(dev, smpl_gpu):
    """set_batchnorm_training(True) / .train() and the switch on, from a (3, 18, 64, 64) batch: every encoder and head parameter gets a
    finite, non-zero gradient; after an SGD step a second forward + backward runs on the stepped weights."""
    import encoder_grad_scenario as ES
    net = HS.make_net("spread")
    ES.randomize_bn(net.image_encoder)
    net = net.to(dev)
    net.set_differentiable_factors(True)
    net.set_batchnorm_training(True)
    net.train()
    x = ES.case("sq64")[0].to(dev)
    B = x.shape[0]
    criterion = PoseMFShapeGaussianLoss(loss_config=configs.get_cfg_defaults().LOSS.STAGE2, img_wh=256)
    target = stage2_targets(B, dev)
    opt = torch.optim.SGD(net.parameters(), lr=1e-6)
    losses = []
    for step in range(2):
        net.zero_grad(set_to_none=True)
        out = outputs(net(x))
        loss, _, _ = stage2_loss(net, smpl_gpu, out, target, criterion, False, 17 + step, 23 + step)
        loss.backward()
        assert bool(torch.isfinite(loss))
        for k, p in net.named_parameters():
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0.0, (step, k)
        if step == 0:
            before = {k: p.detach().clone() for k, p in net.named_parameters()}
            opt.step()
            assert all(not torch.equal(p, before[k]) for k, p in net.named_parameters())
            fresh = HS.make_net("spread").to(dev)
            fresh.load_state_dict(net.state_dict())
            fresh.set_batchnorm_training(True)
            fresh.train()
            with torch.no_grad():
                want, got = outputs(fresh(x)), outputs(net(x))         # the stale-copy detection saw the step
            for k in want:
                assert torch.equal(want[k], got[k]), k
        losses.append(float(loss.detach()))
    su.check_sampling()
    print("stage-2 loss of the two steps: %s" % losses)
