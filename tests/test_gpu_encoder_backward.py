"""GPU: ResNet.forward under autograd (csrc/conv_backward.hip) against the pinned float64 reference of encoder_grad_scenario, by the
project's accuracy rule (smpl_grad_scenario.bound / check): per tensor max|g_dev - g64| <= 4 max(max|g32 - g64|, 2^-23 max|g64|), the
masks and pool winners of both references pinned to the device's own run (ResNet.activations)."""
import copy

import pytest
import torch
import torch.nn.functional as F

import encoder_grad_scenario as ES
from hierarchicalprobabilistic3dhuman_amd import _capi

pytestmark = pytest.mark.gpu

_ENCODERS = {}
MODES = ("default", "no_winograd", "latency")


def encoder_of(in_channels, dev):
    """The recipe's encoder on the device, shared by the tests (they restore every switch they touch and never step its parameters)."""
    if in_channels not in _ENCODERS:
        _ENCODERS[in_channels] = ES.make_encoder(in_channels).to(dev)
    return _ENCODERS[in_channels]


class mode_of:
    def __init__(self, enc, mode):
        self.enc, self.mode = enc, mode

    def __enter__(self):
        if self.mode == "no_winograd":
            self.enc.set_winograd(False)
        elif self.mode == "latency":
            self.enc.set_latency_mode(True)

    def __exit__(self, *exc):
        self.enc.set_winograd(True)
        self.enc.set_latency_mode(False)


def device_grads(enc, x, cot, input_grad=True):
    """(gradients dict over "input" and the parameter names, features) of <cot, features> on the device."""
    enc.zero_grad(set_to_none=True)
    xd = x.detach().clone().requires_grad_(input_grad)
    feats = enc(xd)
    (cot.to(xd.device) * feats).sum().backward()
    grads = {k: p.grad for k, p in enc.named_parameters()}
    grads["input"] = xd.grad
    return grads, feats.detach()


def check_all(tag, grads, g64, g32, keys=None):
    worst = 0.0
    for k in (keys or g64):
        assert grads[k] is not None, (k, "no gradient on the device")
        worst = max(worst, ES.check("%s %s" % (tag, k), grads[k], g64[k], g32[k]))
    print("%s worst error in 2^-23 max|g64|: %.2f" % (tag, worst))


# ---- per kernel, on the test's own frames ----
def frame(t_nchw, pad, channels=None):
    """(B, H + 2 pad, W + 2 pad, C') zero frame with the NCHW tensor in its interior."""
    B, C, H, W = t_nchw.shape
    f = torch.zeros(B, H + 2 * pad, W + 2 * pad, channels or C, device=t_nchw.device, dtype=torch.float32)
    f[:, pad:pad + H, pad:pad + W, :C] = t_nchw.permute(0, 2, 3, 1)
    return f


WGRAD_LAYERS = [(18, 64, 7, 2), (64, 64, 3, 1), (64, 128, 3, 2), (64, 128, 1, 2), (256, 512, 3, 2), (512, 512, 3, 1)]


def wgrad_inputs(cin, cout, k, stride):
    """(B, H, W) per layer: one output pixel; 5 x (5 x 7) = 175 pixels = one slice of 128 and a part of one; and for the two small
    layers 2 x (24 x 24) = 1152 pixels = two slices of 512 and a part of one."""
    one = (1, 1, 1)
    odd = (5, 5, 7) if stride == 1 else (5, 10, 14) if k != 7 else (5, 9, 13)
    big = [(2, 24, 24) if stride == 1 else (2, 48, 48)] if cin <= 64 and cout <= 64 else []
    return [one, odd] + big


@pytest.mark.parametrize("cin,cout,k,stride", WGRAD_LAYERS)
def test_weight_gradient_kernel(dev, cin, cout, k, stride):
    pad, lib = (k // 2 if k > 1 else 0), _capi.load()
    ipad = max(pad, 1)
    gen = torch.Generator().manual_seed(cin + cout + k)
    for B, H, W in wgrad_inputs(cin, cout, k, stride):
        Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
        x, g = torch.randn(B, cin, H, W, generator=gen), torch.randn(B, cout, Ho, Wo, generator=gen)
        S = lib.hps_conv_wgrad_slice_pixels(Ho, Wo)
        if (B, H, W) != (1, 1, 1):
            assert (B * Ho * Wo) % S != 0 and B * Ho * Wo > S               # a partial last slice
        ref = {}
        for dt in (torch.float64, torch.float32):
            patches = F.unfold(x.to(dt), k, padding=pad, stride=stride)                         # (B, cin k k, Ho Wo)
            G = torch.einsum("bol,bkl->ok", g.to(dt).flatten(2), patches).view(cout, cin, k, k)
            ref[dt] = G.permute(0, 2, 3, 1).double()                                            # the kernel's (Cout, KH, KW, Cin)
        cx = cin + 2 if cin == 18 else cin                                   # a frame with more channels per pixel than the filter reads
        xf, gf = frame(x.to(dev), ipad, cx), frame(g.to(dev), 1)
        out = torch.full((cout, k, k, cin), float("nan"), device=dev)
        ws = torch.empty(lib.hps_conv_wgrad_workspace(B, H, W, cin, cout, k, k, stride, pad) // 4, device=dev)
        _capi.call("hps_conv_wgrad", _capi.ptr(xf), _capi.ptr(gf), _capi.ptr(out), _capi.ptr(ws), B, H, W, ipad, cx, cin, cout, k, k,
                   stride, pad, 1, _capi.stream())
        ES.check("wgrad %s B=%d %dx%d" % ((cin, cout, k, stride), B, H, W), out, ref[torch.float64], ref[torch.float32])
        again = torch.empty_like(out)
        _capi.call("hps_conv_wgrad", _capi.ptr(xf), _capi.ptr(gf), _capi.ptr(again), _capi.ptr(ws), B, H, W, ipad, cx, cin, cout, k, k,
                   stride, pad, 1, _capi.stream())
        assert torch.equal(out, again)


@pytest.mark.parametrize("cin,cout,k,stride,B,H,W", [(64, 128, 3, 2, 3, 10, 14), (64, 128, 3, 2, 2, 9, 13), (64, 128, 1, 2, 3, 9, 14),
                                                      (18, 64, 7, 2, 2, 18, 22), (64, 64, 3, 1, 2, 5, 7), (512, 512, 3, 1, 5, 1, 1),
                                                      (256, 512, 3, 2, 1, 3, 4)])
def test_data_gradient_kernel(dev, cin, cout, k, stride, B, H, W):
    """With and without the accumulated branch, against float64 conv_transpose (torch.nn.grad.conv2d_input)."""
    pad = k // 2 if k > 1 else 0
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    gen = torch.Generator().manual_seed(cin + cout + k + H)
    g, w = torch.randn(B, cout, Ho, Wo, generator=gen), torch.randn(cout, cin, k, k, generator=gen) / (cout * k * k) ** 0.5
    other = torch.randn(B, cin, H, W, generator=gen)
    ref = {dt: torch.nn.grad.conv2d_input((B, cin, H, W), w.to(dt), g.to(dt), stride=stride, padding=pad).double()
           for dt in (torch.float64, torch.float32)}
    wt = w.permute(2, 3, 0, 1).contiguous().to(dev)
    gf = frame(g.to(dev), 1)
    for with_other in (False, True):
        dx = torch.zeros(B, H + 2, W + 2, cin, device=dev)
        of = frame(other.to(dev), 1) if with_other else None
        _capi.call("hps_conv_dgrad", _capi.ptr(gf), _capi.ptr(wt), _capi.ptr(of), _capi.ptr(dx), B, H, W, cin, cout, k, k, stride, pad, 1, 1,
                   cin, _capi.stream())
        got = dx[:, 1:-1, 1:-1].permute(0, 3, 1, 2)
        add = other.double() if with_other else 0.0
        add32 = (ref[torch.float32].float() + other).double() if with_other else ref[torch.float32]
        ES.check("dgrad %s %dx%dx%d other=%d" % ((cin, cout, k, stride), B, H, W, with_other), got, ref[torch.float64] + add, add32)
        halo = dx.clone()
        halo[:, 1:-1, 1:-1] = 0
        assert float(halo.abs().max()) == 0.0                               # only the interior is written


def test_relu_gate_and_channel_sums(dev):
    lib = _capi.load()
    gen = torch.Generator().manual_seed(9)
    for B, H, W, C, gpad, ypad in [(3, 5, 7, 64, 1, 1), (2, 9, 4, 128, 1, 1), (1, 1, 1, 512, 1, 1), (2, 16, 24, 64, 0, 0)]:
        g, y = torch.randn(B, C, H, W, generator=gen), torch.randn(B, C, H, W, generator=gen)
        y[:, :, ::2, ::3] = 0.0                                             # exact zeros and negative zeros are closed gates
        y[:, :, 0, 0] = -0.0
        gf, yf = frame(g.to(dev), gpad), frame(y.to(dev), ypad)
        sums = torch.empty(C, device=dev)
        ws = torch.empty(lib.hps_relu_gate_workspace(B, H, W, C) // 8, device=dev, dtype=torch.float64)
        _capi.call("hps_relu_gate_pad", _capi.ptr(gf), _capi.ptr(yf), _capi.ptr(ws, torch.float64), _capi.ptr(sums), B, H, W, C, gpad, ypad,
                   _capi.stream())
        want = torch.where(y > 0, g, torch.zeros_like(g))
        assert torch.equal(gf.cpu(), frame(want, gpad))
        ref = want.double().sum((0, 2, 3))
        err = float((sums.cpu().double() - ref).abs().max())
        print("gate %s: max|sums - f64| = %.3e, max|ref| = %.3e" % ((B, H, W, C), err, float(ref.abs().max())))
        assert err <= 2.0 ** -24 * float(ref.abs().max()) * 1.001           # a float64 sum rounded once
        # without sums: the same gate, no workspace
        gf2 = frame(g.to(dev), gpad)
        _capi.call("hps_relu_gate_pad", _capi.ptr(gf2), _capi.ptr(yf), None, None, B, H, W, C, gpad, ypad, _capi.stream())
        assert torch.equal(gf2, gf)


def test_pool_backwards(dev):
    """Max pool: small-integer data (ties everywhere, whole windows of zeros, exact sums) against torch's CPU autograd, which sends a
    window's cotangent to its first maximum; average pool: g / (h w)."""
    gen = torch.Generator().manual_seed(4)
    for B, H, W, C in [(2, 8, 8, 64), (1, 5, 7, 64), (3, 16, 12, 64), (1, 1, 1, 64)]:
        x = torch.randint(0, 3, (B, C, H, W), generator=gen).float()
        x[:, :, : (H + 1) // 2] *= (torch.rand(B, C, 1, 1, generator=gen) > 0.5).float()       # all-zero windows in half the planes
        x64 = x.double().requires_grad_(True)
        pooled = F.max_pool2d(x64, 3, 2, 1)
        g = torch.randint(-4, 5, pooled.shape, generator=gen).float()
        pooled.backward(g.double())
        dx = torch.full((B, H, W, C), float("nan"), device=dev)
        xd, gf = x.permute(0, 2, 3, 1).contiguous().to(dev), frame(g.to(dev), 1)
        _capi.call("hps_maxpool3x3s2_backward", _capi.ptr(xd), _capi.ptr(gf), _capi.ptr(dx), B, H, W, C, 1, _capi.stream())
        assert torch.equal(dx.cpu().permute(0, 3, 1, 2).double(), x64.grad), (B, H, W)
    for B, h, w, C in [(3, 2, 2, 512), (2, 3, 4, 512), (5, 1, 1, 512)]:
        gfeat = torch.randn(B, C, generator=gen).to(dev)
        gfr = torch.zeros(B, h + 2, w + 2, C, device=dev)
        _capi.call("hps_global_avgpool_backward", _capi.ptr(gfeat), _capi.ptr(gfr), B, h, w, C, 1, _capi.stream())
        want = (gfeat.cpu() / float(h * w))[:, :, None, None].expand(B, C, h, w)               # the IEEE quotient (host division)
        assert torch.equal(gfr.cpu(), frame(want, 1))


# ---- the whole encoder ----
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(ES.CASES))
def test_all_gradients_against_the_pinned_float64_reference(dev, name, mode):
    """Gradient of the input, every convolution weight, every BatchNorm weight and bias; the differentiable forward's features and
    activations()'s features equal the no_grad forward's bit for bit."""
    cin, _ = ES.CASES[name]
    enc = encoder_of(cin, dev)
    x, cot = ES.case(name)
    with mode_of(enc, mode):
        with torch.no_grad():
            plain = enc(x.to(dev))
        assert plain.grad_fn is None
        grads, feats = device_grads(enc, x.to(dev), cot)
        act_feats, maps = enc.activations(x.to(dev))
        with torch.no_grad():
            after = enc(x.to(dev))
    assert torch.equal(feats, plain) and torch.equal(act_feats, plain) and torch.equal(after, plain)
    pins = ES.pins_from_maps(maps)
    print("%s %s: %d mask / winner flips against the fp32 CPU restatement" % (name, mode, ES.flips(pins, ES.self_pins(name))))
    g64, g32 = ES.reference((name, mode), ES.state(cin), x, pins, cot)
    assert set(g64) == set(grads)
    check_all("%s %s" % (name, mode), grads, g64, g32)


def test_route_and_frozen_variants(dev):
    """Fails without the feature: features carry a grad_fn.  A frozen encoder with an input gradient, a frozen input, and a net whose
    layer1 is frozen: what is asked for meets the rule, what is not asked for stays None."""
    name = "odd"
    enc = copy.deepcopy(encoder_of(18, dev))
    x, cot = ES.case(name)
    assert enc(x.to(dev)).grad_fn is not None
    with torch.no_grad():
        assert enc(x.to(dev)).grad_fn is None
    pins = ES.pins_from_maps(enc.activations(x.to(dev))[1])
    g64, g32 = ES.reference((name, "default"), ES.state(18), x, pins, cot)
    # frozen input
    grads, _ = device_grads(enc, x.to(dev), cot, input_grad=False)
    assert grads["input"] is None
    check_all("frozen input", grads, g64, g32, [k for k in g64 if k != "input"])
    # layer1 frozen
    enc.layer1.requires_grad_(False)
    grads, _ = device_grads(enc, x.to(dev), cot)
    frozen = [k for k in g64 if k.startswith("layer1.")]
    assert frozen and all(grads[k] is None for k in frozen)
    check_all("layer1 frozen", grads, g64, g32, [k for k in g64 if k not in frozen])
    # only layer3 and up wants a gradient: nothing below it is computed
    enc.requires_grad_(False)
    enc.layer3.requires_grad_(True)
    enc.layer4.requires_grad_(True)
    grads, _ = device_grads(enc, x.to(dev), cot, input_grad=False)
    upper = [k for k in g64 if k.startswith(("layer3.", "layer4."))]
    assert all(grads[k] is None for k in g64 if k not in upper)
    check_all("layer3-4 only", grads, g64, g32, upper)
    # frozen encoder, input gradient
    enc.requires_grad_(False)
    grads, feats = device_grads(enc, x.to(dev), cot)
    assert all(grads[k] is None for k in g64 if k != "input")
    check_all("frozen encoder", grads, g64, g32, ["input"])
    # all frozen: the plain route
    assert enc(x.to(dev)).grad_fn is None


def test_two_forwards_then_two_backwards_and_repeatability(dev):
    """The backward recomputes into frames of its own: a second forward between a forward and its backward changes nothing, bit for
    bit; the same call twice gives the same bits."""
    enc = encoder_of(18, dev)
    xa, cot = ES.case("sq64")
    xb = torch.rand(xa.shape, generator=torch.Generator().manual_seed(77))
    single_a, _ = device_grads(enc, xa.to(dev), cot)
    single_a = {k: v.clone() for k, v in single_a.items()}
    again, _ = device_grads(enc, xa.to(dev), cot)
    for k in single_a:
        assert torch.equal(single_a[k], again[k]), k
    single_b, _ = device_grads(enc, xb.to(dev), cot)
    single_b = {k: v.clone() for k, v in single_b.items()}
    enc.zero_grad(set_to_none=True)
    a, b = xa.to(dev).requires_grad_(True), xb.to(dev).requires_grad_(True)
    fa, fb = enc(a), enc(b)
    params = list(enc.parameters())
    c = cot.to(dev)
    ga = torch.autograd.grad((c * fa).sum(), [a] + params)
    gb = torch.autograd.grad((c * fb).sum(), [b] + params)
    names = ["input"] + [k for k, _ in enc.named_parameters()]
    for k, va, vb in zip(names, ga, gb):
        assert torch.equal(va, single_a[k]) and torch.equal(vb, single_b[k]), k


def test_input_gradient_of_an_image_does_not_depend_on_the_batch(dev):
    enc = encoder_of(18, dev)
    x, cot = ES.case("sq64")
    g3, _ = device_grads(enc, x.to(dev), cot)
    g3 = g3["input"].clone()
    for i in range(x.shape[0]):
        g1, _ = device_grads(enc, x[i:i + 1].to(dev), cot[i:i + 1])
        assert torch.equal(g1["input"][0], g3[i]), i


def test_training_mode_is_still_refused(dev):
    enc = copy.deepcopy(encoder_of(18, dev))
    enc.train()
    with pytest.raises(RuntimeError):
        enc(ES.case("tiny32")[0].to(dev))
    with pytest.raises(RuntimeError):
        enc.activations(ES.case("tiny32")[0].to(dev))


# ---- the chain: loss -> SMPL / rot6d -> head -> encoder ----
def chain_net(dev):
    import head_grad_scenario as HS
    net = HS.make_net("spread")
    ES.randomize_bn(net.image_encoder)
    return net.to(dev)


def chain_loss(net, smpl_gpu, x):
    from torch.distributions import Normal
    from hierarchicalprobabilistic3dhuman_amd import configs, rigid_transform_utils as rtu
    from hierarchicalprobabilistic3dhuman_amd.matrix_fisher_loss import PoseMFShapeGaussianLoss
    dev, B = x.device, x.shape[0]
    pose_F, pose_U, pose_S, pose_V, mode, shape_dist, glob, cam = net(x)
    glob_rotmats = rtu.rot6d_to_rotmat(glob)
    smpl_out = smpl_gpu(body_pose=mode, global_orient=glob_rotmats.unsqueeze(1), betas=shape_dist.loc, pose2rot=False)
    g = torch.Generator().manual_seed(21)
    target = {"pose_params_rotmats": rtu.batch_rodrigues((torch.randn(B * 23, 3, generator=g) * 0.3).to(dev)).view(B, 23, 3, 3),
              "shape_params": torch.randn(B, 10, generator=g).to(dev),
              "joints2D": (torch.rand(B, 17, 2, generator=g) * 256).to(dev),
              "joints2D_vis": torch.ones(B, 17, dtype=torch.bool, device=dev),
              "glob_rotmats": rtu.batch_rodrigues((torch.randn(B, 3, generator=g) * 0.3).to(dev)),
              "verts": torch.randn(B, 6890, 3, generator=g).to(dev), "joints3D": torch.randn(B, 14, 3, generator=g).to(dev)}
    joints2D = (smpl_out.joints[:, :17, :2] * cam[:, None, :1] + cam[:, None, 1:]).unsqueeze(1)
    pred = {"pose_params_F": pose_F, "pose_params_U": pose_U, "pose_params_S": pose_S, "pose_params_V": pose_V,
            "shape_params": Normal(shape_dist.loc, shape_dist.scale, validate_args=False), "joints2D": joints2D,
            "glob_rotmats": glob_rotmats, "verts": smpl_out.vertices, "joints3D": smpl_out.joints[:, :14]}
    return PoseMFShapeGaussianLoss(loss_config=configs.get_cfg_defaults().LOSS.STAGE1, img_wh=256)(target, pred)


def test_loss_chain_reaches_the_encoder_and_stepped_weights_are_not_stale(dev, smpl_gpu):
    """Fails without the feature (the encoder's .grad stayed None): PoseMFShapeGaussianLoss -> SMPL / rot6d -> head -> encoder from an
    image batch.  The encoder's gradients meet the rule against the reference VJP fed with the feature cotangent the device chain
    produced.  After one SGD step on all parameters the next forward equals a freshly built net with the stepped weights."""
    net = chain_net(dev)
    x, _ = ES.case("sq64")
    kept = []

    def keep_features(module, args, output):
        output.retain_grad()
        kept.append(output)

    hook = net.image_encoder.register_forward_hook(keep_features)
    opt = torch.optim.SGD(net.parameters(), lr=1e-6)
    net.zero_grad(set_to_none=True)
    xd = x.to(dev).requires_grad_(True)
    loss = chain_loss(net, smpl_gpu, xd)
    loss.backward()
    hook.remove()
    feats = kept[0]
    assert feats.grad is not None and bool(torch.isfinite(feats.grad).all())
    enc = net.image_encoder
    assert enc.conv1.weight.grad is not None and enc.layer4[1].bn2.bias.grad is not None
    sd = {k: v.detach().cpu().clone() for k, v in enc.state_dict().items()}
    pins = ES.pins_from_maps(enc.activations(x.to(dev))[1])
    g64, g32 = ES.reference(("chain",), sd, x, pins, feats.grad)
    grads = {k: p.grad for k, p in enc.named_parameters()}
    grads["input"] = xd.grad
    check_all("chain", grads, g64, g32)
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in net.parameters())
    opt.step()
    fresh = chain_net(dev)
    fresh.load_state_dict(net.state_dict())
    with torch.no_grad():
        want = fresh(x.to(dev))
        plain = net(x.to(dev))
    grad_mode = net(x.to(dev))
    for w, p, q in zip(want, plain, grad_mode):
        if isinstance(w, torch.Tensor):
            assert torch.equal(w, p) and torch.equal(w, q)
        else:
            assert torch.equal(w.loc, p.loc) and torch.equal(w.loc, q.loc) and torch.equal(w.scale, p.scale)
    # an encoder that never took the differentiable route does not look at its parameters again
    never = copy.deepcopy(fresh.image_encoder)
    with torch.no_grad():
        never(x.to(dev))
        state = never.device_state()
        never.bn1.bias.add_(1.0)
        never(x.to(dev))
    assert never.device_state() is state and not never._track_versions
