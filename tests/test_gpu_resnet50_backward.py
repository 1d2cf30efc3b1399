"""GPU: the Bottleneck encoder's backward (ResNet.set_differentiable; the block walk of ResNet._backward), its training-mode BatchNorm
(csrc/bn_train.hip at 2048 channels), the training loop on a 50-layer net and the 1x1 backward GEMM kernels (csrc/conv1x1_backward.hip).

hps_conv1x1_dgrad owes hps_conv_dgrad its bits (torch.equal on the same buffers); everything else is held to the pinned float64
reference of resnet50_grad_scenario by the project's accuracy rule (smpl_grad_scenario.bound / check): per tensor
max|g_dev - g64| <= 4 max(max|g32 - g64|, 2^-23 max|g64|), masks and pool winners pinned to the device's own run.
Every test prints its figures; the worst ratios measured are recorded in the docstrings (in units of 2^-23 max|g64|)."""
import copy

import pytest
import torch

import resnet50_grad_scenario as GS
import resnet50_scenario as S
from hierarchicalprobabilistic3dhuman_amd import _capi
from hierarchicalprobabilistic3dhuman_amd.device_optim import DeviceAdam
from test_gpu_encoder_backward import chain_loss, check_all, device_grads, mode_of

pytestmark = pytest.mark.gpu

SENTINEL = 7.25
_ENCODERS = {}
MODES = ("default", "no_winograd", "latency", "gemm_off")


def encoder_of(name, dev):
    """The case's encoder on the device with the backward switched on, shared by the tests (they restore every switch they touch and
    never step its parameters)."""
    sd, _, _ = GS.case(name)
    key = S.layers_of(sd)
    if key not in _ENCODERS:
        _ENCODERS[key] = S.build_encoder(key, sd).to(dev)
        _ENCODERS[key].set_differentiable(True)
    return _ENCODERS[key]


class mode50(mode_of):
    def __enter__(self):
        super().__enter__()
        if self.mode == "gemm_off":
            self.enc.gemm_backward = False

    def __exit__(self, *exc):
        super().__exit__(*exc)
        self.enc.gemm_backward = True


def frame_of(t_nchw, pad, channels, fill):
    """(B, H + 2 pad, W + 2 pad, channels) frame filled with ``fill``, the NCHW tensor in the first channels of its interior."""
    B, C, H, W = t_nchw.shape
    f = torch.full((B, H + 2 * pad, W + 2 * pad, channels), fill, device=t_nchw.device, dtype=torch.float32)
    f[:, pad:pad + H, pad:pad + W, :C] = t_nchw.permute(0, 2, 3, 1)
    return f


# ---- per kernel, on the test's own frames ----
# ragged in every tile dimension; K across four chain pieces and an LDS stage with a remainder of 8; stride 2 on odd maps (off-lattice
# pixels); one pixel per image under 2048 input channels
DGRAD_SHAPES = [(40, 72, 1, 3, 5, 7), (64, 264, 1, 2, 9, 13), (256, 512, 2, 3, 9, 14), (128, 64, 2, 1, 5, 7), (2048, 512, 1, 5, 1, 1)]


@pytest.mark.parametrize("cin,cout,stride,B,H,W", DGRAD_SHAPES)
def test_the_gemm_data_gradient_has_the_bits_of_hps_conv_dgrad(dev, cin, cout, stride, B, H, W):
    """With and without the accumulated branch, halos of 0 and 1, more channels in dx than the layer has: torch.equal with
    hps_conv_dgrad on the same buffers (the whole frame: halos and extra channels keep the sentinel), and float64
    torch.nn.grad.conv2d_input by the rule.  g's halo holds NaN: it is never read.
    Measured, worst error in units of 2^-23 max|g64| per shape in the order of DGRAD_SHAPES (the bound is 4 x max(that of the CPU's fp32
    run, 1)): 2.06, 1.64, 1.55, 1.71, 1.31; 0 differing bits against hps_conv_dgrad in all 40 calls."""
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    gen = torch.Generator().manual_seed(cin + cout + H)
    g, w = torch.randn(B, cout, Ho, Wo, generator=gen), torch.randn(cout, cin, 1, 1, generator=gen) / cout ** 0.5
    other = torch.randn(B, cin, H, W, generator=gen)
    ref = {dt: torch.nn.grad.conv2d_input((B, cin, H, W), w.to(dt), g.to(dt), stride=stride, padding=0).double()
           for dt in (torch.float64, torch.float32)}
    wt = w[:, :, 0, 0].contiguous().to(dev)                                  # (Cout, Cin): _dgrad_filter's operand at KH = KW = 1
    worst, P, s = 0.0, _capi.ptr, _capi.stream()
    for gpad, dpad, extra in [(1, 1, 0), (0, 0, 0), (1, 0, 8), (0, 1, 3)]:
        cdx = cin + extra
        gf = frame_of(g.to(dev), gpad, cout, float("nan"))
        for with_other in (False, True):
            of = frame_of(other.to(dev), dpad, cdx, SENTINEL) if with_other else None
            new = torch.full((B, H + 2 * dpad, W + 2 * dpad, cdx), SENTINEL, device=dev)
            old = torch.full_like(new, SENTINEL)
            _capi.call("hps_conv1x1_dgrad", P(gf), P(wt), P(of), P(new), B, H, W, cin, cout, stride, gpad, dpad, cdx, s)
            _capi.call("hps_conv_dgrad", P(gf), P(wt), P(of), P(old), B, H, W, cin, cout, 1, 1, stride, 0, gpad, dpad, cdx, s)
            assert torch.equal(new, old), (gpad, dpad, extra, with_other)
            got = new[:, dpad:dpad + H, dpad:dpad + W, :cin].permute(0, 3, 1, 2)
            add = other.double() if with_other else 0.0
            add32 = (ref[torch.float32].float() + other).double() if with_other else ref[torch.float32]
            worst = max(worst, GS.check("dgrad1x1 %s %dx%dx%d pads=%d,%d Cdx=%d other=%d" % ((cin, cout, stride), B, H, W, gpad, dpad, cdx,
                                                                                         with_other), got, ref[torch.float64] + add, add32))
            rest = new.clone()
            rest[:, dpad:dpad + H, dpad:dpad + W, :cin] = SENTINEL
            assert bool((rest == SENTINEL).all())                            # halos and the extra channels are never touched
            if stride == 2 and not with_other:                               # off the stride lattice: exact zeros
                assert float(got[:, :, 1::2, :].abs().max()) == 0.0 and float(got[:, :, :, 1::2].abs().max()) == 0.0
    print("dgrad1x1 %s worst error in 2^-23 max|g64|: %.2f" % ((cin, cout, stride, B, H, W), worst))


# one output pixel; 15 x (13 x 11) = 2145 pixels: the slices of hps_conv1x1_wgrad_slice_pixels(64, 72) = 1024 pixels end at 1024 and
# 2048, a remainder of 97 follows (B = 5, 715 pixels, would stay inside the first slice); the ragged and the stride-2 shapes
WGRAD_SHAPES = [(64, 64, 1, 1, 1, 1), (64, 72, 1, 15, 13, 11), (40, 72, 1, 3, 5, 7), (64, 264, 1, 2, 9, 13), (256, 512, 2, 3, 9, 14),
                (128, 64, 2, 1, 5, 7), (2048, 512, 1, 5, 1, 1)]


@pytest.mark.parametrize("cin,cout,stride,B,H,W", WGRAD_SHAPES)
def test_the_gemm_weight_gradient_against_float64(dev, cin, cout, stride, B, H, W):
    """float64 torch.nn.grad.conv2d_weight by the rule, e_ref32 from the CPU fp32 run; frames with Cx > Cin and halos of 1 whose extra
    channels and halos hold NaN (never read), gpad 0 and 1; the same bits on a second call and with a poisoned workspace.
    Measured, worst error in units of 2^-23 max|g64| (the CPU's fp32 run in brackets) in the order of WGRAD_SHAPES: 0.42 (0.42),
    1.41 (2.23), 1.91 (1.09), 2.06 (2.80), 1.92 (3.65), 1.30 (1.30), 0.97 (0.97)."""
    lib, P, s = _capi.load(), _capi.ptr, _capi.stream()
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    if (B, H, W) == (15, 13, 11):
        S1 = lib.hps_conv1x1_wgrad_slice_pixels(cin, cout)
        assert S1 == 1024 and B * Ho * Wo == 2 * S1 + 97
    gen = torch.Generator().manual_seed(cin + cout + W)
    x, g = torch.randn(B, cin, H, W, generator=gen), torch.randn(B, cout, Ho, Wo, generator=gen)
    ref = {dt: torch.nn.grad.conv2d_weight(x.to(dt), (cout, cin, 1, 1), g.to(dt), stride=stride, padding=0)[:, :, 0, 0].double()
           for dt in (torch.float64, torch.float32)}
    ws = torch.empty(lib.hps_conv1x1_wgrad_workspace(B, H, W, cin, cout, stride) // 4, device=dev)
    first = None
    for ipad, cx, gpad in [(1, cin + 8, 1), (1, cin, 0), (0, cin + 3, 1)]:
        xf, gf = frame_of(x.to(dev), ipad, cx, float("nan")), frame_of(g.to(dev), gpad, cout, float("nan"))
        out = torch.full((cout, cin), float("nan"), device=dev)
        ws.fill_(float("nan"))                                               # a poisoned workspace: every partial is written before it is read
        _capi.call("hps_conv1x1_wgrad", P(xf), P(gf), P(out), P(ws), B, H, W, ipad, cx, cin, cout, stride, gpad, s)
        GS.check("wgrad1x1 %s %dx%dx%d ipad=%d Cx=%d gpad=%d" % ((cin, cout, stride), B, H, W, ipad, cx, gpad), out, ref[torch.float64],
                 ref[torch.float32])
        again = torch.empty_like(out)
        _capi.call("hps_conv1x1_wgrad", P(xf), P(gf), P(again), P(ws), B, H, W, ipad, cx, cin, cout, stride, gpad, s)
        assert torch.equal(out, again)
        first = out if first is None else first
        assert torch.equal(out, first)                                       # the frames' layout changes no bit


# ---- the whole encoder ----
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["small_wino", "small_generic"])
def test_all_gradients_against_the_pinned_float64_reference(dev, name, mode):
    """Gradient of the input, every convolution weight, every BatchNorm weight and bias; the differentiable forward's features and
    activations()'s features equal the no_grad forward's bit for bit.
    Measured, worst tensor in units of 2^-23 max|g64| (the bound is 4 x max(the CPU fp32 restatement's, 1) per tensor), default /
    no_winograd / latency / gemm_off: small_wino 4.05 / 3.79 / 4.18 / 4.05 (1 or 2 mask flips against the CPU's own run),
    small_generic 6.24 in every mode (0 flips)."""
    enc = encoder_of(name, dev)
    sd, x, cot = GS.case(name)
    with mode50(enc, mode):
        with torch.no_grad():
            plain = enc(x.to(dev))
        assert plain.grad_fn is None
        grads, feats = device_grads(enc, x.to(dev), cot)
        act_feats, maps = enc.activations(x.to(dev))
        with torch.no_grad():
            after = enc(x.to(dev))
    assert torch.equal(feats, plain) and torch.equal(act_feats, plain) and torch.equal(after, plain)
    assert "layer4.0.c3" in maps and "layer1.1.c3" in maps
    pins = GS.pins_from_maps(maps)
    print("%s %s: %d mask / winner flips against the fp32 CPU restatement" % (name, mode, GS.flips(pins, GS.self_pins(name))))
    g64, g32 = GS.reference((name, mode), sd, x, pins, cot)
    assert set(g64) == set(grads)
    check_all("%s %s" % (name, mode), grads, g64, g32)


def test_all_gradients_of_the_50_layer_stack(dev):
    """layers (3, 4, 6, 3) at (2, 18, 64, 64), default mode.  Measured: worst tensor 7.21 x 2^-23 max|g64|."""
    enc = encoder_of("full", dev)
    sd, x, cot = GS.case("full")
    grads, feats = device_grads(enc, x.to(dev), cot)
    act_feats, maps = enc.activations(x.to(dev))
    assert torch.equal(act_feats, feats) and feats.shape == (2, 2048)
    g64, g32 = GS.reference(("full", "default"), sd, x, GS.pins_from_maps(maps), cot)
    assert set(g64) == set(grads) and len(g64) == 1 + 3 * 53
    check_all("full", grads, g64, g32)


@pytest.mark.parametrize("name", ["small_wino", "small_generic"])
def test_the_gemm_kernels_change_no_bit_of_the_input_gradient(dev, name):
    """hps_conv1x1_dgrad has hps_conv_dgrad's bits, and the weight gradients never enter the data path."""
    enc = encoder_of(name, dev)
    _, x, cot = GS.case(name)
    on, _ = device_grads(enc, x.to(dev), cot)
    on = {k: v.clone() for k, v in on.items()}
    with mode50(enc, "gemm_off"):
        off, _ = device_grads(enc, x.to(dev), cot)
    assert torch.equal(on["input"], off["input"])
    prep = enc._prepared
    routed = {n for (n, _, _), cb in zip(enc._enc_layers(), type(enc)._convs(prep)) if enc._gemm_wgrad(cb)}
    assert routed and len(routed) < len(enc._enc_layers())
    for (n, conv, bn) in enc._enc_layers():
        key = [k for k, p in enc.named_parameters() if p is bn.bias][0]
        assert torch.equal(on[key], off[key]), key                           # the shift gradients are sums of the same cotangents
        wkey = [k for k, p in enc.named_parameters() if p is conv.weight][0]
        if n not in routed:
            assert torch.equal(on[wkey], off[wkey]), wkey                    # ... and an unrouted layer runs the very same launches


def test_route_and_frozen_variants(dev):
    """Fails without the feature (no set_differentiable).  What is asked for meets the rule, what is not asked for stays None.
    Measured (units of 2^-23 max|g64|): frozen input 6.24, layer1 frozen 5.27, layer3-4 only 5.27, one weight 3.31, frozen encoder 2.29."""
    name = "small_generic"
    enc = copy.deepcopy(encoder_of(name, dev))
    assert not enc._forward_only                                             # the switch travels with the copy
    sd, x, cot = GS.case(name)
    assert enc(x.to(dev)).grad_fn is not None
    with torch.no_grad():
        assert enc(x.to(dev)).grad_fn is None
    pins = GS.pins_from_maps(enc.activations(x.to(dev))[1])
    g64, g32 = GS.reference((name, "default"), sd, x, pins, cot)
    grads, _ = device_grads(enc, x.to(dev), cot, input_grad=False)
    assert grads["input"] is None
    check_all("frozen input", grads, g64, g32, [k for k in g64 if k != "input"])
    enc.layer1.requires_grad_(False)
    grads, _ = device_grads(enc, x.to(dev), cot)
    frozen = [k for k in g64 if k.startswith("layer1.")]
    assert frozen and all(grads[k] is None for k in frozen)
    check_all("layer1 frozen", grads, g64, g32, [k for k in g64 if k not in frozen])
    enc.requires_grad_(False)
    enc.layer3.requires_grad_(True)
    enc.layer4.requires_grad_(True)
    grads, _ = device_grads(enc, x.to(dev), cot, input_grad=False)
    upper = [k for k in g64 if k.startswith(("layer3.", "layer4."))]
    assert all(grads[k] is None for k in g64 if k not in upper)
    check_all("layer3-4 only", grads, g64, g32, upper)
    enc.requires_grad_(False)                                                # only conv2 of layer2.1: the walk stops inside a block
    enc.layer2[1].conv2.weight.requires_grad_(True)
    grads, _ = device_grads(enc, x.to(dev), cot, input_grad=False)
    assert [k for k in g64 if grads[k] is not None] == ["layer2.1.conv2.weight"]
    check_all("one weight", grads, g64, g32, ["layer2.1.conv2.weight"])
    enc.requires_grad_(False)
    grads, _ = device_grads(enc, x.to(dev), cot)
    assert all(grads[k] is None for k in g64 if k != "input")
    check_all("frozen encoder", grads, g64, g32, ["input"])
    assert enc(x.to(dev)).grad_fn is None                                    # all frozen: the plain route
    enc.set_differentiable(False)
    with pytest.raises(NotImplementedError, match=r"torch\.no_grad\(\)"):
        enc(x.to(dev).requires_grad_(True))


def test_a_second_forward_between_a_forward_and_its_backward_changes_nothing(dev):
    enc = encoder_of("small_wino", dev)
    _, xa, cot = GS.case("small_wino")
    xb = torch.rand(xa.shape, generator=torch.Generator().manual_seed(78))
    single, _ = device_grads(enc, xa.to(dev), cot)
    single = {k: v.clone() for k, v in single.items()}
    again, _ = device_grads(enc, xa.to(dev), cot)
    assert all(torch.equal(single[k], again[k]) for k in single)             # bitwise repeatable
    enc.zero_grad(set_to_none=True)
    a, b = xa.to(dev).requires_grad_(True), xb.to(dev).requires_grad_(True)
    fa, fb = enc(a), enc(b)
    ga = torch.autograd.grad((cot.to(dev) * fa).sum(), [a] + list(enc.parameters()))
    del fb
    for k, v in zip(["input"] + [k for k, _ in enc.named_parameters()], ga):
        assert torch.equal(v, single[k]), k


def test_input_gradient_of_an_image_does_not_depend_on_the_batch(dev):
    enc = encoder_of("small_wino", dev)
    _, x, cot = GS.case("small_wino")
    g3, _ = device_grads(enc, x.to(dev), cot)
    g3 = g3["input"].clone()
    for i in range(x.shape[0]):
        g1, _ = device_grads(enc, x[i:i + 1].to(dev), cot[i:i + 1])
        assert torch.equal(g1["input"][0], g3[i]), i


# ---- optimiser steps ----
def frame_pointers(enc):
    out = []
    for kind in ("frames", "backward_frames"):
        for entry in enc.device_state().get(kind, {}).values():
            sets = entry[0] if kind == "backward_frames" else (entry[0],)
            for fs in sets[:2]:
                out += [t.data_ptr() for ent in fs["blocks"] for t in ent.values() if isinstance(t, torch.Tensor)]
    return out


@pytest.mark.parametrize("name,winograd", [("small_generic", True), ("small_wino", False), ("small_wino", True)])
def test_device_adam_refreshes_a_bottleneck_encoder_in_place(dev, name, winograd):
    """After one DeviceAdam(..., refresh=(enc,)) step the prepared state, the frames and the launch lists survive, and the next forward
    and the next backward equal those of a freshly built encoder with the stepped weights bit for bit (every filter form the forward
    and the backward kernels read was rewritten: hps_bottleneck_expand_down's, the data gradient's scaled filters, the folds).
    Where the stem runs in its Winograd form (small_wino with Winograd on) the refreshed ``stem_u`` differs from the host-built one in
    last bits -- tests/test_gpu_optim.py records the same for the 18-layer encoder and holds the features to 1e-4 there --: then every
    other derived tensor is compared bit for bit and the features by that bound."""
    sd, x, cot = GS.case(name)
    layers = S.layers_of(sd)

    def build(state_dict):
        e = S.build_encoder(layers, state_dict).to(dev)
        e.set_differentiable(True)
        e.set_winograd(winograd)
        return e

    enc = build(sd)
    stem_wino = enc._prepared["stem"].stem_winograd_ok(*x.shape[1:])
    assert stem_wino == (name == "small_wino" and winograd)
    opt = DeviceAdam(enc.parameters(), lr=1e-3, refresh=(enc,))
    device_grads(enc, x.to(dev), cot)
    state, prep, pointers = enc.device_state(), enc._prepared, frame_pointers(enc)
    assert len(pointers) > 40
    before = {k: p.detach().clone() for k, p in enc.named_parameters()}
    opt.step()
    assert all(not torch.equal(before[k], p.detach()) for k, p in enc.named_parameters())      # every encoder parameter moved
    grads, feats = device_grads(enc, x.to(dev), cot)
    assert enc.device_state() is state and enc._prepared is prep and frame_pointers(enc) == pointers
    fresh = build({k: v.detach().cpu() for k, v in enc.state_dict().items()})
    want, want_feats = device_grads(fresh, x.to(dev), cot)
    names = [n for n, _, _ in enc._enc_layers()]
    compared = 0
    for n, a, b in zip(names, type(enc)._convs(enc._prepared), type(enc)._convs(fresh._prepared)):
        for attr in ("wk", "wn", "wrow", "wino_u", "scale", "shift"):       # (not stem_u: see above; unread unless stem_wino)
            if getattr(a, attr) is not None:
                assert torch.equal(getattr(a, attr), getattr(b, attr)), (n, attr)
                compared += 1
    bwd, fresh_bwd = enc._prepared["bwd"], fresh._prepared["bwd"]
    assert set(bwd) == set(fresh_bwd) and len(bwd) >= len(names) - 1 and all(torch.equal(bwd[k], fresh_bwd[k]) for k in bwd)
    assert compared >= 4 * len(names)
    if stem_wino:
        assert float((feats - want_feats).abs().max()) <= 1e-4 * float(want_feats.abs().max())
    else:
        assert torch.equal(feats, want_feats)
        for k in want:
            assert torch.equal(grads[k], want[k]), k
    # switched off, the refresh drops the state instead (always correct)
    enc.set_differentiable(False)
    enc.refresh_weights()
    assert enc._prepared is None


def test_loss_chain_reaches_a_50_layer_encoder_and_refreshes_in_place(dev, smpl_gpu):
    """PoseMFShapeGaussianLoss -> SMPL / rot6d -> head -> Bottleneck encoder from an image batch, the net of MODEL.NUM_RESNET_LAYERS =
    50 with set_differentiable_encoder(True).  The encoder's gradients meet the rule against the reference VJP fed with the feature
    cotangent the device chain produced; after one DeviceAdam(..., refresh=(net,)) step the next forward equals a freshly built net
    with the stepped weights bit for bit on the frames of before the step.  Measured: worst tensor 5.15 x 2^-23 max|g64|."""
    from hierarchicalprobabilistic3dhuman_amd import configs
    from hierarchicalprobabilistic3dhuman_amd.poseMF_shapeGaussian_net import PoseMFShapeGaussianNet

    def build(state_dict):
        net = PoseMFShapeGaussianNet(configs.SMPL_PARENTS, S.net_config()).eval()
        net.load_state_dict(state_dict, strict=True)
        net.set_differentiable_encoder(True)
        # every layer direct: the Winograd stem's refreshed form differs from the host-built one in last bits (see the test above;
        # the all-gradients tests cover the Winograd kernels), and this test compares a refreshed net with a fresh one bit for bit
        net = net.to(dev)
        net.image_encoder.set_winograd(False)
        return net

    net = build(S.net_state_dict(PoseMFShapeGaussianNet, configs.SMPL_PARENTS))
    enc = net.image_encoder
    x = S.case("full")[1]
    kept = []

    def keep_features(module, args, output):
        output.retain_grad()
        kept.append(output)

    hook = enc.register_forward_hook(keep_features)
    opt = DeviceAdam(net.parameters(), lr=1e-5, refresh=(net,))
    net.zero_grad(set_to_none=True)
    xd = x.to(dev).requires_grad_(True)
    chain_loss(net, smpl_gpu, xd).backward()
    hook.remove()
    feats = kept[0]
    assert feats.shape == (2, 2048) and feats.grad is not None and bool(torch.isfinite(feats.grad).all())
    sd = {k: v.detach().cpu().clone() for k, v in enc.state_dict().items()}
    pins = GS.pins_from_maps(enc.activations(x.to(dev))[1])
    g64, g32 = GS.reference(("chain",), sd, x, pins, feats.grad)
    grads = {k: p.grad for k, p in enc.named_parameters()}
    grads["input"] = xd.grad
    check_all("chain50", grads, g64, g32)
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in net.parameters())
    state, pointers = enc.device_state(), frame_pointers(enc)
    opt.step()
    with torch.no_grad():
        plain = net(x.to(dev))
    assert enc.device_state() is state and frame_pointers(enc) == pointers
    fresh = build({k: v.detach().cpu() for k, v in net.state_dict().items()})
    with torch.no_grad():
        want = fresh(x.to(dev))
    for w, p in zip(want, plain):
        if isinstance(w, torch.Tensor):
            assert torch.equal(w, p)
        else:
            assert torch.equal(w.loc, p.loc) and torch.equal(w.scale, p.scale)


# ---- training-mode BatchNorm (csrc/bn_train.hip at 2048 channels; ResNet.set_batchnorm_training on a Bottleneck encoder) ----
@pytest.mark.parametrize("B,H,W,C", [(5, 1, 1, 2048), (2, 3, 5, 2048), (3, 2, 2, 3072)])
def test_batchnorm_kernels_at_more_than_1024_channels(dev, B, H, W, C):
    """tests/test_gpu_bn_train.py's kernel tests as they stand, at channel counts the kernels cut into windows of 1024."""
    import test_gpu_bn_train as TB
    for pad in (0, 1):
        TB.test_batch_statistics_kernel(dev, B, H, W, C, pad)
    TB.test_apply_kernel(dev, B, H, W, C)
    for gated in (False, True):
        TB.test_backward_kernels(dev, B, H, W, C, gated)


def train_encoder(name, dev):
    """A fresh encoder of the case on the device, both switches on, every BatchNorm training."""
    sd, _, _ = GS.case(name)
    enc = S.build_encoder(S.layers_of(sd), sd).to(dev)
    enc.set_differentiable(True)
    enc.set_batchnorm_training(True)
    return enc.train()


def check_train(tag, grads, feats, ref64, ref32):
    (g64, f64), (g32, f32) = ref64, ref32
    own = max(float((g32[k] - g64[k]).abs().max()) / (GS.EPS32 * float(g64[k].abs().max())) for k in g64)
    print("%s: the fp32 restatement's own worst-tensor error %.1f x 2^-23 max|g|" % (tag, own))
    worst = GS.check("%s features" % tag, feats, f64, f32)
    for k in g64:
        assert grads[k] is not None, (k, "no gradient on the device")
        worst = max(worst, GS.check("%s %s" % (tag, k), grads[k], g64[k], g32[k]))
    print("%s worst error in 2^-23 max|g64|: %.2f" % (tag, worst))


@pytest.mark.parametrize("name", ["small_wino", "small_generic"])
def test_training_batchnorm_features_gradients_and_running_buffers(dev, name):
    """Every BatchNorm on batch statistics (small_generic: n = 4 values per channel in layer4, where the restatement's own fp32 error
    is large and the rule's bound with it -- the printed figure says how large): features and every gradient against the scenario;
    the running buffers follow the float64 formula on the device's own statistics, move once per forward and not by the backward or
    by training_activations.  Measured, worst tensor in units of 2^-23 max|g64| (the CPU fp32 restatement's own worst tensor in
    brackets): small_wino 88.4 (105.1), small_generic 884.0 (547.8) -- every tensor within 4 x its own fp32 figure."""
    from test_gpu_bn_train import buffers, within_one_ulp
    enc = train_encoder(name, dev)
    sd, x, cot = GS.case(name)
    before = buffers(enc)
    feats_a, maps, stats = enc.training_activations(x.to(dev))
    assert all(torch.equal(v, before[k]) for k, v in buffers(enc).items())
    assert len(stats) == 1 + 3 * 6 + 4 and "layer1.0.down" in maps and "layer4.0.c3" in maps
    grads, feats = device_grads(enc, x.to(dev), cot)
    after = buffers(enc)
    assert torch.equal(feats, feats_a)
    keys = GS.layer_keys(sd)
    for layer, (mean, var, n) in stats.items():
        bn = keys[layer][1]
        assert within_one_ulp(after[bn + ".running_mean"], GS.running_update(before[bn + ".running_mean"], mean, 0.1)), layer
        assert within_one_ulp(after[bn + ".running_var"], GS.running_update(before[bn + ".running_var"], var * (n / (n - 1.0)), 0.1)), layer
        assert int(after[bn + ".num_batches_tracked"]) == int(before[bn + ".num_batches_tracked"]) + 1
    ref64, ref32 = GS.reference_train((name, "all"), sd, x, GS.pins_from_maps(maps), cot)
    assert set(ref64[0]) == set(grads)
    check_train("%s train" % name, grads, feats, ref64, ref32)


@pytest.mark.parametrize("variant", ["layer1_eval", "down_only", "c3_only"])
@pytest.mark.parametrize("name", ["small_wino", "small_generic"])
def test_mixed_training_and_eval_layers(dev, name, variant):
    """enc.layer1.eval() freezes layer1 onto the folded path (its entry block through hps_bottleneck_expand_down again); entry blocks
    with only the down-sample's or only conv3's BatchNorm training are taken apart.  Measured, as above, layer1_eval / down_only /
    c3_only: small_wino 59.4 (114.9) / 25.1 (39.4) / 54.1 (45.6); small_generic 399.6 (213.0) / 248.8 (85.8) / 170.9 (102.8)."""
    from test_gpu_bn_train import buffers
    enc = train_encoder(name, dev)
    sd, x, cot = GS.case(name)
    names = list(GS.layer_keys(sd))
    if variant == "layer1_eval":
        enc.layer1.eval()
        train = [n for n in names if not n.startswith("layer1.")]
    else:
        for m in enc.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.eval()
        for stage in (enc.layer1, enc.layer2, enc.layer3, enc.layer4):
            (stage[0].downsample[1] if variant == "down_only" else stage[0].bn3).train()
        train = [n for n in names if n.endswith(".0.down" if variant == "down_only" else ".0.c3")]
    before = buffers(enc)
    _, maps, stats = enc.training_activations(x.to(dev))
    assert sorted(stats) == sorted(train) and len(train) >= 4
    grads, feats = device_grads(enc, x.to(dev), cot)
    after = buffers(enc)
    keys = GS.layer_keys(sd)
    moved = {keys[n][1] for n in train}
    for k in before:
        assert torch.equal(before[k], after[k]) == (k.rsplit(".", 1)[0] not in moved), k
    ref64, ref32 = GS.reference_train((name, variant), sd, x, GS.pins_from_maps(maps), cot, tuple(train))
    check_train("%s %s" % (name, variant), grads, feats, ref64, ref32)


def test_every_layer_in_eval_with_both_switches_on_is_the_eval_run(dev):
    name = "small_wino"
    sd, x, cot = GS.case(name)
    on = train_encoder(name, dev)
    for m in on.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.eval()
    g_on, f_on = device_grads(on, x.to(dev), cot)
    g_off, f_off = device_grads(encoder_of(name, dev), x.to(dev), cot)
    assert torch.equal(f_on, f_off) and all(torch.equal(g_on[k], g_off[k]) for k in g_off)


# ---- the training loop ----
def test_the_training_loop_runs_a_50_layer_net(dev, smpl_gpu, tmp_path):
    """train_poseMF_shapeGaussian_net on the tiny datasets of tests/test_gpu_train_loop.py with a 50-layer net, the switch on: two
    train iterations per stage (stage change at epoch 1), finite losses, checkpoints with the reference's six keys, the net's own
    state-dict keys, every encoder parameter moved, the BatchNorm opt-in restored (the registered DeviceAdam's in-place refresh has its
    own test above; the loop ends by loading the best weights, which drops the state).  The same net with the switch off is refused at entry with nothing written."""
    import os
    import pickle
    import head_grad_scenario as HS
    import encoder_grad_scenario as ES
    import test_gpu_train_loop as TL
    from hierarchicalprobabilistic3dhuman_amd import train_poseMF_shapeGaussian_net as tp
    cfg = TL.make_cfg()
    cfg.MODEL.NUM_RESNET_LAYERS = 50
    w = TL.make_world(dev, smpl_gpu, cfg, metrics=list(TL.METRICS))
    net = HS.make_net("spread", config=cfg)
    assert net.fc1.in_features == 2048 and net.image_encoder._forward_only
    ES.randomize_bn(net.image_encoder)
    net = net.to(dev)
    opt = DeviceAdam(net.parameters(), lr=1e-4, refresh=(net,))
    train, val = TL.datasets()
    train = list(train) + list(val)                                          # two iterations of B = 2 per epoch, one epoch per stage
    off_dir = str(tmp_path / "off")
    os.makedirs(off_dir)
    with pytest.raises(NotImplementedError, match="ResNet-50"):
        tp.train_poseMF_shapeGaussian_net(net, cfg, smpl_gpu, w["edge"], w["renderer"], dev, train, val, w["criterion"], opt, list(TL.METRICS),
                                          off_dir, os.path.join(off_dir, "log.pkl"))
    assert not os.listdir(off_dir)
    net.set_differentiable_encoder(True)
    before = {k: p.detach().clone() for k, p in net.image_encoder.named_parameters()}
    out_dir = str(tmp_path / "on")
    os.makedirs(out_dir)
    TL.seed_all(9)
    model = tp.train_poseMF_shapeGaussian_net(net, cfg, smpl_gpu, w["edge"], w["renderer"], dev, train, val, w["criterion"], opt,
                                              list(TL.METRICS), out_dir, os.path.join(out_dir, "log.pkl"))
    assert model is net and not net.image_encoder._bn_training and not net.image_encoder._forward_only
    with open(os.path.join(out_dir, "log.pkl"), "rb") as f:
        history = pickle.load(f)
    assert all(len(v) == 2 and all(x == x and abs(x) != float("inf") for x in v) for v in history.values())
    for name in ("epoch_000.tar", "epoch_001.tar"):
        ckpt = torch.load(os.path.join(out_dir, name), map_location="cpu", weights_only=False)
        assert sorted(ckpt) == ["best_epoch", "best_epoch_val_metrics", "best_model_state_dict", "epoch", "model_state_dict", "optimiser_state_dict"]
        assert set(ckpt["model_state_dict"]) == set(net.state_dict()) == set(ckpt["best_model_state_dict"])
    assert all(not torch.equal(before[k], p.detach()) for k, p in net.image_encoder.named_parameters())
