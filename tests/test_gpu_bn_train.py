"""GPU: training-mode BatchNorm of the encoder (csrc/bn_train.hip, ResNet.set_batchnorm_training).  The five kernels alone against
float64 on frames the tests build; the fold and running update against the float64 formula on the device's own statistics; the whole
encoder (features, input gradient, 20 convolution weights, 40 BatchNorm tensors) against the pinned float64 restatement of
bn_train_scenario by the project's rule, in all three kernel modes; mixed train / eval layers; eval after train; refusals;
repeatability; the loss chain.  Every test fails on a tree without the feature (no switch, no symbols)."""
import copy

import pytest
import torch

import bn_train_scenario as BS
import encoder_grad_scenario as ES
from hierarchicalprobabilistic3dhuman_amd import _capi
from hierarchicalprobabilistic3dhuman_amd.resnet import _ConvBN

pytestmark = pytest.mark.gpu

MODES = ("default", "no_winograd", "latency")
EPS = 1e-5
# (B, H, W, C): two pixels; odd map; more rows than one chunk walks alone and 128 channels; one pixel per image and 512 channels;
# B H W a multiple of no chunk or vector count
SHAPES = [(1, 1, 2, 64), (2, 3, 5, 64), (3, 16, 24, 128), (5, 1, 1, 512), (2, 7, 9, 64)]
P = _capi.ptr
D = lambda t: _capi.ptr(t, torch.float64)


def set_mode(enc, mode):
    enc.set_winograd(mode != "no_winograd")
    enc.set_latency_mode(mode == "latency")
    return enc


def train_encoder(in_channels, dev, mode="default"):
    """A fresh encoder of the recipe on the device, switch on, every BatchNorm training."""
    enc = set_mode(ES.make_encoder(in_channels).to(dev), mode)
    enc.set_batchnorm_training(True)
    return enc.train()


def frame(t_nchw, pad, garbage=False):
    """(B, H + 2 pad, W + 2 pad, C) frame with the NCHW tensor in its interior; halo zero or large garbage."""
    B, C, H, W = t_nchw.shape
    shape = (B, H + 2 * pad, W + 2 * pad, C)
    f = (torch.randn(shape, generator=torch.Generator().manual_seed(3)) * 1e6) if garbage else torch.zeros(shape)
    f[:, pad:pad + H, pad:pad + W] = t_nchw.permute(0, 2, 3, 1).cpu()
    return f.to(t_nchw.device).contiguous()


def interior(f, pad):
    return (f[:, pad:f.shape[1] - pad, pad:f.shape[2] - pad] if pad else f).permute(0, 3, 1, 2)


def raw_map(B, H, W, C, gen):
    """A pre-BatchNorm map: per-channel means and spreads of order one; channels 4..7 have mean 1000 and standard deviation 0.01."""
    z = torch.randn(B, C, H, W, generator=gen) * (0.5 + torch.rand(1, C, 1, 1, generator=gen)) + torch.randn(1, C, 1, 1, generator=gen)
    z[:, 4:8] = 1000.0 + 0.01 * torch.randn(B, 4, H, W, generator=gen)
    return z


def device_stats(zf, B, H, W, C, pad):
    lib = _capi.load()
    ws = torch.empty(lib.hps_bn_batch_stats_workspace(B, H, W, C) // 8, device=zf.device, dtype=torch.float64)
    mean, var = (torch.full((C,), float("nan"), device=zf.device, dtype=torch.float64) for _ in range(2))
    _capi.call("hps_bn_batch_stats", P(zf), D(ws), D(mean), D(var), B, H, W, C, pad, _capi.stream())
    return mean, var


# ---- the kernels alone ----
@pytest.mark.parametrize("pad", [0, 1])
@pytest.mark.parametrize("B,H,W,C", SHAPES)
def test_batch_statistics_kernel(dev, B, H, W, C, pad):
    """float64 accumulation over n <= 2 10^4 values gives ~ n 2^-53 ~ 10^-12; the bound leaves three orders; a bare E[z^2] - mean^2
    lands near 10^-6 on the channels with mean 1000 and standard deviation 0.01."""
    z = raw_map(B, H, W, C, torch.Generator().manual_seed(B * H * W + C))
    z64 = z.double()
    mean64, var64 = z64.mean((0, 2, 3)), z64.var((0, 2, 3), unbiased=False)
    mean, var = device_stats(frame(z.to(dev), pad), B, H, W, C, pad)
    dm, dv = (mean.cpu() - mean64).abs(), (var.cpu() - var64).abs()
    print("stats %s pad %d: max rel mean error %.2e, max rel var error %.2e"
          % ((B, H, W, C), pad, float((dm / (mean64.abs() + var64.sqrt())).max()), float((dv / var64).max())))
    assert bool((dm <= 1e-9 * (mean64.abs() + var64.sqrt())).all())
    assert bool((dv <= 1e-9 * var64).all())
    if pad:                                                      # a halo full of garbage changes nothing, bit for bit
        mean_g, var_g = device_stats(frame(z.to(dev), pad, garbage=True), B, H, W, C, pad)
        assert torch.equal(mean_g, mean) and torch.equal(var_g, var)
    again = device_stats(frame(z.to(dev), pad), B, H, W, C, pad)
    assert torch.equal(again[0], mean) and torch.equal(again[1], var)


@pytest.mark.parametrize("B,H,W,C", SHAPES)
def test_apply_kernel(dev, B, H, W, C):
    """With and without residual and ReLU, out of place (raw halo 0 -> output halo 1) and in place; the halo is untouched."""
    gen = torch.Generator().manual_seed(C + H)
    z, res = torch.randn(B, C, H, W, generator=gen), torch.randn(B, C, H, W, generator=gen)
    scale, shift = 0.5 + torch.rand(C, generator=gen), torch.randn(C, generator=gen)
    bc = lambda v: v[None, :, None, None]
    scale_d, shift_d = scale.to(dev), shift.to(dev)
    for with_res in (False, True):
        for relu in (False, True):
            exact = z.double() * bc(scale).double() + bc(shift).double() + (res.double() if with_res else 0.0)
            if relu:
                exact = exact.clamp_min(0.0)
            tol = 2.0 ** -23 * ((z * bc(scale)).abs() + bc(shift).abs() + (res.abs() if with_res else 0.0)).double()
            for in_place in (False, True):
                zpad, ypad = (1, 1) if in_place else (0, 1)
                zf = frame(z.to(dev), zpad, garbage=True)
                yf = zf if in_place else torch.full((B, H + 2, W + 2, C), 7.0, device=dev)
                halo_before = yf.clone()
                rf = frame(res.to(dev), ypad) if with_res else None
                _capi.call("hps_bn_apply_act_pad", P(zf), P(scale_d), P(shift_d), P(rf) if with_res else None, P(yf), B, H, W, C,
                           zpad, ypad, 1 if relu else 0, _capi.stream())
                got = interior(yf, ypad).cpu().double()
                assert bool(((got - exact).abs() <= tol).all()), (with_res, relu, in_place)
                yf[:, 1:-1, 1:-1] = halo_before[:, 1:-1, 1:-1]
                assert torch.equal(yf, halo_before)


@pytest.mark.parametrize("winograd", [True, False])
def test_apply_kernel_against_the_fused_epilogues(dev, winograd):
    """A 3x3 / 1 layer on 16 x 16 maps with the eval fold's scale and shift: raw convolution (identity pair) + apply against the fused
    hps_conv3x3_winograd / hps_conv2d_bn_act_pad launch, with residual and ReLU: one rounding of contraction difference at most."""
    torch.manual_seed(11)
    conv, bn = torch.nn.Conv2d(64, 64, 3, 1, 1, bias=False), torch.nn.BatchNorm2d(64)
    ES.randomize_bn(bn, seed=2)
    cb = _ConvBN(conv.to(dev), bn.to(dev))
    cb.use_winograd = winograd
    assert cb.winograd_ok(16, 16, 1) == winograd
    gen = torch.Generator().manual_seed(12)
    B = 3
    x, res = torch.randn(B, 64, 16, 16, generator=gen).to(dev), torch.randn(B, 64, 16, 16, generator=gen).to(dev)
    xf, rf = frame(x, 1), frame(res, 1)
    fused, raw, out = (torch.zeros(B, 18, 18, 64, device=dev) for _ in range(3))
    cb.padded(xf, 1, fused, 1, residual=rf, relu=True)
    cb.padded(xf, 1, raw, 1, relu=False, ident=True)
    _capi.call("hps_bn_apply_act_pad", P(raw), P(cb.scale), P(cb.shift), P(rf), P(out), B, 16, 16, 64, 1, 1, 1, _capi.stream())
    zc = interior(raw, 1)
    tol = 2.0 ** -23 * ((zc * cb.scale[None, :, None, None]).abs() + cb.shift.abs()[None, :, None, None] + res.abs())
    err = (interior(out, 1) - interior(fused, 1)).abs()
    print("apply vs fused (winograd=%s): %d of %d elements differ, max ratio to the bound %.3f"
          % (winograd, int((err > 0).sum()), err.numel(), float((err / tol).max())))
    assert bool((err <= tol).all())
    assert float(out[:, 0].abs().max()) == 0.0 and float(out[:, :, 0].abs().max()) == 0.0


@pytest.mark.parametrize("gated", [False, True])
@pytest.mark.parametrize("B,H,W,C", SHAPES)
def test_backward_kernels(dev, B, H, W, C, gated):
    """d beta, d gamma and dz against the float64 formulas of torch's batch_norm backward; the gate fused or off."""
    lib = _capi.load()
    gen = torch.Generator().manual_seed(B + H + W + C)
    z = raw_map(B, H, W, C, gen)
    g, y = torch.randn(B, C, H, W, generator=gen), torch.randn(B, C, H, W, generator=gen)
    y[:, ::2, ::2, ::3] = 0.0                                    # exact zeros are closed gates (every other channel: 1 x 1 maps keep open ones)
    gamma = 0.5 + torch.rand(C, generator=gen)
    n = B * H * W
    z64 = z.double()
    mean, var = z64.mean((0, 2, 3)), z64.var((0, 2, 3), unbiased=False)
    invstd = 1.0 / torch.sqrt(var + EPS)
    bc = lambda v: v[None, :, None, None]
    g64 = (torch.where(y > 0, g, torch.zeros_like(g)) if gated else g).double()
    zhat = (z64 - bc(mean)) * bc(invstd)
    dbeta, dgamma = g64.sum((0, 2, 3)), (g64 * zhat).sum((0, 2, 3))
    dz64 = bc(gamma.double() * invstd) * (g64 - bc(dbeta) / n - zhat * bc(dgamma) / n)
    gf, zf, yf = frame(g.to(dev), 1), frame(z.to(dev), 1, garbage=True), frame(y.to(dev), 1)
    ws = torch.empty(lib.hps_bn_train_backward_sums_workspace(B, H, W, C) // 8, device=dev, dtype=torch.float64)
    mean_d, invstd_d, gamma_d = mean.to(dev), invstd.to(dev), gamma.to(dev)
    sums = torch.full((2 * C,), float("nan"), device=dev, dtype=torch.float64)
    _capi.call("hps_bn_train_backward_sums", P(gf), P(zf), P(yf) if gated else None, D(mean_d), D(invstd_d), D(ws), D(sums),
               B, H, W, C, 1, 1, 1, _capi.stream())
    assert torch.equal(gf.cpu(), frame(g64.float(), 1))                        # gated in place, or untouched
    tol = 4.0 * 2.0 ** -23
    for name, got, ref in (("d beta", sums[:C], dbeta), ("d gamma", sums[C:], dgamma)):
        err = float((got.cpu() - ref).abs().max())
        print("%s %s gated=%s: max error %.3e of max|.| %.3e" % (name, (B, H, W, C), gated, err, float(ref.abs().max())))
        assert err <= tol * float(ref.abs().max())
    dz = torch.zeros(B, H + 2, W + 2, C, device=dev)
    _capi.call("hps_bn_train_backward_dz", P(gf), P(zf), D(mean_d), D(invstd_d), P(gamma_d), D(sums), P(dz), B, H, W, C,
               1, 1, 1, _capi.stream())
    got = interior(dz, 1).cpu().double()
    scale = float(dz64.abs().max())
    assert float((got - dz64).abs().max()) <= tol * scale
    assert float(got.sum((0, 2, 3)).abs().max()) <= tol * scale * n          # the batch mean carries no gradient
    halo = dz.clone()
    halo[:, 1:-1, 1:-1] = 0
    assert float(halo.abs().max()) == 0.0


# ---- fold and running update ----
def buffers(enc):
    return {k: v.clone() for k, v in enc.state_dict().items() if "running" in k or k.endswith("num_batches_tracked")}


def within_one_ulp(got, want32):
    up, down = torch.nextafter(want32, torch.full_like(want32, float("inf"))), torch.nextafter(want32, torch.full_like(want32, -float("inf")))
    return bool(((got == want32) | (got == up) | (got == down)).all())


def test_fold_and_running_update(dev):
    """Every buffer after one training forward = the float64 formula on the device's own training_activations statistics, rounded
    once; momentum 0.1, 0.5 on one layer; the counter moves by one per forward and not by training_activations or backward()."""
    enc = train_encoder(18, dev)
    enc.layer2[0].bn1.momentum = 0.5
    x, cot = ES.case("sq64")
    before = buffers(enc)
    feats_a, _, stats = enc.training_activations(x.to(dev))
    assert all(torch.equal(v, before[k]) for k, v in buffers(enc).items())    # no update
    assert len(stats) == 20
    with torch.no_grad():
        feats = enc(x.to(dev))
    assert torch.equal(feats, feats_a)
    after = buffers(enc)
    keys = BS.layer_keys(ES.state(18))
    for name, (mean, var, n) in stats.items():
        bn = keys[name][1]
        m = 0.5 if name == "layer2.0.c1" else 0.1
        assert n == x.shape[0] * {"stem": 32 * 32}.get(name, n // x.shape[0])
        want_mean = BS.running_update(before[bn + ".running_mean"], mean, m)
        want_var = BS.running_update(before[bn + ".running_var"], var * (n / (n - 1.0)), m)
        assert within_one_ulp(after[bn + ".running_mean"], want_mean), name
        assert within_one_ulp(after[bn + ".running_var"], want_var), name
        assert int(after[bn + ".num_batches_tracked"]) == int(before[bn + ".num_batches_tracked"]) + 1
    # two forwards then two backwards: + 2, the backwards change nothing
    a, b = x.to(dev).requires_grad_(True), (x + 0.25).to(dev).requires_grad_(True)
    fa, fb = enc(a), enc(b)
    mid = buffers(enc)
    assert all(int(mid[k]) == int(after[k]) + 2 for k in mid if k.endswith("num_batches_tracked"))
    params = list(enc.parameters())
    ga = torch.autograd.grad((cot.to(dev) * fa).sum(), [a] + params)
    gb = torch.autograd.grad((cot.to(dev) * fb).sum(), [b] + params)
    assert all(torch.equal(v, mid[k]) for k, v in buffers(enc).items())
    assert all(bool(torch.isfinite(t).all()) for t in ga + gb)
    # ... and each backward differentiated ITS forward (saved statistics, frames of its own): the same call alone gives the same bits
    enc2 = train_encoder(18, dev)
    enc2.layer2[0].bn1.momentum = 0.5
    enc2.load_state_dict({**enc2.state_dict(), **after})
    a2 = x.to(dev).requires_grad_(True)
    g2 = torch.autograd.grad((cot.to(dev) * enc2(a2)).sum(), [a2] + list(enc2.parameters()))
    assert all(torch.equal(u, v) for u, v in zip(ga, g2))


# ---- the whole encoder ----
def device_grads(enc, x, cot, input_grad=True):
    enc.zero_grad(set_to_none=True)
    xd = x.detach().clone().requires_grad_(input_grad)
    feats = enc(xd)
    (cot.to(xd.device) * feats).sum().backward()
    grads = {k: p.grad for k, p in enc.named_parameters()}
    grads["input"] = xd.grad
    return grads, feats.detach()


def check_all(tag, grads, feats, ref64, ref32, keys=None):
    (g64, f64), (g32, f32) = ref64, ref32
    own = BS.own_error({k: g64[k] for k in (keys or g64)}, g32)
    print("%s: the fp32 restatement's own worst-tensor error %.1f x 2^-23 max|g| (cap %d)" % (tag, own, BS.CAP))
    assert own <= BS.CAP
    worst = BS.check("%s features" % tag, feats, f64, f32) if feats is not None else 0.0
    ratio = 0.0
    for k in (keys or g64):
        assert grads[k] is not None, (k, "no gradient on the device")
        worst = max(worst, BS.check("%s %s" % (tag, k), grads[k], g64[k], g32[k]))
        ratio = max(ratio, float((grads[k].detach().cpu().double().reshape(g64[k].shape) - g64[k]).abs().max()) / BS.bound(g64[k], g32[k]))
    print("%s worst error in 2^-23 max|g64|: %.2f; worst error / bound: %.3f" % (tag, worst, ratio))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", BS.GRADIENT_CASES)
def test_features_and_all_gradients_against_the_pinned_float64_reference(dev, name, mode):
    cin, _ = ES.CASES[name]
    enc = train_encoder(cin, dev, mode)
    x, cot = ES.case(name)
    feats_a, maps, _ = enc.training_activations(x.to(dev))
    grads, feats = device_grads(enc, x.to(dev), cot)
    assert torch.equal(feats, feats_a)
    pins = ES.pins_from_maps(maps)
    ref64, ref32 = BS.reference((name, mode), ES.state(cin), x, pins, cot)
    assert set(ref64[0]) == set(grads) and len(grads) == 61
    check_all("%s %s" % (name, mode), grads, feats, ref64, ref32)


def test_frozen_input_frozen_layer_and_skipped_kernels(dev):
    name = "sq64"
    enc = train_encoder(18, dev)
    x, cot = ES.case(name)
    pins = ES.pins_from_maps(enc.training_activations(x.to(dev))[1])
    ref64, ref32 = BS.reference((name, "default"), ES.state(18), x, pins, cot)
    g64 = ref64[0]
    state = {k: v.clone() for k, v in enc.state_dict().items()}
    grads, _ = device_grads(enc, x.to(dev), cot, input_grad=False)
    assert grads["input"] is None
    check_all("frozen input", grads, None, ref64, ref32, [k for k in g64 if k != "input"])
    enc.load_state_dict(state)                                   # the statistics of the recipe again
    enc.layer1.requires_grad_(False)                             # frozen parameters, statistics still training
    grads, _ = device_grads(enc, x.to(dev), cot)
    frozen = [k for k in g64 if k.startswith("layer1.")]
    assert frozen and all(grads[k] is None for k in frozen)
    check_all("layer1 frozen", grads, None, ref64, ref32, [k for k in g64 if k not in frozen])
    enc.load_state_dict(state)
    enc.requires_grad_(False)
    enc.layer3.requires_grad_(True)
    enc.layer4.requires_grad_(True)
    grads, _ = device_grads(enc, x.to(dev), cot, input_grad=False)
    upper = [k for k in g64 if k.startswith(("layer3.", "layer4."))]
    assert all(grads[k] is None for k in g64 if k not in upper)
    check_all("layer3-4 only", grads, None, ref64, ref32, upper)
    enc.load_state_dict(state)
    enc.requires_grad_(False)
    grads, _ = device_grads(enc, x.to(dev), cot)
    check_all("frozen encoder", grads, None, ref64, ref32, ["input"])


# ---- mixed mode ----
def test_stem_and_layer1_in_eval_under_train(dev):
    name = "sq64"
    enc = train_encoder(18, dev)
    enc.bn1.eval()
    enc.layer1.eval()
    x, cot = ES.case(name)
    before = buffers(enc)
    _, maps, stats = enc.training_activations(x.to(dev))
    train = [k for k in BS.layer_keys(ES.state(18)) if k != "stem" and not k.startswith("layer1.")]
    assert sorted(stats) == sorted(train)
    grads, feats = device_grads(enc, x.to(dev), cot)
    after = buffers(enc)
    for k in before:
        still = k.startswith(("bn1.", "layer1."))
        assert torch.equal(before[k], after[k]) == still, k
    ref64, ref32 = BS.reference((name, "mixed"), ES.state(18), x, ES.pins_from_maps(maps), cot, tuple(train))
    check_all("mixed", grads, feats, ref64, ref32)


def test_every_layer_in_eval_with_the_switch_on_is_the_eval_run(dev):
    name = "wide"
    x, cot = ES.case(name)
    off = ES.make_encoder(18).to(dev)
    on = ES.make_encoder(18).to(dev)
    on.set_batchnorm_training(True)
    on.train()
    for m in on.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.eval()
    g_off, f_off = device_grads(off, x.to(dev), cot)
    g_on, f_on = device_grads(on, x.to(dev), cot)
    assert torch.equal(f_on, f_off)
    for k in g_off:
        assert torch.equal(g_on[k], g_off[k]), k
    with torch.no_grad():
        assert torch.equal(on(x.to(dev)), off(x.to(dev)))
    assert all(torch.equal(v, buffers(off)[k]) for k, v in buffers(on).items())


# ---- eval after train ----
def test_eval_after_training_sees_the_new_statistics(dev):
    enc = train_encoder(18, dev)
    x, _ = ES.case("sq64")
    with torch.no_grad():
        enc.eval()
        stale = enc(x.to(dev))                                   # the eval fold of the recipe's statistics exists now
        enc.train()
        enc(x.to(dev))
        enc((x + 0.5).to(dev))
        enc.eval()
        got = enc(x.to(dev))
        fresh = ES.make_encoder(18)
        fresh.load_state_dict(enc.state_dict())
        want = fresh.to(dev).eval()(x.to(dev))
    assert torch.equal(got, want) and not torch.equal(got, stale)
    # the differentiable eval route after training: the data gradient's scaled filters are refolded too
    cot = ES.case("sq64")[1]
    g_enc, _ = device_grads(enc, x.to(dev), cot)
    g_fresh, _ = device_grads(fresh, x.to(dev), cot)
    assert all(torch.equal(g_enc[k], g_fresh[k]) for k in g_enc)


# ---- errors and repeatability ----
def test_refusals_leave_every_buffer_untouched(dev):
    enc = train_encoder(18, dev)
    before = {k: v.clone() for k, v in enc.state_dict().items()}
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        enc(torch.rand(1, 18, 32, 32, device=dev))
    with pytest.raises(ValueError):
        enc.training_activations(torch.rand(1, 18, 32, 32, device=dev))
    enc.layer4[0].bn1.momentum = None
    with pytest.raises(NotImplementedError):
        enc(torch.rand(2, 18, 64, 64, device=dev))
    enc.layer4[0].bn1.momentum = 0.1
    with pytest.raises(RuntimeError):
        enc(torch.rand(2, 18, 64, 64, device=dev), _gate=lambda: None)
    assert all(torch.equal(v, before[k]) for k, v in enc.state_dict().items())
    enc.set_batchnorm_training(False)
    with pytest.raises(RuntimeError):                            # switch off: .train() is refused as ever
        enc(torch.rand(2, 18, 64, 64, device=dev))


def test_two_identical_modules_give_the_same_bits(dev):
    x, cot = ES.case("wide")
    a = train_encoder(18, dev)
    b = copy.deepcopy(a)
    assert b._bn_training and b.training
    ga, fa = device_grads(a, x.to(dev), cot)
    gb, fb = device_grads(b, x.to(dev), cot)
    assert torch.equal(fa, fb)
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k
    assert all(torch.equal(v, buffers(b)[k]) for k, v in buffers(a).items())


# ---- the chain: loss -> SMPL / rot6d -> head -> encoder, training mode ----
def test_training_step_from_the_loss(dev, smpl_gpu):
    """PoseMFShapeGaussianNet with the switch on under .train(): the loss reaches every encoder and head parameter; after an SGD step
    the next forward uses the new weights (and the statistics the first forward left)."""
    from test_gpu_encoder_backward import chain_loss, chain_net
    net = chain_net(dev)
    net.set_batchnorm_training(True)
    net.train()
    x, _ = ES.case("sq64")
    opt = torch.optim.SGD(net.parameters(), lr=1e-6)
    net.zero_grad(set_to_none=True)
    loss = chain_loss(net, smpl_gpu, x.to(dev))
    loss.backward()
    assert bool(torch.isfinite(loss))
    for k, p in net.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0.0, k
    assert int(net.image_encoder.bn1.num_batches_tracked) == 1
    opt.step()
    fresh = chain_net(dev)
    fresh.load_state_dict(net.state_dict())
    fresh.set_batchnorm_training(True)
    fresh.train()
    with torch.no_grad():
        want, got = fresh(x.to(dev)), net(x.to(dev))
    for w, g in zip(want, got):
        if isinstance(w, torch.Tensor):
            assert torch.equal(w, g)
        else:
            assert torch.equal(w.loc, g.loc) and torch.equal(w.scale, g.scale)
    assert all(torch.equal(v, fresh.state_dict()[k]) for k, v in net.state_dict().items())
