"""GPU parity: ResNet-18 encoder (fp32 MFMA implicit GEMM) and the distribution head against the golden
vectors of the imported reference and against the oracle.

Stated tolerances: encoder features <= 1e-4 relative; head F, S, mode <= 1e-4 absolute given
identical features and the host LAPACK SVD; U, V <= 1e-3 (they are sign-ambiguous and ill-conditioned where
singular values are close; the sign choice is LAPACK's, the same as the reference's)."""
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_cpu as O
from hierarchicalprobabilistic3dhuman_amd import configs, _capi
from hierarchicalprobabilistic3dhuman_amd.resnet import _ConvBN
from conftest import maxerr
from conv_scenario import assert_halo_untouched
from devlib import plain_conv, plain_forward, head_levels_fused, sync_workspaces

pytestmark = pytest.mark.gpu


def test_encoder_reproduces_reference_features(dev, net_gpu, golden, golden_input):
    feats = net_gpu.image_encoder(golden_input.to(dev))
    ref = golden["net_feats"]
    assert feats.shape == (2, 512)
    assert maxerr(feats, ref) <= 1e-4 * float(ref.abs().max())


@pytest.mark.parametrize("svd_mode", ["device", "host"])
def test_net_reproduces_reference_outputs(svd_mode, dev, net_gpu, golden, golden_input):
    """Both SVD modes against the reference's outputs: "host" = MKL sgesdd (the reference's routine), "device" = the in-kernel
    SVD that follows sgesdd step by step -- same signs on the golden matrices, so U and V agree too."""
    net_gpu.svd_mode = svd_mode
    try:
        pose_F, pose_U, pose_S, pose_V, mode, shape_dist, glob, cam = net_gpu(golden_input.to(dev))
    finally:
        net_gpu.svd_mode = "device"
    assert maxerr(pose_F, golden["net_F"]) <= 1e-4
    assert maxerr(pose_S, golden["net_S"]) <= 1e-5 * max(1.0, float(golden["net_S"].max()))
    assert maxerr(mode, golden["net_mode"]) <= 1e-5 if svd_mode == "device" else maxerr(mode, golden["net_mode"]) <= 1e-4
    assert maxerr(pose_U, golden["net_U"]) <= 1e-3 and maxerr(pose_V, golden["net_V"]) <= 1e-3
    assert maxerr(shape_dist.loc, golden["net_shape_loc"]) <= 1e-4
    assert maxerr(shape_dist.scale, golden["net_shape_scale"]) <= 1e-4
    assert maxerr(glob, golden["net_glob"]) <= 1e-4 and maxerr(cam, golden["net_cam"]) <= 1e-4
    assert isinstance(shape_dist, torch.distributions.Normal)


@pytest.mark.parametrize("B", [1, 3, 17, 64])
def test_head_from_features_matches_oracle(B, dev, net_gpu, net_cpu):
    feats = torch.rand(B, 512, generator=torch.Generator().manual_seed(B)) * 2
    ref = O.head_forward(net_cpu[1], feats, configs.SMPL_PARENTS)
    out = net_gpu(None, input_feats=feats.to(dev))
    assert maxerr(out[0], ref[0]) <= 1e-4 and maxerr(out[2], ref[2]) <= 1e-4 and maxerr(out[4], ref[4]) <= 1e-4
    assert maxerr(out[5].loc, ref[5][0]) <= 1e-4 and maxerr(out[6], ref[6]) <= 1e-4 and maxerr(out[7], ref[7]) <= 1e-4


@pytest.mark.parametrize("cfg", [
    # B, H, Cin, Cout, k, stride, pad   -- one case per tile configuration / layer type of ResNet-18
    (2, 64, 64, 64, 3, 1, 1), (2, 64, 64, 128, 3, 2, 1), (2, 64, 64, 128, 1, 2, 0), (64, 8, 512, 512, 3, 1, 1),
    (3, 16, 256, 256, 3, 1, 1), (1, 8, 512, 512, 3, 1, 1), (1, 30, 20, 64, 7, 2, 3), (2, 9, 128, 256, 3, 2, 1)])
def test_conv_bn_relu_kernel(cfg, dev):
    B, H, Cin, Cout, k, s, p = cfg
    torch.manual_seed(sum(cfg))
    conv = torch.nn.Conv2d(Cin, Cout, k, s, p, bias=False)
    bn = torch.nn.BatchNorm2d(Cout).eval()
    bn.running_mean.normal_(); bn.running_var.uniform_(0.5, 2); bn.weight.data.uniform_(0.5, 1.5); bn.bias.data.normal_()
    x = torch.randn(B, Cin, H, H)
    Ho = (H + 2 * p - k) // s + 1
    res = torch.randn(B, Cout, Ho, Ho)
    with torch.no_grad():
        want = F.relu(bn(conv(x)) + res)
        want_nores = bn(conv(x))
    cb = _ConvBN(conv.to(dev), bn.to(dev))
    xh = x.to(dev).permute(0, 2, 3, 1).contiguous()
    got = plain_conv(cb, xh, residual=res.to(dev).permute(0, 2, 3, 1).contiguous(), relu=True)
    assert maxerr(got.permute(0, 3, 1, 2), want) <= 1e-4 * max(1.0, float(want.abs().max()))
    got2 = plain_conv(cb, xh, relu=False)
    assert maxerr(got2.permute(0, 3, 1, 2), want_nores) <= 1e-4 * max(1.0, float(want_nores.abs().max()))
    # every kernel generation / tile shape that supports this layer gives the same answer
    kernels = [("v1", 0)] + ([(kern, v) for kern in ("v2", "v3") for v in (1, 2, 3)] if Cin % 32 == 0 else [])
    for kern, v in kernels:
        cb.variant = v
        alt = plain_conv(cb, xh, residual=res.to(dev).permute(0, 2, 3, 1).contiguous(), relu=True, kernel=kern)
        assert maxerr(alt, got) <= 1e-4 * max(1.0, float(want.abs().max())), (kern, v)
    # split-K (two-pass, deterministic) where the shape allows it
    if Cin % 32 == 0 and Cout % 128 == 0:
        chunks = k * k * Cin // 32
        for ks in (2, 4):
            if chunks % ks == 0:
                cb.variant, cb.ksplit = 0, ks
                alt = plain_conv(cb, xh, residual=res.to(dev).permute(0, 2, 3, 1).contiguous(), relu=True)
                assert maxerr(alt, got) <= 1e-4 * max(1.0, float(want.abs().max())), ("split-K", ks)
                assert torch.equal(alt, plain_conv(cb, xh, residual=res.to(dev).permute(0, 2, 3, 1).contiguous(), relu=True))


def _frame(t_nhwc, pad):
    """(B,H,W,C) -> zero-haloed (B,H+2p,W+2p,C) frame."""
    return F.pad(t_nhwc, (0, 0, pad, pad, pad, pad)).contiguous()


@pytest.mark.parametrize("cfg", [
    # B, H, Cin, Cout, k, stride, pad, ipad -- every layer type of ResNet-18, ragged tiles, Wo % 4 != 0, split-K, the row-mode stem
    (2, 64, 64, 64, 3, 1, 1, 1), (2, 64, 64, 128, 3, 2, 1, 1), (2, 64, 64, 128, 1, 2, 0, 1), (64, 8, 512, 512, 3, 1, 1, 1),
    (3, 16, 256, 256, 3, 1, 1, 1), (1, 8, 512, 512, 3, 1, 1, 1), (2, 9, 128, 256, 3, 2, 1, 1), (3, 14, 64, 64, 3, 1, 1, 2),
    (2, 30, 18, 64, 7, 2, 3, 3), (1, 256, 18, 64, 7, 2, 3, 3), (2, 12, 4, 64, 7, 2, 3, 3),
    (1, 5, 32, 64, 1, 1, 0, 1)])      # a K loop of ONE chunk on a partial tile: the stage prologue and the vmcnt ladder have nothing to prefetch
def test_padded_conv_kernel(cfg, dev):
    """csrc/conv_pad.hip against torch's convolution and, bit for bit, against the conv.hip kernel it replaces
    (same K order and summation order; the row-mode stem has its own K order and is held to the tolerance only)."""
    B, H, Cin, Cout, k, s, p, ipad = cfg
    torch.manual_seed(sum(cfg))
    conv = torch.nn.Conv2d(Cin, Cout, k, s, p, bias=False)
    bn = torch.nn.BatchNorm2d(Cout).eval()
    bn.running_mean.normal_(); bn.running_var.uniform_(0.5, 2); bn.weight.data.uniform_(0.5, 1.5); bn.bias.data.normal_()
    x = torch.randn(B, Cin, H, H)
    Ho = (H + 2 * p - k) // s + 1
    res = torch.randn(B, Cout, Ho, Ho)
    with torch.no_grad():
        want = F.relu(bn(conv(x)) + res)
        want_nores = bn(conv(x))
    tol = 1e-4 * max(1.0, float(want.abs().max()))
    cb = _ConvBN(conv.to(dev), bn.to(dev))
    cb.use_winograd = False                     # this test is about the direct kernel (test_winograd_conv_kernel covers the other)
    xh = x.to(dev).permute(0, 2, 3, 1).contiguous()
    resh = res.to(dev).permute(0, 2, 3, 1).contiguous()
    xp = _frame(xh, ipad)
    for opad in (0, 1):
        out = torch.full((B, Ho + 2 * opad, Ho + 2 * opad, Cout), 7.0, device=dev)
        cb.padded(xp, ipad, out, opad, residual=_frame(resh, opad), relu=True)
        inner = out[:, opad:opad + Ho, opad:opad + Ho]
        assert maxerr(inner.permute(0, 3, 1, 2), want) <= tol
        assert_halo_untouched(out, opad, 7.0)        # the halo is never written: all four sides
        out2 = torch.zeros_like(out)
        cb.padded(xp, ipad, out2, opad, relu=False)
        assert maxerr(out2[:, opad:opad + Ho, opad:opad + Ho].permute(0, 3, 1, 2), want_nores) <= tol
    if Cin % 32 == 0:
        for v in (0, 1, 2, 3, 4):
            if v == 4 and Cout != 64:
                continue
            cb.variant = v
            plain = plain_conv(cb, xh, residual=resh, relu=True)        # same tile / split-K rule on both sides
            out = torch.zeros(B, Ho + 2, Ho + 2, Cout, device=dev)
            cb.padded(xp, ipad, out, 1, residual=_frame(resh, 1), relu=True)
            assert torch.equal(out[:, 1:-1, 1:-1], plain), v
        cb.variant = 0
        if Cout % 128 == 0:
            chunks = k * k * Cin // 32
            for ks in (2, 4):
                if chunks % ks == 0:
                    cb.ksplit = ks
                    plain_k = plain_conv(cb, xh, residual=resh, relu=True)
                    out = torch.zeros(B, Ho + 2, Ho + 2, Cout, device=dev)
                    cb.padded(xp, ipad, out, 1, residual=_frame(resh, 1), relu=True)
                    assert torch.equal(out[:, 1:-1, 1:-1], plain_k), ("split-K", ks)
            cb.ksplit = 0
    # the latency mode's form (round 5): 64 x 64 tiles with a four-stage K loop (variant 5), with and without K slices -- the tile
    # shape and the prefetch distance never change an output's summation order: the bits of the default tiles, slice count for slice count
    for ks in (1, 2, 3, 4, 6, 9, 18):
        if ks > 1 and (Cin % 32 != 0 or (k * k * Cin // 32) % ks != 0):
            continue
        cb.latency, cb.variant, cb.ksplit = False, (3 if Cin % 32 == 0 else 0), ks
        want_k = torch.zeros(B, Ho + 2, Ho + 2, Cout, device=dev)
        cb.padded(xp, ipad, want_k, 1, residual=_frame(resh, 1), relu=True)          # 64 x 64 tiles, two stages (128-row tiles when sliced)
        if ks > 1:
            cb.variant = 0
            ref128 = torch.zeros_like(want_k)
            cb.padded(xp, ipad, ref128, 1, residual=_frame(resh, 1), relu=True)
            assert torch.equal(want_k, ref128), ("64 x 64 tiles, sliced", ks)
        cb.latency, cb.variant = True, 0                                              # -> variant 5 through _tile_variant
        got5 = torch.zeros_like(want_k)
        cb.padded(xp, ipad, got5, 1, residual=_frame(resh, 1), relu=True)
        assert cb._tile_variant(ks) == 5 and torch.equal(got5, want_k), ("four stages", ks)
    cb.latency, cb.variant, cb.ksplit = False, 0, 0


@pytest.mark.parametrize("cfg", [            # (B, H, Cin, Cout, k): the three block entries of ResNet-18 at the bench batch, small / ragged maps, k = 5
    (64, 64, 64, 128, 3), (64, 32, 128, 256, 3), (64, 16, 256, 512, 3), (1, 64, 64, 128, 3), (3, 18, 64, 128, 3), (2, 16, 256, 512, 3),
    (5, 10, 32, 128, 5)])
def test_down_sample_rides_in_the_blocks_first_convolution(cfg, dev):
    """hps_conv2d_bn_act_pad_down (models/resnet.py:62-78 with the down-sample branch of :71-72, :184-188): the block's k x k / 2 convolution
    + bn + relu and its 1 x 1 / 2 down-sample + bn from one launch -- each output equal, BIT FOR BIT, to its own hps_conv2d_bn_act_pad launch
    (and to torch within the tolerance), for every tile variant the entry takes, with K slices, in latency mode, and the halo untouched."""
    B, H, Cin, Cout, k = cfg
    torch.manual_seed(sum(cfg))
    conv = torch.nn.Conv2d(Cin, Cout, k, 2, k // 2, bias=False)
    dconv = torch.nn.Conv2d(Cin, Cout, 1, 2, 0, bias=False)
    bns = []
    for _ in range(2):
        bn = torch.nn.BatchNorm2d(Cout).eval()
        bn.running_mean.normal_(); bn.running_var.uniform_(0.5, 2); bn.weight.data.uniform_(0.5, 1.5); bn.bias.data.normal_()
        bns.append(bn)
    x = torch.randn(B, Cin, H, H)
    with torch.no_grad():
        want, want_d = F.relu(bns[0](conv(x))), bns[1](dconv(x))
    Ho = want.shape[2]
    assert want_d.shape == want.shape
    c1, down = _ConvBN(conv.to(dev), bns[0].to(dev)), _ConvBN(dconv.to(dev), bns[1].to(dev))
    ipad = k // 2                                   # the input halo covers the main convolution's padding
    xp = _frame(x.to(dev).permute(0, 2, 3, 1).contiguous(), ipad)
    assert c1.folds_down(down, H, H, ipad)
    chunks = k * k * Cin // 32
    settings = [(0, 0, False), (1, 0, False), (3, 0, False), (0, 0, True)] + [(0, ks, False) for ks in (2, 4) if chunks % ks == 0] + \
               [(3, ks, False) for ks in (3,) if chunks % ks == 0] + [(0, ks, True) for ks in (9,) if chunks % ks == 0]
    for variant, ks, latency in settings:
        for c in (c1, down):
            c.variant, c.latency = variant, latency
        c1.ksplit = ks
        sep, sep_d = torch.full((B, Ho + 2, Ho + 2, Cout), 7.0, device=dev), torch.full((B, Ho + 2, Ho + 2, Cout), 7.0, device=dev)
        c1.padded(xp, ipad, sep, 1, relu=True)
        down.padded(xp, ipad, sep_d, 1, relu=False)
        got, got_d = torch.full_like(sep, 7.0), torch.full_like(sep, 7.0)
        c1.padded_with_down(xp, ipad, got, 1, down, got_d)
        assert torch.equal(got, sep) and torch.equal(got_d, sep_d), (variant, ks, latency)
        assert_halo_untouched(got, 1, 7.0)           # the halo is never written: all four sides of both frames
        assert_halo_untouched(got_d, 1, 7.0)
        tol = 1e-4 * max(1.0, float(want.abs().max()))
        assert maxerr(got[:, 1:-1, 1:-1].permute(0, 3, 1, 2), want) <= tol and maxerr(got_d[:, 1:-1, 1:-1].permute(0, 3, 1, 2), want_d) <= tol
    c1.ksplit = 0
    # what does not fold: a stride-1 entry, other channel counts on the branch, a Winograd layer
    other = _ConvBN(torch.nn.Conv2d(Cin, Cout, 1, 1, 0, bias=False).to(dev), bns[1])
    assert not c1.folds_down(other, H, H, ipad) and not c1.folds_down(None, H, H, ipad)


def test_encoder_with_and_without_the_folded_down_samples_gives_the_same_features(dev, net_gpu, golden_input):
    enc = net_gpu.image_encoder
    x = torch.cat([golden_input.to(dev), torch.rand(3, 18, 256, 256, generator=torch.Generator().manual_seed(9)).to(dev)])
    assert enc.fold_downsample
    folded = enc(x).clone()
    try:
        enc.composite = False
        folded_b = enc(x).clone()
        enc.fold_downsample = False
        two_b = enc(x).clone()
        enc.composite = True
        two = enc(x).clone()
        net_gpu.set_latency_mode(True)               # latency mode: 64 x 64 four-stage tiles, K slices on the main convolution
        lat_two = enc(x[:1]).clone()
        enc.fold_downsample = True
        lat_folded = enc(x[:1]).clone()
    finally:
        net_gpu.set_latency_mode(False)
        enc.fold_downsample, enc.composite = True, True
    assert torch.equal(folded, folded_b) and torch.equal(folded, two) and torch.equal(folded, two_b)
    assert torch.equal(lat_folded, lat_two)


def test_padded_and_plain_encoders_agree(dev, net_gpu, golden, golden_input):
    enc = net_gpu.image_encoder
    x = golden_input.to(dev)
    plain = plain_forward(enc, x)                           # the un-padded kernel generation (libhps_dev.so, tests/devlib.py)
    padded = enc(x)
    again = enc(x)
    assert torch.equal(padded, again)                       # frames are reused: nothing stale leaks between calls
    ref = golden["net_feats"]
    assert maxerr(plain, ref) <= 1e-4 * float(ref.abs().max()) and maxerr(padded, ref) <= 1e-4 * float(ref.abs().max())
    assert maxerr(padded, plain) <= 2e-5 * float(ref.abs().max())
    # a different batch in between does not disturb the cached frames
    other = enc(torch.rand(3, 18, 256, 256, device=dev))
    assert torch.isfinite(other).all() and torch.equal(enc(x), padded)


@pytest.mark.parametrize("svd_mode", ["device", "host"])
def test_composite_calls_issue_the_same_work(svd_mode, dev, net_gpu, golden_input):
    """hps_encoder_run / hps_head_pose_levels against the one-launch-per-call Python loops: bit-identical outputs."""
    x = torch.cat([golden_input, torch.rand(3, 18, 256, 256, generator=torch.Generator().manual_seed(5))]).to(dev)
    enc = net_gpu.image_encoder
    net_gpu.svd_mode = svd_mode
    try:
        want = net_gpu(x)
        enc.composite = False
        net_gpu.composite_head = False
        got = net_gpu(x)
    finally:
        enc.composite = True
        net_gpu.composite_head = True
        net_gpu.svd_mode = "device"
    for a, b in zip(want, got):
        if isinstance(a, torch.distributions.Normal):
            assert torch.equal(a.loc, b.loc) and torch.equal(a.scale, b.scale)
        else:
            assert torch.equal(a, b)


def test_padded_pooling_and_layout_kernels(dev):
    P = _capi.ptr
    x = torch.randn(2, 18, 12, 10, generator=torch.Generator().manual_seed(0))
    xp = torch.zeros(2, 18, 16, 18, device=dev)
    _capi.call("hps_nchw_to_padded_nhwc", P(x.to(dev)), P(xp), 2, 18, 12, 10, 3, _capi.stream())
    assert maxerr(xp[:, 3:-3, 3:-3].permute(0, 3, 1, 2), x) == 0.0
    xp[:, 3:-3, 3:-3] = 0
    assert float(xp.abs().max()) == 0.0
    y = torch.randn(2, 64, 13, 11)
    yh = y.to(dev).permute(0, 2, 3, 1).contiguous()
    out = torch.zeros(2, 9, 8, 64, device=dev)
    _capi.call("hps_maxpool3x3s2_pad", P(yh), P(out), 2, 13, 11, 64, 1, _capi.stream())
    assert maxerr(out[:, 1:-1, 1:-1].permute(0, 3, 1, 2), F.max_pool2d(y, 3, 2, 1)) == 0.0
    assert float(out[:, 0].abs().max()) == 0.0 and float(out[:, :, 0].abs().max()) == 0.0
    # a thread pools a 2 x 2 block of outputs: odd / even output sizes, a single row, a single pixel
    for (h, w, c) in [(1, 1, 4), (2, 5, 8), (6, 6, 64), (7, 1, 12), (16, 9, 64)]:
        z = torch.randn(3, c, h, w, generator=torch.Generator().manual_seed(h * 31 + w))
        ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        zo = torch.zeros(3, ho + 4, wo + 4, c, device=dev)
        _capi.call("hps_maxpool3x3s2_pad", P(z.to(dev).permute(0, 2, 3, 1).contiguous()), P(zo), 3, h, w, c, 2, _capi.stream())
        assert maxerr(zo[:, 2:-2, 2:-2].permute(0, 3, 1, 2), F.max_pool2d(z, 3, 2, 1)) == 0.0, (h, w, c)
        zo[:, 2:-2, 2:-2] = 0
        assert float(zo.abs().max()) == 0.0, (h, w, c)
    avg = torch.empty(2, 64, device=dev)
    _capi.call("hps_global_avgpool_pad", P(_frame(yh, 1)), P(avg), 2, 13, 11, 64, 1, _capi.stream())
    plain = torch.empty(2, 64, device=dev)
    with _capi.dev_library():                       # the un-padded generation lives in libhps_dev.so
        _capi.call("hps_global_avgpool", P(yh), P(plain), 2, 13 * 11, 64, _capi.stream())
    assert torch.equal(avg, plain) and maxerr(avg, y.mean(dim=(2, 3))) <= 1e-6


def test_pooling_and_layout_kernels(dev):
    """The un-padded generation's relayout / pooling kernels (libhps_dev.so; the cross-check of the product's padded ones)."""
    with _capi.dev_library():
        _pooling_and_layout_kernels(dev)


def _pooling_and_layout_kernels(dev):
    P = _capi.ptr
    x = torch.randn(2, 18, 12, 10, generator=torch.Generator().manual_seed(0))
    xh = torch.empty(2, 12, 10, 20, device=dev)
    _capi.call("hps_nchw_to_nhwc", P(x.to(dev)), P(xh), 2, 18, 12, 10, 20, _capi.stream())
    assert maxerr(xh[..., :18].permute(0, 3, 1, 2), x) == 0.0 and float(xh[..., 18:].abs().max()) == 0.0
    y = torch.randn(2, 64, 13, 11)
    yh = y.to(dev).permute(0, 2, 3, 1).contiguous()
    out = torch.empty(2, 7, 6, 64, device=dev)
    _capi.call("hps_maxpool3x3s2", P(yh), P(out), 2, 13, 11, 64, _capi.stream())
    assert maxerr(out.permute(0, 3, 1, 2), F.max_pool2d(y, 3, 2, 1)) == 0.0
    avg = torch.empty(2, 64, device=dev)
    _capi.call("hps_global_avgpool", P(yh), P(avg), 2, 13 * 11, 64, _capi.stream())
    assert maxerr(avg, y.mean(dim=(2, 3))) <= 1e-6


def test_training_mode_is_refused(dev, net_gpu):
    net_gpu.train()
    try:
        with pytest.raises(RuntimeError):
            net_gpu(torch.zeros(1, 18, 256, 256, device=dev))
    finally:
        net_gpu.eval()


def test_load_state_dict_invalidates_prepared_weights(dev, net_gpu, net_cpu, golden, golden_input):
    import copy
    net = copy.deepcopy(net_gpu)
    sd = {k: v.clone() for k, v in net_cpu[1].items()}
    sd["fc_cam.bias"] = sd["fc_cam.bias"] + 1.0
    net.load_state_dict(sd)
    out = net(None, input_feats=golden["net_feats"].to(dev))
    assert maxerr(out[7], golden["net_cam"] + 1.0) <= 1e-4


def test_reload_through_the_parent_resets_the_encoder_and_copies_own_their_weights(dev, net_gpu, net_cpu, golden, golden_input):
    """nn.Module.load_state_dict recurses with _load_from_state_dict, so a child's load_state_dict override never
    runs -- the encoder's folded filters must be reset by a post hook; and a deepcopy of a PREPARED net must not keep the
    original's device addresses in its pointer tables."""
    import copy
    x = golden_input.to(dev)
    net = copy.deepcopy(net_gpu)
    feats0 = net.image_encoder(x).clone()                          # prepares encoder (and frames)
    net(x)                                                          # prepares the head
    assert net._prepared is not None and net.image_encoder._prepared is not None
    sd = {k: v.clone() for k, v in net_cpu[1].items()}
    sd["image_encoder.bn1.weight"] = sd["image_encoder.bn1.weight"] * 0.5
    net.load_state_dict(sd)                                         # through the PARENT
    assert net._prepared is None and net.image_encoder._prepared is None
    feats1 = net.image_encoder(x)
    assert maxerr(feats1, feats0) > 1e-3                            # the new BatchNorm scale is in effect
    net.load_state_dict(net_cpu[1])
    assert maxerr(net.image_encoder(x), golden["net_feats"]) <= 1e-4 * float(golden["net_feats"].abs().max())
    # a copy of a prepared net rebuilds its own tables; deleting the original must not matter
    net(x)
    clone = copy.deepcopy(net)
    assert clone._prepared is None and clone.image_encoder._prepared is None and clone._pinned_bufs == {}
    del net
    torch.cuda.empty_cache()
    out = clone(x)
    assert maxerr(out[0], golden["net_F"]) <= 1e-4


def test_device_svd_kernel_is_the_host_emulation_and_tracks_lapack(dev, golden):
    """hps_svd3_packed (device) against the same header compiled for the host (bit for bit in both rounding flavours:
    contraction is off in svd3_gesdd.h and its fused multiply-adds are explicit), and -- in the flavour calibrated for THIS
    host's MKL -- against torch.svd: U, S and V bit-identical on every matrix of the 22 families."""
    import ctypes
    from test_host_logic import _svd_families
    fams = [("golden net_F", golden["net_F"].reshape(-1, 3, 3).contiguous())] + _svd_families(20000)
    native = _capi.svd_flavor()
    assert native == _capi.load().hps_host_svd_flavor() and native in (0, 1)
    total = 0
    for name, F in fams:
        n = F.shape[0]
        for flavor in (0, 1):
            usv = torch.empty(n, 21, device=dev)
            _capi.call("hps_svd3_packed", _capi.ptr(F.to(dev)), _capi.ptr(usv), n, flavor, _capi.stream())
            host = torch.empty(n, 21)
            assert _capi.load().hps_host_svd3_emulated(ctypes.c_void_p(F.data_ptr()), ctypes.c_void_p(host.data_ptr()), n, flavor) == 0
            got = usv.cpu()
            assert torch.equal(got, host), (name, flavor)                # device build == host build of the header, both flavours
            if flavor != native:
                continue
            U, S, V = torch.svd(F)
            u, s, v = got[:, :9].reshape(n, 3, 3), got[:, 9:12], got[:, 12:].reshape(n, 3, 3)
            assert torch.equal(s, S) and torch.equal(u, U) and torch.equal(v, V), name      # == this host's LAPACK, bit for bit
            total += n
    print("device svd3 (flavour %d) vs torch.svd on this host: %d of %d matrices bit-identical in U, S, V" % (native, total, total))


def test_head_svd_modes_agree(dev, net_gpu):
    """The head with the in-kernel SVD (default) against the head with the reference's own routine (host MKL sgesdd, one round
    trip per kinematic level): all eight outputs BIT-IDENTICAL -- for the seed-0 weights and for weights scaled to
    trained-like concentrations (x10: singular values up to ~10^2), where a differently signed ancestor vector
    would change every descendant's F by O(1).  The other rounding flavour is run beside it to show what that looks like."""
    import copy
    for gain in (1.0, 10.0):
        net = copy.deepcopy(net_gpu)
        if gain != 1.0:
            with torch.no_grad():
                for m in net.fc_pose:
                    m[2].weight.mul_(gain)
                    m[2].bias.mul_(gain)
            net.invalidate()
        feats = (torch.rand(256, 512, generator=torch.Generator().manual_seed(8)) * 2).to(dev)
        net.svd_mode = "host"
        h = net(None, input_feats=feats)
        net.svd_mode = "device"
        d = net(None, input_feats=feats)
        for i, what in enumerate(("pose_F", "pose_U", "pose_S", "pose_V", "pose_rotmats_mode")):
            assert torch.equal(d[i], h[i]), (gain, what, maxerr(d[i], h[i]))                      # the same bits
        assert torch.equal(d[5].loc, h[5].loc) and torch.equal(d[6], h[6]) and torch.equal(d[7], h[7])
        # the OTHER rounding flavour (what a host with the other MKL code path computes): rounding-level differences, plus the
        # rare differently signed vector pair, which changes the descendants' F by O(gain)
        net.svd_flavor = 1 - _capi.svd_flavor()
        o = net(None, input_feats=feats)
        net.svd_flavor = None
        same = ((h[1] * o[1]).sum(2) > 0).all(2) & ((h[3] * o[3]).sum(2) > 0).all(2)            # (B, 23)
        clean = same.all(1)
        print("head, fc_pose gain %g: other flavour: %d of %d joints differently signed, max |dF| among unaffected images %.2e, "
              "among affected %.2e" % (gain, int((~same).sum()), same.numel(), maxerr(o[0][clean], h[0][clean]),
                                       maxerr(o[0][~clean], h[0][~clean]) if (~clean).any() else 0.0))
        assert float((~same).float().mean()) <= 2e-3
        assert maxerr(o[0][clean], h[0][clean]) <= 1e-4 * max(1.0, float(h[2].max()))


# a matrix (harvested from 4 x 10^5 draws of I + 0.3 N on the CPU) whose second and third singular vectors come out NEGATED in
# one rounding flavour of csrc/svd3_gesdd.h relative to the other -- i.e. on which torch.svd itself returns other signs on an
# Intel host than on an AMD host.  Well conditioned: S = (1.42, 0.88, 0.69).
_F_SIGN_CASE = [float.fromhex(h) for h in (
    "0x1.c983640000000p-1", "0x1.8394320000000p-2", "-0x1.37db980000000p-1", "0x1.28d6da0000000p-2", "0x1.13a95a0000000p+0",
    "-0x1.2e9e040000000p-4", "0x1.cfd8360000000p-2", "0x1.15af3a0000000p-3", "0x1.60e67c0000000p-1")]


def test_cost_of_a_differently_signed_vector_pair(dev, net_gpu, smpl_gpu):
    """what ONE sign disagreement costs downstream.  Body joint 0 (left hip) is forced to F = the matrix
    above for every image (its last layer's weight zeroed, bias F - I); the head then runs in both rounding flavours: the hip's
    own S and mode agree (the pair negated together: U diag(s) V^T unchanged), its U_proper / V differ in sign, and the
    descendants -- knee, ankle, foot (body joints 3, 6, 9) -- see other inputs.  Reported for the seed-0 weights and for
    last-layer weights x 10 (trained-like concentrations): max |dF|, |dmode| of the descendants and the mode vertices.  With the
    calibrated flavour the device path has no such disagreement with this host's torch.svd at all (tests above); this is the
    size of the effect the REFERENCE itself shows between hosts whose MKL rounds differently, one matrix in 10^4."""
    import copy
    from hierarchicalprobabilistic3dhuman_amd.rigid_transform_utils import rot6d_to_rotmat
    F0 = torch.tensor(_F_SIGN_CASE).reshape(3, 3)
    feats = (torch.rand(8, 512, generator=torch.Generator().manual_seed(12)) * 2).to(dev)
    for gain in (1.0, 10.0):
        net = copy.deepcopy(net_gpu)
        with torch.no_grad():
            for j, m in enumerate(net.fc_pose):
                m[2].weight.mul_(gain)
                m[2].bias.mul_(gain)
            net.fc_pose[0][2].weight.zero_()
            net.fc_pose[0][2].bias.copy_((F0 - torch.eye(3)).reshape(9))
        net.invalidate()
        out = {}
        for fl in (0, 1):
            net.svd_flavor = fl
            out[fl] = net(None, input_feats=feats)
        a, b = out[0], out[1]
        assert torch.equal(a[0][:, 0].cpu(), F0.expand(8, 3, 3))                                   # the hip's F is the harvested matrix
        flipped = ((a[1][:, 0] * b[1][:, 0]).sum(1) < 0)                                             # (B, 3) columns of U
        assert flipped[:, 1:].all() and not flipped[:, 0].any()
        assert maxerr(a[2][:, 0], b[2][:, 0]) <= 1e-6 and maxerr(a[4][:, 0], b[4][:, 0]) <= 1e-6     # S, mode of the hip itself
        desc, others = [3, 6, 9], [j for j in range(23) if j not in (0, 3, 6, 9)]
        assert maxerr(a[0][:, others], b[0][:, others]) <= 1e-4 * gain                               # unrelated chains: rounding only
        dF, dM = maxerr(a[0][:, desc], b[0][:, desc]), maxerr(a[4][:, desc], b[4][:, desc])
        glob = rot6d_to_rotmat(a[6])
        va = smpl_gpu(body_pose=a[4].contiguous(), global_orient=glob[:, None].contiguous(), betas=a[5].loc.contiguous(), pose2rot=False).vertices
        vb = smpl_gpu(body_pose=b[4].contiguous(), global_orient=glob[:, None].contiguous(), betas=a[5].loc.contiguous(), pose2rot=False).vertices
        print("one differently signed vector pair at the left hip, fc_pose last layers x %g: descendants max |dF| %.3e, "
              "max |dmode| %.3e, mode vertices max %.3e m" % (gain, dF, dM, maxerr(va, vb)))
        assert dF > 1e-4                                        # the signs do reach the descendants: this is why they matter


@pytest.mark.parametrize("cfg", [
    # B, H, Cin, Cout -- the stride-1 3x3 layers of layer1 / layer2 / layer3 at the 256x256 input, plus an odd batch
    (2, 64, 64, 64), (2, 32, 128, 128), (3, 16, 256, 256), (1, 16, 64, 128), (5, 48, 8, 64), (300, 16, 64, 64),
    # one, two and three chunks of input channels: the window ring and the DMA waits at the ends of a short K loop
    (2, 16, 16, 64), (3, 32, 24, 128),
    # layer4's 8 x 8 maps: four images per item (full and partial quads), K in four slices (512, 256) or one (64)
    (4, 8, 512, 512), (5, 8, 512, 512), (1, 8, 256, 128), (7, 8, 64, 64), (70, 8, 256, 64)])
def test_winograd_conv_kernel(cfg, dev):
    """csrc/conv_wino.hip (Winograd F(2x2, 3x3) + BatchNorm + residual + ReLU) against torch's convolution and against the direct
    implicit-GEMM kernel: same results up to fp32 rounding of a different summation order (<= 1e-5 of the output scale)."""
    B, H, Cin, Cout = cfg
    torch.manual_seed(sum(cfg))
    conv = torch.nn.Conv2d(Cin, Cout, 3, 1, 1, bias=False)
    bn = torch.nn.BatchNorm2d(Cout).eval()
    bn.running_mean.normal_(); bn.running_var.uniform_(0.5, 2); bn.weight.data.uniform_(0.5, 1.5); bn.bias.data.normal_()
    x = torch.randn(B, Cin, H, H)
    res = torch.randn(B, Cout, H, H)
    with torch.no_grad():
        want = F.relu(bn(conv(x)) + res)
        want_nores = bn(conv(x))
    scale_ref = max(1.0, float(want.abs().max()))
    cb = _ConvBN(conv.to(dev), bn.to(dev))
    assert cb.wino_u is not None and cb.winograd_ok(H, H, 1)
    xp = _frame(x.to(dev).permute(0, 2, 3, 1).contiguous(), 1)
    resh = res.to(dev).permute(0, 2, 3, 1).contiguous()
    for opad in (0, 1):
        out = torch.full((B, H + 2 * opad, H + 2 * opad, Cout), 7.0, device=dev)
        cb.padded(xp, 1, out, opad, residual=_frame(resh, opad), relu=True)
        inner = out[:, opad:opad + H, opad:opad + H]
        assert maxerr(inner.permute(0, 3, 1, 2), want) <= 1e-5 * scale_ref
        assert_halo_untouched(out, opad, 7.0)        # the halo is never written: all four sides
        out2 = torch.zeros_like(out)
        cb.padded(xp, 1, out2, opad, relu=False)
        assert maxerr(out2[:, opad:opad + H, opad:opad + H].permute(0, 3, 1, 2), want_nores) <= 1e-5 * scale_ref
        if Cin % 32 == 0:                            # the direct kernel's non-row mode needs 32-channel chunks
            cb.use_winograd = False
            direct = torch.zeros_like(out)
            cb.padded(xp, 1, direct, opad, relu=False)
            cb.use_winograd = True
            assert maxerr(out2, direct) <= 1e-5 * scale_ref
    # maps that are neither 16 x 16-pixel blocks nor 8 x 8 stay on the direct kernel, for every batch size
    assert cb.winograd_ok(8, 8, 1) and not cb.winograd_ok(30, 30, 1) and not cb.winograd_ok(24, 24, 1) and not cb.winograd_ok(4, 4, 1)
    if H == 8:          # per-image results do not depend on the quad an image sits in (bit for bit)
        one = torch.zeros(1, H + 2, H + 2, Cout, device=dev)
        cb.padded(xp[B - 1:B].contiguous(), 1, one, 1, relu=False)
        assert torch.equal(one[0], out2[B - 1])


@pytest.mark.parametrize("cfg", [(1, 32, 32), (2, 64, 96), (3, 256, 256), (5, 224, 224), (33, 128, 64), (1, 32, 288)])
def test_winograd_stem_kernel(cfg, dev):
    """csrc/stem_wino.hip (the 7x7 / 2 stem as four stride-1 phase correlations, F(2x2, r x s), + bn1 + relu) against an fp64
    convolution and against the direct row-mode kernel: both within 2e-6 of the output scale of the fp64 result (the Winograd
    form does 81 instead of 196 multiplications per tile and is at least as close as the direct fp32 sum), for odd item counts
    (a team of the last workgroup idles), non-square maps, an output halo, and bit-identical per image whatever the batch."""
    B, H, W = cfg
    torch.manual_seed(B + H + W)
    conv = torch.nn.Conv2d(18, 64, 7, 2, 3, bias=False)
    bn = torch.nn.BatchNorm2d(64).eval()
    bn.running_mean.normal_(); bn.running_var.uniform_(0.5, 2); bn.weight.data.uniform_(0.5, 1.5); bn.bias.data.normal_()
    x = torch.randn(B, 18, H, W)
    import copy
    with torch.no_grad():
        want = F.relu(copy.deepcopy(bn).double()(copy.deepcopy(conv).double()(x.double()))).permute(0, 2, 3, 1).contiguous()
        want_lin = bn(conv(x)).permute(0, 2, 3, 1).contiguous()
    scale_ref = max(1.0, float(want.abs().max()))
    cb = _ConvBN(conv.to(dev), bn.to(dev), cin_pad=20)
    assert cb.stem_u is not None and cb.stem_winograd_ok(18, H, W) and not cb.stem_winograd_ok(18, H + 2, W) and not cb.stem_winograd_ok(4, H, W)
    P, s = _capi.ptr, _capi.stream()
    xd = x.to(dev)
    frames = torch.zeros(int(_capi.load().hps_stem_phase_frames_bytes(B, H, W)) // 4, device=dev)
    _capi.call("hps_stem_phase_split", P(xd), P(frames), B, 18, H, W, s)
    # the phase frames: frames[b][2 ry + rx][i][j][slot] = x[b][order[slot], 2 i + ry - 3, 2 j + rx - 3], zero outside the image
    # ... and two pixels are followed by two floats of padding (38 floats per pixel pair), which stay zero
    FR, FC = H // 2 + 4, W // 2 + 4
    pairs = frames[:B * 4 * FR * (FC // 2) * 38].view(B, 2, 2, FR, FC // 2, 38).cpu()
    assert float(pairs[..., 36:].abs().max()) == 0
    fr = pairs[..., :36].reshape(B, 2, 2, FR, FC, 18)
    order = [0, 2, 1, 3, 4, 6, 5, 7, 8, 10, 9, 11, 12, 14, 13, 15, 16, 17]
    xpad = torch.zeros(B, 18, 2 * FR, 2 * FC)
    xpad[:, :, 3:3 + H, 3:3 + W] = x
    for ry in (0, 1):
        for rx in (0, 1):
            assert torch.equal(fr[:, ry, rx], xpad[:, order][:, :, ry::2, rx::2].permute(0, 2, 3, 1)), (ry, rx)
    for opad in (0, 1):
        out = torch.full((B, H // 2 + 2 * opad, W // 2 + 2 * opad, 64), 7.0, device=dev)
        _capi.call("hps_stem_winograd", P(frames), P(cb.stem_u), P(cb.scale), P(cb.shift), P(out), B, H, W, opad, 1, s)
        inner = out[:, opad:opad + H // 2, opad:opad + W // 2]
        assert float((inner.cpu().double() - want).abs().max()) <= 2e-6 * scale_ref
        assert_halo_untouched(out, opad, 7.0)        # the halo is never written: all four sides
    lin = torch.empty(B, H // 2, W // 2, 64, device=dev)
    _capi.call("hps_stem_winograd", P(frames), P(cb.stem_u), P(cb.scale), P(cb.shift), P(lin), B, H, W, 0, 0, s)
    assert maxerr(lin, want_lin.to(dev)) <= 1e-5 * scale_ref
    # the direct kernel on the same input
    xin = torch.zeros(B, H + 6, W + 6, 18, device=dev)
    _capi.call("hps_nchw_to_padded_nhwc", P(xd), P(xin), B, 18, H, W, 3, s)
    direct = torch.empty(B, H // 2, W // 2, 64, device=dev)
    cb.use_winograd = False
    cb.padded(xin, 3, direct, 0, relu=False)
    cb.use_winograd = True
    assert maxerr(lin, direct) <= 2e-6 * scale_ref
    # one image alone: the same bits as inside the batch (the summation order depends on the layer only)
    b = B - 1
    f1 = torch.zeros(int(_capi.load().hps_stem_phase_frames_bytes(1, H, W)) // 4, device=dev)
    _capi.call("hps_stem_phase_split", P(xd[b:b + 1].contiguous()), P(f1), 1, 18, H, W, s)
    one = torch.empty(1, H // 2, W // 2, 64, device=dev)
    _capi.call("hps_stem_winograd", P(f1), P(cb.stem_u), P(cb.scale), P(cb.shift), P(one), 1, H, W, 0, 0, s)
    assert torch.equal(one[0], lin[b])
    # argument checks
    with pytest.raises(_capi.HpsError):
        _capi.call("hps_stem_winograd", P(frames), P(cb.stem_u), P(cb.scale), P(cb.shift), P(lin), B, H + 8, W, 0, 0, s)
    with pytest.raises(_capi.HpsError):
        _capi.call("hps_stem_phase_split", P(xd), P(frames), B, 20, H, W, s)


@pytest.mark.parametrize("cfg", [(3, 64, 64), (2, 96, 160), (5, 32, 64), (1, 32, 32), (64, 256, 256)])
def test_stem_with_the_max_pool_in_its_epilogue(cfg, dev):
    """hps_stem_winograd_pooled (stem + bn1 + relu + the 3x3 / 2 / pad 1 max pool of models/resnet.py:150 in one call: the pool is formed
    from the tiles' registers, the full-resolution stem output is never written, a second kernel completes the pooled pixels that see a
    neighbouring work item) against hps_stem_winograd followed by hps_maxpool3x3s2_pad: EQUAL, for odd item counts, one-item and
    non-square maps and the bench shape; the halo of the pooled frame is never written; and against torch's max_pool2d on the stem output."""
    B, H, W = cfg
    torch.manual_seed(11 * B + H + W)
    conv = torch.nn.Conv2d(18, 64, 7, 2, 3, bias=False)
    bn = torch.nn.BatchNorm2d(64).eval()
    bn.running_mean.normal_(); bn.running_var.uniform_(0.5, 2); bn.weight.data.normal_(); bn.bias.data.normal_()      # (negative scales too)
    cb = _ConvBN(conv.to(dev), bn.to(dev), cin_pad=20)
    P, s = _capi.ptr, _capi.stream()
    x = torch.randn(B, 18, H, W, device=dev)
    frames = torch.zeros(int(_capi.load().hps_stem_phase_frames_bytes(B, H, W)) // 4, device=dev)
    _capi.call("hps_stem_phase_split", P(x), P(frames), B, 18, H, W, s)
    Ho, Wo = H // 2, W // 2
    full = torch.empty(B, Ho, Wo, 64, device=dev)
    _capi.call("hps_stem_winograd", P(frames), P(cb.stem_u), P(cb.scale), P(cb.shift), P(full), B, H, W, 0, 1, s)
    want = torch.full((B, Ho // 2 + 2, Wo // 2 + 2, 64), 7.0, device=dev)
    _capi.call("hps_maxpool3x3s2_pad", P(full), P(want), B, Ho, Wo, 64, 1, s)
    side_bytes = int(_capi.load().hps_stem_pool_side_bytes(B, H, W))
    assert side_bytes == B * (H // 32) * (W // 32) * 2048 * 4
    side = torch.full((side_bytes // 4,), float("nan"), device=dev)          # (every entry that is read has been written by the call)
    got = torch.full((B, Ho // 2 + 2, Wo // 2 + 2, 64), 7.0, device=dev)
    _capi.call("hps_stem_winograd_pooled", P(frames), P(cb.stem_u), P(cb.scale), P(cb.shift), P(got), P(side), B, H, W, 1, 1, s)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    assert_halo_untouched(got, 1, 7.0)
    ref = F.max_pool2d(full.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    assert torch.equal(got[:, 1:-1, 1:-1], ref)
    # ... and fed by the NCHW input itself (hps_stem_winograd_pooled_nchw gathers the phase windows: no phase split, no frames): equal again
    direct = torch.full((B, Ho // 2 + 2, Wo // 2 + 2, 64), 7.0, device=dev)
    side.fill_(float("nan"))
    _capi.call("hps_stem_winograd_pooled_nchw", P(x), P(cb.stem_u), P(cb.scale), P(cb.shift), P(direct), P(side), B, H, W, 1, 1, s)
    torch.cuda.synchronize()
    assert torch.equal(direct, want)
    # without ReLU (negative values): the same maxima
    _capi.call("hps_stem_winograd", P(frames), P(cb.stem_u), P(cb.scale), P(cb.shift), P(full), B, H, W, 0, 0, s)
    _capi.call("hps_stem_winograd_pooled", P(frames), P(cb.stem_u), P(cb.scale), P(cb.shift), P(got), P(side), B, H, W, 1, 0, s)
    assert torch.equal(got[:, 1:-1, 1:-1], F.max_pool2d(full.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1))
    with pytest.raises(_capi.HpsError):
        _capi.call("hps_stem_winograd_pooled", P(frames), P(cb.stem_u), P(cb.scale), P(cb.shift), P(got), None, B, H, W, 1, 1, s)


def test_encoder_with_and_without_the_fused_pool_gives_the_same_features(dev, net_gpu, golden_input):
    enc = net_gpu.image_encoder
    x = torch.cat([golden_input.to(dev), torch.rand(3, 18, 256, 256, generator=torch.Generator().manual_seed(4)).to(dev)])
    assert enc.fused_pool and enc.stem_reads_nchw
    direct = enc(x).clone()                      # the default: the stem gathers its windows from the NCHW input, pool in its epilogue
    try:
        enc.composite = False
        direct_b = enc(x).clone()
        enc.stem_reads_nchw = False              # phase split + frame-fed stem with the pool (round 5's default)
        framed_b = enc(x).clone()
        enc.composite = True
        fused = enc(x).clone()
        enc.fused_pool = False                   # ... and the max pool as its own kernel
        two = enc(x).clone()
        enc.composite = False
        two_b = enc(x).clone()
    finally:
        enc.fused_pool, enc.composite, enc.stem_reads_nchw = True, True, True
    for other in (direct_b, framed_b, fused, two_b, two):
        assert torch.equal(direct, other)


def test_winograd_and_direct_encoders_agree_and_are_batch_invariant(dev, net_gpu, golden, golden_input):
    enc = net_gpu.image_encoder
    x = golden_input.to(dev)
    ref = golden["net_feats"]
    wino = enc(x).clone()
    try:
        enc.set_winograd(False)
        direct = enc(x).clone()
    finally:
        enc.set_winograd(True)
    scale_ref = float(ref.abs().max())
    assert maxerr(wino, ref) <= 1e-4 * scale_ref and maxerr(direct, ref) <= 1e-4 * scale_ref
    assert maxerr(wino, direct) <= 2e-5 * scale_ref
    # per-image features do not depend on the batch they were computed in (bit for bit)
    big = torch.cat([x, torch.rand(5, 18, 256, 256, generator=torch.Generator().manual_seed(9)).to(dev)])
    assert torch.equal(enc(big)[:2], wino) and torch.equal(enc(x[1:2]), wino[1:2])


def test_latency_mode_encoder_matches_reference_and_is_batch_invariant(dev, net_gpu, golden, golden_input):
    """ResNet.set_latency_mode: every layer on the direct kernel, the 3x3 layers of layer2-4 with 12-18 K slices (a rule on
    the layer, not on the batch).  Same 1e-4 tolerance against the reference's features; bit-identical per image for every
    batch size within the mode; the default mode's features come back bit for bit when it is switched off."""
    enc = net_gpu.image_encoder
    x = golden_input.to(dev)
    ref = golden["net_feats"]
    scale_ref = float(ref.abs().max())
    default = enc(x).clone()
    try:
        enc.set_latency_mode(True)
        lat = enc(x).clone()
        one = enc(x[1:2]).clone()
        big = enc(torch.cat([x, torch.rand(3, 18, 256, 256, generator=torch.Generator().manual_seed(9)).to(dev)])).clone()
    finally:
        enc.set_latency_mode(False)
    assert maxerr(lat, ref) <= 1e-4 * scale_ref and maxerr(lat, default) <= 2e-5 * scale_ref
    assert torch.equal(one, lat[1:2]) and torch.equal(big[:2], lat)
    assert torch.equal(enc(x), default)


@pytest.mark.parametrize("shape", [(2, 3, 65, 47), (1, 3, 224, 224), (3, 5, 40, 72), (2, 32, 64, 66), (2, 18, 130, 67)])
def test_encoder_takes_any_channel_count_and_image_size(shape, dev):
    """models/resnet.py:127-176: ResNet(in_channels=k) on any image size.  The product library runs them all: a channel-padded,
    even-width input frame (hps_nchw_to_padded_nhwc_generic) in front of the row-mode / direct stem, direct kernels on maps that
    do not split into Winograd blocks.  Against torch's convolutions (the oracle's resnet18_forward), 1e-4 relative; results do
    not depend on the batch; the composite launch list and the per-layer calls agree bit for bit."""
    from hierarchicalprobabilistic3dhuman_amd.resnet import resnet18
    B, C, H, W = shape
    torch.manual_seed(100 + C)
    enc = resnet18(in_channels=C).eval()
    for m in enc.modules():                                   # non-trivial BatchNorm statistics
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0.0, 0.1)
            m.running_var.uniform_(0.6, 1.4)
            m.weight.data.uniform_(0.7, 1.3)
            m.bias.data.normal_(0.0, 0.1)
    sd = {"image_encoder." + k: v.clone() for k, v in enc.state_dict().items()}
    x = torch.rand(B, C, H, W, generator=torch.Generator().manual_seed(sum(shape)))
    with torch.no_grad():
        want = O.resnet18_forward(sd, x)
    enc = enc.to(dev)
    got = enc(x.to(dev))
    assert got.shape == (B, 512)
    assert maxerr(got, want) <= 1e-4 * float(want.abs().max())
    assert torch.equal(enc(x[:1].to(dev)), got[:1])
    enc.composite = False
    assert torch.equal(enc(x.to(dev)), got)


def test_latency_mode_of_the_whole_net(dev, net_gpu, net_cpu, golden, golden_input):
    """PoseMFShapeGaussianNet.set_latency_mode: encoder latency mode + 1024-thread / eight-K-slice workgroups for the joint MLPs
    (HPS_HEAD_WIDE_WORKGROUPS).  Against the reference's golden outputs with the usual tolerances, against the oracle from
    features at B = 1, 3, 17, and bit-identical per image for every batch size within the mode; the default mode's outputs come
    back bit for bit when it is switched off."""
    x = golden_input.to(dev)
    default = [t.clone() if torch.is_tensor(t) else t for t in net_gpu(x)]
    try:
        net_gpu.set_latency_mode(True)
        pose_F, pose_U, pose_S, pose_V, mode, shape_dist, glob, cam = net_gpu(x)
        assert maxerr(pose_F, golden["net_F"]) <= 1e-4 and maxerr(mode, golden["net_mode"]) <= 1e-4
        assert maxerr(pose_S, golden["net_S"]) <= 1e-5 * max(1.0, float(golden["net_S"].max()))
        assert maxerr(pose_U, golden["net_U"]) <= 1e-3 and maxerr(pose_V, golden["net_V"]) <= 1e-3
        assert maxerr(shape_dist.loc, golden["net_shape_loc"]) <= 1e-4 and maxerr(glob, golden["net_glob"]) <= 1e-4
        one = net_gpu(x[1:2])
        assert torch.equal(one[0], pose_F[1:2]) and torch.equal(one[1], pose_U[1:2]) and torch.equal(one[4], mode[1:2])
        for B in (1, 3, 17):
            feats = torch.rand(B, 512, generator=torch.Generator().manual_seed(B)) * 2
            ref = O.head_forward(net_cpu[1], feats, configs.SMPL_PARENTS)
            out = net_gpu(None, input_feats=feats.to(dev))
            assert maxerr(out[0], ref[0]) <= 1e-4 and maxerr(out[2], ref[2]) <= 1e-4 and maxerr(out[4], ref[4]) <= 1e-4
    finally:
        net_gpu.set_latency_mode(False)
    again = net_gpu(x)
    for a, b in zip(default, again):
        if torch.is_tensor(a):
            assert torch.equal(a, b)


@pytest.mark.gpu
def test_all_levels_in_one_launch_equal_the_per_level_launches(dev, net_gpu):
    """VERDICT r4 item 6, the experiment that was measured and not adopted (dev library: hps_dev_head_pose_levels_fused, switched
    driven by tests/devlib.py head_levels_fused): the eight kinematic levels as ONE launch -- workgroups of an image tile hand their level's results to
    each other through counters in global memory.  It stays as a cross-check of "images are independent through the head" and of the
    per-joint code: all eight outputs bit for bit against the eight launches, for batches that leave ragged tiles, for many calls in a row (the counters reset
    themselves), on two streams at once (a workspace per stream), and the fall-back to per-level launches when the grid would not
    fit the chip at once."""
    feats = {B: (torch.rand(B, 512, generator=torch.Generator().manual_seed(70 + B)) * 2).to(dev) for B in (1, 2, 3, 4, 5, 17, 64, 204, 300)}

    def run(B, fused):
        out = head_levels_fused(net_gpu, feats[B]) if fused else net_gpu(None, input_feats=feats[B])
        if out is None:                          # the single launch's grid would not fit the chip at once: the per-level path is the only one
            assert fused and B == 300
            out = net_gpu(None, input_feats=feats[B])
        return [t.clone() for t in out[:5]] + [out[5].loc.clone(), out[5].scale.clone(), out[6].clone(), out[7].clone()]

    try:
        net_gpu.set_latency_mode(True)
        for B in feats:
            want = run(B, False)
            for rep in range(3 if B > 5 else 12):
                got = run(B, True)
                for i, (a, b) in enumerate(zip(want, got)):
                    assert torch.equal(a, b), (B, rep, i, float((a - b).abs().max()))
        # the workspace is left zero (self-resetting counters), whatever the batch
        syncs = sync_workspaces(net_gpu)
        assert syncs and all(int(v.abs().sum()) == 0 for v in syncs.values())
        assert not any(k[2] == (300 + 3) // 4 for k in syncs)     # 5 x 75 workgroups > 256 CUs: per-level launches
        # two streams in flight at once
        want = {B: run(B, False) for B in (1, 5)}
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        outs = {1: [], 5: []}
        for rep in range(10):
            for st, B in ((s1, 1), (s2, 5)):
                with torch.cuda.stream(st):
                    o = head_levels_fused(net_gpu, feats[B])
                    outs[B].append([o[0], o[1], o[2], o[3], o[4]])
        torch.cuda.synchronize()
        for B in (1, 5):
            for o in outs[B]:
                for a, b in zip(want[B][:5], o):
                    assert torch.equal(a, b), B
    finally:
        net_gpu.set_latency_mode(False)

