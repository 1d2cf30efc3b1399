"""The convolution kernels on NON-SQUARE maps against float64 (tests/conv_scenario.py: the cases, the CPU references, the accuracy rule
bound = 4 * max(e_cpu32, e_seq32[, e_wino32], 2^-23 max|y64|) and the four-sided halo check).

csrc/conv_wino.hip, csrc/conv_pad.hip (direct tiles, K slices, latency form, the row-mode stem, the folded down-sample) and the whole
encoder at 256 x 192-like crops: every WHOLE output tensor is held to the rule, every halo row and column must keep its fill value, and
every bit-equality the square tests of tests/test_gpu_net.py claim is asserted again where H != W.

Worst err / bound per family as the tests printed them on an MI355X with the kernels of commit f95e52c (every test prints a
"worst err/bound" line) -- measured values, not limits; a family above 0.5 would have a thin margin, none has:

    Winograd (conv_wino.hip)            0.183   (2, 32, 32, 128, 128); non-square worst 0.161 at (11, 64, 48, 64, 128)
    direct (conv_pad.hip)               0.450   the direct kernel on the Winograd case (2, 32, 32, 128, 128), linear output;
                                                0.435 at (1, 16, 48, 512, 512); its own case list 0.292 at (1, 33, 64, 64, 128, 1, 2, 0, 1);
                                                K slices and the latency form included
    row-mode stem                       0.318   (1, 18, 44, 18, 64, 7, 2, 3, 3)
    folded down-sample                  0.320   (1, 32, 24, 128, 256, 3), the 3 x 3 / 2 output
    encoder (vs 4 max(e_cpu32, 2^-23))  0.464   (1, 18, 256, 256); non-square worst 0.377 at (1, 18, 192, 256)

No CPU evaluation beyond cpu32, the sequential chain and the Winograd emulation was needed in the bound.
"""
import copy

import pytest
import torch

import conv_scenario as S
from oracle import ref_cpu as O
from hierarchicalprobabilistic3dhuman_amd.resnet import _ConvBN, resnet18
from conftest import maxerr
from devlib import plain_conv

pytestmark = pytest.mark.gpu

FILL = 7.0


def _conv_bn(c, dev, **kw):
    return _ConvBN(copy.deepcopy(c["conv"]).to(dev), copy.deepcopy(c["bn"]).to(dev), **kw)      # (the case's modules stay on the CPU)


def _launch(cb, xp, ipad, c, opad, res_frame, relu, fill=FILL):
    out = torch.full((c["B"], c["Ho"] + 2 * opad, c["Wo"] + 2 * opad, c["Cout"]), fill, device=xp.device)
    cb.padded(xp, ipad, out, opad, residual=res_frame, relu=relu)
    return out


def _inner(out, opad, c):
    return out[:, opad:opad + c["Ho"], opad:opad + c["Wo"]].permute(0, 3, 1, 2)


@pytest.mark.parametrize("cfg", S.WINO_CASES)
def test_winograd_kernel_on_non_square_maps(cfg, dev):
    B, H, W, Cin, Cout = cfg
    c = S.wino_case(cfg)
    cb = _conv_bn(c, dev)
    assert cb.wino_u is not None and cb.winograd_ok(H, W, 1)
    xp = S.frame(S.nhwc(c["x"].to(dev)), 1)
    resh = S.nhwc(c["res"].to(dev))
    worst, worst_direct = 0.0, 0.0
    for opad in (0, 1):
        resf = S.frame(resh, opad)
        name = "wino %s opad %d" % (cfg, opad)
        out = _launch(cb, xp, 1, c, opad, resf, True)
        worst = max(worst, S.check(name, _inner(out, opad, c), c, "res_relu", wino=True))
        S.assert_halo_untouched(out, opad, FILL)
        lin = _launch(cb, xp, 1, c, opad, None, False)
        worst = max(worst, S.check(name, _inner(lin, opad, c), c, "lin", wino=True))
        S.assert_halo_untouched(lin, opad, FILL)
        # the last image alone: the bits it has in the batch
        one_c = dict(c, B=1)
        one = _launch(cb, xp[B - 1:B].contiguous(), 1, one_c, opad, resf[B - 1:B].contiguous(), True)
        assert torch.equal(one[0], out[B - 1]), ("alone", opad)
        one = _launch(cb, xp[B - 1:B].contiguous(), 1, one_c, opad, None, False)
        assert torch.equal(one[0], lin[B - 1]), ("alone, linear", opad)
        if Cin % 32 == 0:                            # the direct kernel on the same input: held to the rule WITHOUT the Winograd evaluation
            cb.use_winograd = False
            try:
                assert not cb.winograd_ok(H, W, 1)
                d = _launch(cb, xp, 1, c, opad, resf, True)
                worst_direct = max(worst_direct, S.check("direct on " + name, _inner(d, opad, c), c, "res_relu"))
                S.assert_halo_untouched(d, opad, FILL)
                d = _launch(cb, xp, 1, c, opad, None, False)
                worst_direct = max(worst_direct, S.check("direct on " + name, _inner(d, opad, c), c, "lin"))
                S.assert_halo_untouched(d, opad, FILL)
            finally:
                cb.use_winograd = True
    print("worst err/bound  winograd  %s  %.3f" % (cfg, worst))
    if Cin % 32 == 0:
        print("worst err/bound  direct  %s  %.3f" % (cfg, worst_direct))


@pytest.mark.parametrize("cfg", S.DIRECT_CASES)
def test_direct_kernel_on_non_square_maps(cfg, dev):
    B, H, W, Cin, Cout, k, s, p, ipad = cfg
    c = S.direct_case(cfg)
    Ho, Wo = c["Ho"], c["Wo"]
    cb = _conv_bn(c, dev)
    cb.use_winograd = False
    xh = S.nhwc(c["x"].to(dev))
    resh = S.nhwc(c["res"].to(dev))
    xp = S.frame(xh, ipad)
    worst = 0.0
    for opad in (0, 1):
        name = "direct %s opad %d" % (cfg, opad)
        out = _launch(cb, xp, ipad, c, opad, S.frame(resh, opad), True)
        worst = max(worst, S.check(name, _inner(out, opad, c), c, "res_relu"))
        S.assert_halo_untouched(out, opad, FILL)
        lin = _launch(cb, xp, ipad, c, opad, None, False)
        worst = max(worst, S.check(name, _inner(lin, opad, c), c, "lin"))
        S.assert_halo_untouched(lin, opad, FILL)
    # the equalities of test_padded_conv_kernel, where H != W
    resf = S.frame(resh, 1)
    try:
        if Cin % 32 == 0:
            for v in (0, 1, 2, 3, 4):
                if v == 4 and Cout != 64:
                    continue
                cb.variant = v
                plain = plain_conv(cb, xh, residual=resh, relu=True)        # same tile / split-K rule on both sides
                out = _launch(cb, xp, ipad, c, 1, resf, True)
                assert torch.equal(out[:, 1:-1, 1:-1], plain), v
                S.assert_halo_untouched(out, 1, FILL)
            cb.variant = 0
            if Cout % 128 == 0:
                chunks = k * k * Cin // 32
                for ks in (2, 4):
                    if chunks % ks == 0:
                        cb.ksplit = ks
                        plain_k = plain_conv(cb, xh, residual=resh, relu=True)
                        out = _launch(cb, xp, ipad, c, 1, resf, True)
                        assert torch.equal(out[:, 1:-1, 1:-1], plain_k), ("split-K", ks)
                        assert torch.equal(out, _launch(cb, xp, ipad, c, 1, resf, True)), ("split-K repeats", ks)
                        worst = max(worst, S.check("direct %s ksplit %d" % (cfg, ks), _inner(out, 1, c), c, "res_relu"))
                cb.ksplit = 0
        for ks in (1, 2, 3, 4, 6, 9, 18):
            if ks > 1 and (Cin % 32 != 0 or (k * k * Cin // 32) % ks != 0):
                continue
            cb.latency, cb.variant, cb.ksplit = False, (3 if Cin % 32 == 0 else 0), ks
            want_k = _launch(cb, xp, ipad, c, 1, resf, True)              # 64 x 64 tiles, two stages (128-row tiles when sliced)
            if ks > 1:
                cb.variant = 0
                assert torch.equal(want_k, _launch(cb, xp, ipad, c, 1, resf, True)), ("64 x 64 tiles, sliced", ks)
            cb.latency, cb.variant = True, 0                              # -> variant 5 through _tile_variant
            got5 = _launch(cb, xp, ipad, c, 1, resf, True)
            assert cb._tile_variant(ks) == 5 and torch.equal(got5, want_k), ("four stages", ks)
            S.assert_halo_untouched(got5, 1, FILL)
            worst = max(worst, S.check("direct %s latency form, %d slices" % (cfg, ks), _inner(got5, 1, c), c, "res_relu"))
    finally:
        cb.latency, cb.variant, cb.ksplit = False, 0, 0
    print("worst err/bound  %s  %s  %.3f" % ("direct" if Cin % 32 == 0 else "row-mode stem", cfg, worst))


@pytest.mark.parametrize("cfg", S.DOWN_CASES)
def test_folded_down_sample_on_non_square_maps(cfg, dev):
    B, H, W, Cin, Cout, k = cfg
    cm, cd = S.down_cases(cfg)
    assert torch.equal(cm["x"], cd["x"]) and (cm["Ho"], cm["Wo"]) == (cd["Ho"], cd["Wo"])
    c1, down = _conv_bn(cm, dev), _conv_bn(cd, dev)
    ipad = k // 2
    xp = S.frame(S.nhwc(cm["x"].to(dev)), ipad)
    assert c1.folds_down(down, H, W, ipad)
    chunks = k * k * Cin // 32
    settings = [(0, 0, False), (1, 0, False), (3, 0, False), (0, 0, True)] + [(0, ks, False) for ks in (2, 4) if chunks % ks == 0] + \
               [(3, ks, False) for ks in (3,) if chunks % ks == 0] + [(0, ks, True) for ks in (9,) if chunks % ks == 0]
    worst = 0.0
    try:
        for variant, ks, latency in settings:
            for cv in (c1, down):
                cv.variant, cv.latency = variant, latency
            c1.ksplit = ks
            sep = _launch(c1, xp, ipad, cm, 1, None, True)
            sep_d = _launch(down, xp, ipad, cd, 1, None, False)
            got, got_d = torch.full_like(sep, FILL), torch.full_like(sep, FILL)
            c1.padded_with_down(xp, ipad, got, 1, down, got_d)
            assert torch.equal(got, sep) and torch.equal(got_d, sep_d), (variant, ks, latency)
            S.assert_halo_untouched(got, 1, FILL)
            S.assert_halo_untouched(got_d, 1, FILL)
            name = "down %s variant %d ks %d latency %d" % (cfg, variant, ks, latency)
            worst = max(worst, S.check(name, _inner(got, 1, cm), cm, "relu"), S.check(name + " (1x1)", _inner(got_d, 1, cd), cd, "lin"))
    finally:
        for cv in (c1, down):
            cv.variant, cv.latency, cv.ksplit = 0, False, 0
    print("worst err/bound  folded down-sample  %s  %.3f" % (cfg, worst))


# ---- the whole encoder ----

@pytest.fixture(scope="module")
def encoder(dev):
    """(device encoder, float64 state dict, fp32 state dict) of resnet18(in_channels=18) with non-trivial BatchNorm statistics."""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(118)
        enc = resnet18(in_channels=18).eval()
        for m in enc.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0.0, 0.1)
                m.running_var.uniform_(0.6, 1.4)
                m.weight.data.uniform_(0.7, 1.3)
                m.bias.data.normal_(0.0, 0.1)
    sd32 = {"image_encoder." + k: v.clone() for k, v in enc.state_dict().items()}
    sd64 = {k: v.double() if v.is_floating_point() else v for k, v in sd32.items()}
    return enc.to(dev), sd64, sd32


def _oracle(encoder, x):
    """(float64 features, max|fp32 oracle - float64|) of the oracle's encoder on x."""
    with torch.no_grad():
        want = O.resnet18_forward(encoder[1], x.double())
        e32 = float((O.resnet18_forward(encoder[2], x).double() - want).abs().max())
    return want, e32


ENCODER_SHAPES = [(2, 18, 256, 192), (1, 18, 192, 256), (3, 18, 256, 128), (1, 18, 128, 512), (1, 18, 256, 256)]


@pytest.mark.parametrize("shape", ENCODER_SHAPES)
def test_encoder_on_non_square_crops(shape, dev, encoder):
    """256 x 192 and its like (and 256 x 256, the control that reaches the 8 x 8 quad form): Winograd stem, conv_wino on layer1 (and on the
    later layers whose maps split into 16 x 16 blocks), the direct kernel on the rest.  Features within 1e-4 max|features| of the float64
    oracle and the Winograd features within 2e-5 of the direct ones (the figures of
    test_winograd_and_direct_encoders_agree_and_are_batch_invariant); the switches' bit-equalities of the square tests; latency mode."""
    enc = encoder[0]
    B = shape[0]
    x = torch.rand(*shape, generator=torch.Generator().manual_seed(sum(shape)))
    extra = torch.rand(2, *shape[1:], generator=torch.Generator().manual_seed(9))
    want, e32 = _oracle(encoder, x)
    scale = float(want.abs().max())
    xd, big = x.to(dev), torch.cat([x, extra]).to(dev)
    assert enc.composite and enc.fold_downsample and enc.fused_pool and enc.stem_reads_nchw
    feats = enc(xd).clone()
    assert feats.shape == (B, 512)
    err = maxerr(feats, want)
    print("worst err/bound  encoder  %s  %.3f   (max|dev - f64| = %.3e, max|cpu32 - f64| = %.3e, max|f64| = %.3e; bound = 4 max(e_cpu32, "
          "2^-23 max|f64|), printed for the record)" % (shape, err / (4 * max(e32, S.EPS32 * scale)), err, e32, scale))
    assert err <= 1e-4 * scale
    try:
        enc.set_winograd(False)
        direct = enc(xd).clone()
        enc.set_winograd(True)
        assert maxerr(direct, want) <= 1e-4 * scale and maxerr(feats, direct) <= 2e-5 * scale
        # one image alone / a larger batch: the same bits per image
        assert torch.equal(enc(xd[B - 1:B]), feats[B - 1:B]) and torch.equal(enc(big)[:B], feats)
        enc.composite = False
        assert torch.equal(enc(xd), feats), "per-layer calls"
        enc.fold_downsample = False
        assert torch.equal(enc(xd), feats), "per-layer calls, down-sample in its own launch"
        enc.composite = True
        assert torch.equal(enc(xd), feats), "down-sample in its own launch"
        enc.fold_downsample = True
        enc.stem_reads_nchw = False
        assert torch.equal(enc(xd), feats), "phase split + frame-fed stem"
        enc.fused_pool = False
        assert torch.equal(enc(xd), feats), "max pool as its own kernel"
        enc.composite = False
        assert torch.equal(enc(xd), feats), "max pool as its own kernel, per-layer calls"
        enc.composite, enc.fused_pool, enc.stem_reads_nchw = True, True, True
        enc.set_latency_mode(True)
        lat = enc(xd).clone()
        assert maxerr(lat, want) <= 1e-4 * scale
        assert torch.equal(enc(xd[B - 1:B]), lat[B - 1:B]) and torch.equal(enc(big)[:B], lat)
        enc.set_latency_mode(False)
        assert torch.equal(enc(xd), feats), "default bits after latency mode"
    finally:
        enc.set_latency_mode(False)
        enc.set_winograd(True)
        enc.composite, enc.fold_downsample, enc.fused_pool, enc.stem_reads_nchw = True, True, True, True


CACHE_SHAPES = [(1, 18, 32, 32), (1, 18, 32, 64), (1, 18, 64, 32), (2, 18, 32, 64), (1, 18, 64, 96), (1, 18, 96, 64), (1, 18, 64, 64)]


def test_frame_cache_keeps_transposed_shapes_apart(dev, encoder):
    """Seven input shapes in turn on one encoder and one stream -- one more than the frame cache holds -- then the first and the third
    again: the same bits as in the first pass, every shape within the oracle tolerance, and an (H, W) / (W, H) pair never shares a frame set."""
    enc = encoder[0]
    enc.invalidate()
    xs = [torch.rand(*s, generator=torch.Generator().manual_seed(sum(s) + 3 * s[2])) for s in CACHE_SHAPES]
    first = []
    for n, (s, x) in enumerate(zip(CACHE_SHAPES, xs)):
        feats = enc(x.to(dev)).clone()
        first.append(feats)
        want, _ = _oracle(encoder, x)
        assert maxerr(feats, want) <= 1e-4 * float(want.abs().max()), s
        frames = enc._frames
        assert len(frames) == (n + 1 if n < 6 else 1)              # the seventh shape starts a new state
        if n in (2, 5):                                            # both members of a transposed pair are resident
            a, b = ([fs for key, fs in frames.items() if key[:4] == t] for t in CACHE_SHAPES[n - 1:n + 1])
            assert len(a) == 1 and len(b) == 1 and a[0] is not b[0]
            assert a[0]["pool"].data_ptr() != b[0]["pool"].data_ptr()
            pa, pb = tuple(a[0]["pool"].shape[1:3]), tuple(b[0]["pool"].shape[1:3])
            assert pa == pb[::-1] and pa != pb
    for n in (0, 2):
        assert torch.equal(enc(xs[n].to(dev)), first[n]), CACHE_SHAPES[n]
    assert len(enc._frames) == 3


def test_hand_edited_layer_gets_a_frame_set_of_its_own(dev, encoder):
    """Fields edited by hand on a prepared layer (layer1.0's first convolution: Winograd off, two K slices over its 18 chunks) select a
    frame set of their own, with the op list and the split-K scratch of the edited state: the bits of a fresh encoder that was edited
    before its first forward, within the Winograd-versus-direct figure of the default ones, and the default bits again once restored."""
    enc = encoder[0]
    enc.invalidate()
    x = torch.rand(1, 18, 32, 32, generator=torch.Generator().manual_seed(41)).to(dev)
    fresh = copy.deepcopy(enc)
    with torch.no_grad():
        default = enc(x).clone()
        n_sets = len(enc._frames)
        cb, cb_fresh = enc._prepared["blocks"][0][0], fresh.prepare()["blocks"][0][0]
        assert cb.winograd_ok(8, 8, 1) and cb.kh * cb.kw * cb.cin_p // 32 == 18
        try:
            cb.use_winograd, cb.ksplit = False, 2
            cb_fresh.use_winograd, cb_fresh.ksplit = False, 2
            edited = enc(x).clone()
            assert len(enc._frames) == n_sets + 1
            assert torch.equal(edited, fresh(x))
            assert maxerr(edited, default) <= 2e-5 * float(default.abs().max())
        finally:
            cb.use_winograd, cb.ksplit = True, 0
        assert torch.equal(enc(x), default)
        assert len(enc._frames) == n_sets + 1
