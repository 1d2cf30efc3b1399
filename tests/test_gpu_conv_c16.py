"""The grouped 16-channel convolution (csrc/conv_c16.hip: hps_conv2d_bn_act_c16) against float64, with the cases, the CPU references,
the accuracy rule and the halo check of tests/conv_scenario.py, unchanged:

    bound = 4 * max(e_cpu32, e_seq32, 2^-23 max|y64|)

Cases (B, H, W, Cin, Cout, k, stride), pad = k // 2: the 48-wide 3x3; an odd map at stride 2; a 1x1 from a 96-wide branch; the masked
Cout = 17 (also as the final layer runs it: scale = 1, shift = bias); fewer pixels than one tile; the minimum shape; the widest
stride-2; the bottleneck's expansion and reduction; the 3-channel stem through the path the module uses (hps_hrnet_pack_input into a
16-channel frame).  Per case the modes res_relu, lin and relu with an output halo of 0 and 1: every WHOLE output is held to the rule,
the halo keeps its fill value, the last image alone has the bits it has in the batch, and two runs are bit-equal.  One grouped
launch holds the first, third, fifth and seventh case: each output bit-equal to its single launch.

All of those launches are small enough for the kernel's narrow tile (16 pixels x 16 channels per wave).  WIDE_CASES are batches of
96 x 72 maps that select the two wide tiles (16 x 64 and 32 x 64) with partly filled channel tiles: held to the same rule, the last
image alone (narrow tile) bit-equal to its place in the batch (wide tile), and one grouped launch of all four (32 x 64) bit-equal to
the four single launches (two of them 16 x 64): an output's bits depend neither on B nor on the tile it lands in.

Worst err / bound as the tests printed them on an MI355X (measured values, not limits; above 0.5 would be a thin margin):

    (1, 9, 12, 48, 48, 3, 1)      0.250        (1, 8, 8, 16, 16, 3, 1)        0.317
    (3, 7, 9, 48, 96, 3, 2)       0.277        (2, 24, 18, 192, 384, 3, 2)    0.288
    (2, 12, 9, 96, 48, 1, 1)      0.237        (1, 16, 12, 64, 256, 1, 1)     0.311
    (1, 18, 24, 48, 17, 1, 1)     0.279        (1, 16, 12, 256, 64, 1, 1)     0.277
    (2, 5, 6, 384, 192, 1, 1)     0.301        (2, 18, 14, 3, 64, 3, 2)       0.201   (the stem)
    final-layer form (scale = 1, shift = bias) of (1, 18, 24, 48, 17, 1, 1)   0.265
    grouped launch                0.301

    wide tiles: (16, 72, 96, 48, 48, 3, 1)  0.464     (6, 72, 96, 96, 48, 1, 1)   0.280
                (16, 72, 96, 48, 17, 1, 1)  0.262     (16, 72, 96, 48, 96, 3, 2)  0.408

No family is above 0.5; the 48-wide 3x3 at batch 16 is the closest (res_relu 0.464: over its 5.3 million outputs the device's worst
error is 4.1 units of 2^-23 max|y64|, the CPU's 2.2 and the sequential chain's, on its 20 000 sampled positions, 2.2).
No CPU evaluation beyond cpu32 and the sequential chain was needed in the bound.
"""
import copy

import pytest
import torch

import conv_scenario as S
from hierarchicalprobabilistic3dhuman_amd import _capi
from hierarchicalprobabilistic3dhuman_amd.pose2D_hrnet import _Layer

pytestmark = pytest.mark.gpu

FILL = 7.0
CASES = [(1, 9, 12, 48, 48, 3, 1), (3, 7, 9, 48, 96, 3, 2), (2, 12, 9, 96, 48, 1, 1), (1, 18, 24, 48, 17, 1, 1), (2, 5, 6, 384, 192, 1, 1),
         (1, 8, 8, 16, 16, 3, 1), (2, 24, 18, 192, 384, 3, 2), (1, 16, 12, 64, 256, 1, 1), (1, 16, 12, 256, 64, 1, 1),
         (2, 18, 14, 3, 64, 3, 2)]
GROUP = [CASES[0], CASES[2], CASES[4], CASES[6]]
# The launch picks its tile from the number of (64 pixel) x (64 channel) tiles t of ALL its problems (csrc/conv_c16.hip): 16 channels
# per wave for t < 512, 64 for t >= 512, and 32 pixels per wave for t > 1024.  Every case above has t < 512; these cross both
# thresholds with output groups that fill their last 64-channel tile only partly (ceil16(Cout) = 48, 32, 96), and their last image
# alone (t = 108 or 216) runs the narrow tile:   case -> t, tile (pixels x channels per wave)
WIDE_CASES = [(16, 72, 96, 48, 48, 3, 1),      # 1728, 32 x 64: the 48-wide 3x3 of the top branch at batch 16
              (6, 72, 96, 96, 48, 1, 1),       #  648, 16 x 64: a 1x1 from a 96-wide map
              (16, 72, 96, 48, 17, 1, 1),      # 1728, 32 x 64: the masked final layer
              (16, 72, 96, 48, 96, 3, 2)]      #  864, 16 x 64: stride 2, two channel tiles, the second half empty


def _case(cfg):
    B, H, W, Cin, Cout, k, s = cfg
    return S.case(B, H, W, Cin, Cout, k, s, k // 2, seed=(CASES + WIDE_CASES).index(cfg))


def _layer(c, dev, bn=None):
    return _Layer(copy.deepcopy(c["conv"]).to(dev), copy.deepcopy(bn if bn is not None else c["bn"]).to(dev))


def _input_frame(c, dev, ipad=1, images=None):
    """The case's input as the kernel reads it; the 3-channel stem goes through the library's pack kernel."""
    x = c["x"] if images is None else c["x"][images]
    if c["Cin"] == 3:
        xd = x.to(dev).contiguous()
        B, _, H, W = xd.shape
        f = torch.zeros(B, H + 2 * ipad, W + 2 * ipad, 16, device=dev)
        _capi.call("hps_hrnet_pack_input", _capi.ptr(xd), _capi.ptr(f), B, H, W, 16, ipad, _capi.stream())
        return f
    return S.frame(S.nhwc(x.to(dev)), ipad)


def _problem(layer, xp, ipad, c, opad, res_frame, relu, fill=FILL):
    B = xp.shape[0]
    out = torch.full((B, c["Ho"] + 2 * opad, c["Wo"] + 2 * opad, c["Cout"]), fill, device=xp.device)
    P = _capi.ptr
    p = _capi.C16Problem(x=P(xp), w=P(layer.w), scale=P(layer.scale), shift=P(layer.shift), residual=P(res_frame), y=P(out), B=B,
                         H=c["H"], W=c["W"], ipad=ipad, Cin=xp.shape[3], Cout=c["Cout"], K=c["k"], stride=c["stride"], opad=opad,
                         relu=1 if relu else 0)
    return p, out


def _run(problems):
    arr = (_capi.C16Problem * len(problems))(*problems)
    _capi.call("hps_conv2d_bn_act_c16", arr, len(problems), _capi.stream())


def _launch(layer, xp, ipad, c, opad, res_frame, relu):
    p, out = _problem(layer, xp, ipad, c, opad, res_frame, relu)
    _run([p])
    return out


def _inner(out, opad, c):
    return out[:, opad:opad + c["Ho"], opad:opad + c["Wo"]].permute(0, 3, 1, 2)


@pytest.mark.parametrize("cfg", CASES)
def test_c16_kernel_against_float64(cfg, dev):
    B, H, W, Cin, Cout, k, s = cfg
    c = _case(cfg)
    layer = _layer(c, dev)
    xp = _input_frame(c, dev)
    resh = S.nhwc(c["res"].to(dev))
    worst = 0.0
    for opad in (0, 1):
        resf = S.frame(resh, opad)
        name = "c16 %s opad %d" % (cfg, opad)
        outs = {}
        for mode in S.MODES:
            res, relu = (resf if mode == "res_relu" else None), mode != "lin"
            out = outs[mode] = _launch(layer, xp, 1, c, opad, res, relu)
            worst = max(worst, S.check(name, _inner(out, opad, c), c, mode))
            S.assert_halo_untouched(out, opad, FILL)
            assert torch.equal(out, _launch(layer, xp, 1, c, opad, res, relu)), ("two runs", mode, opad)
        # the last image alone: the bits it has in the batch
        x1 = _input_frame(c, dev, images=slice(B - 1, B))
        one = _launch(layer, x1, 1, dict(c, B=1), opad, resf[B - 1:B].contiguous(), True)
        assert torch.equal(one[0], outs["res_relu"][B - 1]), ("alone", opad)
        one = _launch(layer, x1, 1, dict(c, B=1), opad, None, False)
        assert torch.equal(one[0], outs["lin"][B - 1]), ("alone, linear", opad)
        if k == 1:                                    # a 1x1 needs no halo: the same bits from a frame without one
            x0 = _input_frame(c, dev, ipad=0)
            assert torch.equal(_launch(layer, x0, 0, c, opad, None, False), outs["lin"]), ("ipad 0", opad)
    print("worst err/bound  c16  %s  %.3f" % (cfg, worst))


def test_c16_final_layer_form_scale_one_shift_bias(dev):
    """The masked Cout = 17 case as the final layer runs it: a convolution with a bias and no BatchNorm, scale = 1, shift = bias.
    References by conv_scenario's own functions on the case with an identity BatchNorm that carries the bias."""
    cfg = CASES[3]
    c = _case(cfg)
    bias = torch.randn(c["Cout"], generator=torch.Generator().manual_seed(17)) * 0.1
    bn = torch.nn.BatchNorm2d(c["Cout"]).eval()
    bn.eps = 0.0                                       # var 1, mean 0, weight 1: the fold is exactly (1, bias)
    bn.bias.data.copy_(bias)
    c2 = dict(c, bn=bn)
    scale, shift = S.fold_bn(bn)
    assert bool((scale == 1).all()) and torch.equal(shift, bias)
    conv = copy.deepcopy(c["conv"])
    conv.bias = torch.nn.Parameter(bias.clone(), requires_grad=False)
    layer = _Layer(copy.deepcopy(conv).to(dev), None)
    assert bool((layer.scale == 1).all()) and torch.equal(layer.shift.cpu(), bias)
    with torch.no_grad():
        y64 = copy.deepcopy(conv).double()(c["x"].double())
        y32 = conv(c["x"])
        idx = S.sample_positions(c2)
        seq = S.seq32_lin(c2, idx)
    scale64 = float(y64.abs().max())
    e_cpu32 = float((y32.double() - y64).abs().max())
    e_seq32 = float((seq.double() - y64.reshape(-1)[idx]).abs().max())
    bound = 4.0 * max(e_cpu32, e_seq32, S.EPS32 * scale64)
    xp = _input_frame(c, dev)
    for opad in (0, 1):
        out = _launch(layer, xp, 1, c, opad, None, False)
        err = float((_inner(out, opad, c).cpu().double() - y64).abs().max())
        print("c16 final-layer form %s opad %d  max|dev - f64| = %.3e  cpu32 %.3e  seq32 %.3e  err/bound = %.3f"
              % (cfg, opad, err, e_cpu32, e_seq32, err / bound))
        assert err <= bound
        S.assert_halo_untouched(out, opad, FILL)
    print("worst err/bound  c16 final-layer form  %s  %.3f" % (cfg, err / bound))


def test_c16_grouped_launch_has_the_bits_of_the_single_launches(dev):
    problems, outs, singles, keep = [], [], [], []
    for cfg in GROUP:
        c = _case(cfg)
        layer = _layer(c, dev)
        xp = _input_frame(c, dev)
        resf = S.frame(S.nhwc(c["res"].to(dev)), 1)
        keep.append((layer, xp, resf))
        singles.append(_launch(layer, xp, 1, c, 1, resf, True))
        p, out = _problem(layer, xp, 1, c, 1, resf, True)
        problems.append(p)
        outs.append(out)
    _run(problems)
    worst = 0.0
    for cfg, out, single in zip(GROUP, outs, singles):
        assert torch.equal(out, single), cfg
        S.assert_halo_untouched(out, 1, FILL)
        worst = max(worst, S.check("c16 grouped %s" % (cfg,), _inner(out, 1, _case(cfg)), _case(cfg), "res_relu"))
    # a group in another order and of another size: the same bits again
    p2, o2 = zip(*[_problem(k[0], k[1], 1, _case(cfg), 1, k[2], True) for cfg, k in list(zip(GROUP, keep))[::-1][:3]])
    _run(list(p2))
    for out, single in zip(o2, singles[::-1][:3]):
        assert torch.equal(out, single)
    print("worst err/bound  c16 grouped  %.3f" % worst)


@pytest.fixture(scope="module")
def wide(dev):
    """Per wide case: (case, layer, input frame, residual frame, res_relu output of the single launch), output halo 1."""
    out = []
    for cfg in WIDE_CASES:
        c = _case(cfg)
        layer, xp = _layer(c, dev), _input_frame(c, dev)
        resf = S.frame(S.nhwc(c["res"].to(dev)), 1)
        out.append((c, layer, xp, resf, _launch(layer, xp, 1, c, 1, resf, True)))
    return out


@pytest.mark.parametrize("i", range(len(WIDE_CASES)))
def test_c16_wide_tiles_against_float64_and_the_narrow_tile(i, wide, dev):
    cfg = WIDE_CASES[i]
    c, layer, xp, resf, out = wide[i]
    B = cfg[0]
    name = "c16 wide %s" % (cfg,)
    worst = S.check(name, _inner(out, 1, c), c, "res_relu")
    S.assert_halo_untouched(out, 1, FILL)
    lin = _launch(layer, xp, 1, c, 0, None, False)
    worst = max(worst, S.check(name, _inner(lin, 0, c), c, "lin"))
    assert torch.equal(out, _launch(layer, xp, 1, c, 1, resf, True)), "two runs"
    # the last image alone runs the narrow tile: the bits it has in the batch
    one = _launch(layer, xp[B - 1:B].contiguous(), 1, dict(c, B=1), 1, resf[B - 1:B].contiguous(), True)
    assert torch.equal(one[0], out[B - 1]), "alone (narrow tile) != in the batch (wide tile)"
    one = _launch(layer, xp[B - 1:B].contiguous(), 1, dict(c, B=1), 0, None, False)
    assert torch.equal(one[0], lin[B - 1]), "alone, linear"
    print("worst err/bound  c16 wide  %s  %.3f" % (cfg, worst))


def test_c16_wide_grouped_launch_has_the_bits_of_the_single_launches(wide, dev):
    problems, outs = zip(*[_problem(layer, xp, 1, c, 1, resf, True) for c, layer, xp, resf, _ in wide])
    _run(list(problems))
    for cfg, out, (_, _, _, _, single) in zip(WIDE_CASES, outs, wide):
        assert torch.equal(out, single), cfg
        S.assert_halo_untouched(out, 1, FILL)
    # ... and a small problem riding in a large launch: the first narrow case beside the first wide one
    c0 = _case(CASES[0])
    layer0, xp0 = _layer(c0, dev), _input_frame(c0, dev)
    res0 = S.frame(S.nhwc(c0["res"].to(dev)), 1)
    alone = _launch(layer0, xp0, 1, c0, 1, res0, True)
    p0, o0 = _problem(layer0, xp0, 1, c0, 1, res0, True)
    pw, ow = _problem(wide[0][1], wide[0][2], 1, wide[0][0], 1, wide[0][3], True)
    _run([p0, pw])
    assert torch.equal(o0, alone) and torch.equal(ow, wide[0][4])
