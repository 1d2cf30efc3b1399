"""GPU: hps_bottleneck_expand_down (csrc/conv_expand_down.hip) alone through the C ABI.  Contract: every output has the bits of

    hps_conv2d_bn_act_pad(x, w_d, ..., stride, relu = 0)            -> d
    hps_conv2d_bn_act_pad(t, w_3, ..., residual = d, relu = 1)

with the same tile variant.  Operands are tests/conv_scenario.py's seeded cases (convolution + eval BatchNorm with non-trivial
statistics, negative scales on odd seeds); the halos of both input frames hold NaN (a 1x1 window never reads them), the output
frame's halo and a guard band on either side of it hold NaN before the call and after it.  So that the identity is not an identity
of two wrong answers, the two launches of case 2 are held to float64 by conv_scenario's rule: the down-sample's launch by
conv_scenario.check itself, and the pair by the same rule on the block's own float64 evaluation
relu(bn3(conv3(t)) + bn_d(conv_d(x))): bound = 4 max(e_cpu32, e_seq32, 2^-23 max|y64|), e_seq32 from conv_scenario.seq32_lin of
both convolutions.

Measured on an MI355X: 0 outputs differ in all 16 (case, variant, halo) combinations; the two launches of case 2 lie at 0.21
(down-sample) and 0.22 (pair) of the float64 bound in every variant."""
import pytest
import torch
import torch.nn.functional as F

import conv_scenario as CS
from hierarchicalprobabilistic3dhuman_amd import _capi
from hierarchicalprobabilistic3dhuman_amd.resnet import _ConvBN

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD = 4096          # floats on either side of the output frame
# B, H, W, stride, Cmid, Cin, Cout, variants, (tpad, xpad, opad) choices
CASES = {
    1: (1, 5, 5, 2, 32, 64, 128, (2, 3), ((1, 0, 1), (0, 1, 0))),                    # one partial tile
    2: (3, 6, 10, 1, 64, 32, 256, (1, 2, 3, 5), ((0, 1, 1), (1, 1, 0))),             # K loops of unequal length either way; non-square; M tiles with a tail
    3: (2, 8, 8, 2, 128, 256, 512, (1,), ((1, 1, 1), (1, 0, 0))),
    4: (1, 16, 16, 1, 64, 64, 256, (0,), ((1, 1, 1), (0, 0, 0))),                    # layer1's entry block
}


def operands(n, dev):
    """(main, down, cb3, cbd): conv_scenario's cases of the expand convolution (its input is t) and of the down-sample (its input is the
    block's input x), and their kernel-side forms on the device."""
    B, H, W, s, Cmid, Cin, Cout = CASES[n][:7]
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    main, down = CS.case(B, Ho, Wo, Cmid, Cout, 1, 1, 0, seed=2 * n), CS.case(B, H, W, Cin, Cout, 1, s, 0, seed=2 * n + 1)
    assert (down["Ho"], down["Wo"]) == (Ho, Wo) == (main["Ho"], main["Wo"])
    dv = lambda m: m.to(dev)
    import copy
    cb3 = _ConvBN(dv(copy.deepcopy(main["conv"])), dv(copy.deepcopy(main["bn"])))
    cbd = _ConvBN(dv(copy.deepcopy(down["conv"])), dv(copy.deepcopy(down["bn"])))
    return main, down, cb3, cbd


def guarded(B, Ho, Wo, C, opad, dev):
    """(buffer, frame): a NaN-filled flat buffer and the (B, Ho + 2 opad, Wo + 2 opad, C) frame in its middle."""
    n = B * (Ho + 2 * opad) * (Wo + 2 * opad) * C
    buf = torch.full((n + 2 * GUARD,), NAN, device=dev)
    return buf, buf[GUARD:GUARD + n].view(B, Ho + 2 * opad, Wo + 2 * opad, C)


def untouched(buf, frame, opad):
    assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all()), "the guard band has been written"
    if opad:
        for side in (frame[:, :opad], frame[:, -opad:], frame[:, :, :opad], frame[:, :, -opad:]):
            assert bool(torch.isnan(side).all()), "the halo has been written"
    inner = frame[:, opad:frame.shape[1] - opad, opad:frame.shape[2] - opad]
    assert bool(torch.isfinite(inner).all())
    return inner


def two_launches(n, pads, variant, dev, ops=None):
    """(d, y, buffers): the down-sample's frame and the block's output by two hps_conv2d_bn_act_pad calls."""
    B, H, W, s, Cmid, Cin, Cout = CASES[n][:7]
    tpad, xpad, opad = pads
    main, down, cb3, cbd = ops or operands(n, dev)
    Ho, Wo = main["Ho"], main["Wo"]
    t = CS.frame(CS.nhwc(main["x"]), tpad, NAN).to(dev)
    x = CS.frame(CS.nhwc(down["x"]), xpad, NAN).to(dev)
    P, st = _capi.ptr, _capi.stream()
    dbuf, d = guarded(B, Ho, Wo, Cout, opad, dev)
    ybuf, y = guarded(B, Ho, Wo, Cout, opad, dev)
    _capi.call("hps_conv2d_bn_act_pad", P(x), P(cbd.wn), P(cbd.scale), P(cbd.shift), None, P(d), B, H, W, xpad, Cin, Cout, 1, 1, s, 0, opad, 0,
               0, variant, 1, None, st)
    # (the residual's halo and guard band stay NaN: they are never read either)
    _capi.call("hps_conv2d_bn_act_pad", P(t), P(cb3.wn), P(cb3.scale), P(cb3.shift), P(d), P(y), B, Ho, Wo, tpad, Cmid, Cout, 1, 1, 1, 0, opad,
               1, 0, variant, 1, None, st)
    return t, x, untouched(dbuf, d, opad), untouched(ybuf, y, opad)


@pytest.mark.parametrize("n,variant,pads", [(n, v, p) for n, c in CASES.items() for v in c[7] for p in c[8]])
def test_every_output_has_the_bits_of_the_two_launches(dev, n, variant, pads):
    B, H, W, s, Cmid, Cin, Cout = CASES[n][:7]
    tpad, xpad, opad = pads
    ops = operands(n, dev)
    main, down, cb3, cbd = ops
    t, x, d, want = two_launches(n, pads, variant, dev, ops)
    Ho, Wo = main["Ho"], main["Wo"]
    P = _capi.ptr
    runs = []
    for _ in range(2):                                         # a second call repeats the bits
        buf, y = guarded(B, Ho, Wo, Cout, opad, dev)
        _capi.call("hps_bottleneck_expand_down", P(t), P(cb3.wn), P(cb3.scale), P(cb3.shift), P(x), P(cbd.wn), P(cbd.scale), P(cbd.shift), P(y),
                   B, H, W, s, tpad, xpad, opad, Cmid, Cin, Cout, variant, 1, _capi.stream())
        runs.append(untouched(buf, y, opad))
    differ = int((runs[0] != want).sum())
    print("case %d variant %d pads %s: %d of %d outputs differ from the two launches, max|diff| = %.3e; zeros after the ReLU: %.3f"
          % (n, variant, pads, differ, want.numel(), float((runs[0] - want).abs().max()), float((want == 0).float().mean())))
    assert torch.equal(runs[0], want)
    assert torch.equal(runs[1], runs[0])
    assert 0.05 < float((want == 0).float().mean()) < 0.95     # the ReLU cuts, and not everything


def test_the_two_launches_of_case_2_against_float64(dev):
    """The yardstick of the bit identity is itself right: the down-sample's launch by conv_scenario.check ("lin"), the pair by the same
    rule on relu(bn3(conv3(t)) + bn_d(conv_d(x))) in float64.
    Measured err / bound, the same in variants 1, 2, 3 and 5: down-sample 0.210, pair 0.221 (0.96 units of 2^-23 max|y64|)."""
    import copy
    n, pads = 2, (0, 1, 1)
    main, down, _, _ = operands(n, dev)
    for variant in CASES[n][7]:
        _, _, d, y = two_launches(n, pads, variant, dev)
        CS.check("case 2 down-sample, variant %d" % variant, d.permute(0, 3, 1, 2), down, "lin")
        lin = lambda c, dt: copy.deepcopy(c["bn"]).to(dt)(copy.deepcopy(c["conv"]).to(dt)(c["x"].to(dt)))
        with torch.no_grad():
            y64 = F.relu(lin(main, torch.float64) + lin(down, torch.float64))
            y32 = F.relu(lin(main, torch.float32) + lin(down, torch.float32))
            idx = CS.sample_positions(main)
            seq = F.relu(CS.seq32_lin(main, idx) + CS.seq32_lin(down, idx))
        scale = float(y64.abs().max())
        e_cpu32 = float((y32.double() - y64).abs().max())
        e_seq32 = float((seq.double() - y64.reshape(-1)[idx]).abs().max())
        bound = 4.0 * max(e_cpu32, e_seq32, CS.EPS32 * scale)
        err = float((y.permute(0, 3, 1, 2).cpu().double() - y64).abs().max())
        u = CS.EPS32 * scale
        print("case 2 pair, variant %d: max|dev - f64| = %.3e  max|y64| = %.3e  in 2^-23 max|y64|: dev %.2f  cpu32 %.2f  seq32 %.2f  err/bound = %.3f"
              % (variant, err, scale, err / u, e_cpu32 / u, e_seq32 / u, err / bound))
        assert err == err and err <= bound, (variant, err, bound)
