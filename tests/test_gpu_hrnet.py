"""pose2D_hrnet.PoseHighResolutionNet on the device against tests/hrnet_scenario.forward64 (float64, CPU).

    fuse kernel      four terms with shifts 0, 1, 2, 3 on a 16 x 24 map, bound 4 * 2^-23 * sum_j max|term_j|, halo untouched
    SMALL, NARROW    heat maps within 4 * max(e_cpu32, 2^-23 max|y64|), e_cpu32 from forward64 on fp32 tensors (no other CPU
                     evaluation is in the family); an image has the same bits alone and in a larger batch; shapes run in turn keep
                     their bits; load_state_dict takes effect; SMALL again at batch 64, where the launches select the kernel's wide tiles,
                     every image bit-equal to what it is alone and in smaller batches
    W48              the full network at (1, 3, 384, 288): the same rule, and the key points of all 17 joints equal those of the
                     float64 heat maps -- under the precondition, asserted on the CPU side, that every joint's two largest float64
                     values are at least 8 bounds apart
    predict_hrnet    the device W48 model behind predict_hrnet.predict_hrnet (no person detector) on a seeded (3, 200, 150) image:
                     joints2D equal those of forward64 on the same crop, joints2Dconfs within the bound

Worst err / bound as the tests printed them on an MI355X (measured values, not limits; above 0.5 would be a thin margin):

    fuse kernel                        0.079
    SMALL  (2, 3, 64, 96)              0.428   ((1, 3, 32, 32): 0.404; second state dict: 0.289)
    SMALL  (64, 3, 64, 96)             0.359   the wide tiles of csrc/conv_c16.hip
    NARROW (1, 3, 32, 64)              0.391   ((1, 3, 32, 32): 0.353; second state dict: 0.323)
    W48    (1, 3, 384, 288)            0.431   (max|dev - f64| = 7.7e-6 at max|y64| = 5.5; cpu32 is 6.9 units of 2^-23 max|y64|,
                                               the device 11.9); smallest top-2 gap = 97 bounds
    predict_hrnet confidences          0.090   smallest top-2 gap = 48 bounds

No family is above 0.5; the networks sit at 0.39 .. 0.43, the deepest (W48) highest.
"""
import ctypes

import pytest
import torch

import conv_scenario as CS
import hrnet_scenario as S
from hierarchicalprobabilistic3dhuman_amd import _capi, predict_hrnet
from hierarchicalprobabilistic3dhuman_amd.pose2D_hrnet import PoseHighResolutionNet

pytestmark = pytest.mark.gpu

FILL = 7.0


def test_fuse_kernel_against_float64(dev):
    B, H, W, C = 2, 16, 24, 48
    g = torch.Generator().manual_seed(11)
    terms = [torch.randn(B, H >> s, W >> s, C, generator=g) * (1.0 + s) for s in range(4)]
    want = torch.zeros(B, H, W, C, dtype=torch.float64)
    for s, t in enumerate(terms):
        want += t.double().repeat_interleave(1 << s, dim=1).repeat_interleave(1 << s, dim=2)
    want = want.clamp_min(0)
    bound = 4.0 * S.EPS32 * sum(float(t.abs().max()) for t in terms)
    frames = [CS.frame(t.to(dev), 1, fill=FILL) for t in terms]            # a term's halo is never read
    worst = 0.0
    for opad in (0, 1):
        out = torch.full((B, H + 2 * opad, W + 2 * opad, C), FILL, device=dev)
        a = _capi.HrnetFuseArgs(n_terms=4, y=_capi.ptr(out), opad=opad, B=B, H=H, W=W, C=C, relu=1)
        for k, f in enumerate(frames):
            a.term[k], a.shift[k], a.pad[k] = f.data_ptr(), k, 1
        _capi.call("hps_hrnet_fuse", ctypes.byref(a), _capi.stream())
        got = out[:, opad:opad + H, opad:opad + W].cpu().double()
        err = float((got - want).abs().max())
        print("fuse opad %d  max|dev - f64| = %.3e  bound %.3e  err/bound = %.3f" % (opad, err, bound, err / bound))
        assert err <= bound
        CS.assert_halo_untouched(out, opad, FILL)
        worst = max(worst, err / bound)
    print("worst err/bound  fuse  %.3f" % worst)


def _net(name, sd, dev):
    net = PoseHighResolutionNet(S.config(name)).eval()
    net.load_state_dict(sd, strict=True)
    return net.to(dev)


@pytest.mark.parametrize("name", ["SMALL", "NARROW"])
def test_small_networks_against_float64(name, dev):
    shape = S.GOLDEN_INPUTS[name]
    shapes = S.shapes_of(PoseHighResolutionNet(S.config(name)).state_dict())
    sd, x, y64, y32 = S.references(name, shape, 0, S.shapes_key(shapes))
    net = _net(name, sd, dev)
    xd = x.to(dev)
    y = net(xd)
    assert y.shape == y64.shape and y.dtype == torch.float32 and y.is_contiguous()
    worst = S.check("%s %s" % (name, shape), y, y64, y32)
    # batch invariance: the last image alone, and the batch with two more images behind it
    B = shape[0]
    assert torch.equal(net(xd[B - 1:]), y[B - 1:])
    more = torch.cat([xd, S.seeded_input((2,) + shape[1:], 5).to(dev)])
    assert torch.equal(net(more)[:B], y)
    # another input shape in between: the first one's frames and plan still give the same bits
    other = S.seeded_input((1, 3, 32, 32), 6)
    y_other = net(other.to(dev))
    assert torch.equal(net(xd), y) and torch.equal(net(other.to(dev)), y_other)
    with torch.no_grad():
        worst = max(worst, S.check("%s (1, 3, 32, 32)" % name, y_other, S.forward64(sd, S.config(name), other.double()),
                                   S.forward64(sd, S.config(name), other)))
    # new weights take effect
    sd2 = S.seeded_state_dict(shapes, 1)
    net.load_state_dict(sd2, strict=True)
    with torch.no_grad():
        y64b, y32b = S.forward64(sd2, S.config(name), x.double()), S.forward64(sd2, S.config(name), x)
    yb = net(xd)
    assert not torch.equal(yb, y)
    worst = max(worst, S.check("%s second state dict" % name, yb, y64b, y32b))
    print("worst err/bound  hrnet %s  %.3f" % (name, worst))


def test_small_network_at_a_batch_that_selects_the_wide_tiles(dev):
    """SMALL at (64, 3, 64, 96), by the number t of (64 pixel x 64 channel) tiles of a launch (csrc/conv_c16.hip): conv1 and layer1's
    64 -> 256 convolutions have t = 1536 or more and run the 32 x 64 tile, the launches of the stages' branches and fuse paths have
    t = 576 .. 684 and run 16 x 64 with partly filled channel tiles (widths 48 and 96), the rest run 16 x 16; at (2, 3, 64, 96) and
    below every launch runs 16 x 16.  Same rule; and an image's bits do not depend on the tiles its batch selects."""
    name, B = "SMALL", 64
    shapes = S.shapes_of(PoseHighResolutionNet(S.config(name)).state_dict())
    sd = S.references(name, S.GOLDEN_INPUTS[name], 0, S.shapes_key(shapes))[0]
    x = S.seeded_input((B, 3, 64, 96), 7)
    with torch.no_grad():
        y64, y32 = S.forward64(sd, S.config(name), x.double()), S.forward64(sd, S.config(name), x)
    net = _net(name, sd, dev)
    xd = x.to(dev)
    y = net(xd)
    worst = S.check("SMALL (64, 3, 64, 96)", y, y64, y32)
    assert torch.equal(net(xd[B - 1:]), y[B - 1:]), "alone (narrow tiles) != in the batch (wide tiles)"
    assert torch.equal(net(xd[:2]), y[:2]) and torch.equal(net(xd[:16]), y[:16])
    assert torch.equal(net(xd), y)
    print("worst err/bound  hrnet SMALL batch 64  %.3f" % worst)


@pytest.fixture(scope="module")
def w48(dev):
    import json
    import os
    keys = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hrnet_w48_keys.json")))
    shapes = {k: (tuple(s), d) for k, s, d in keys}
    sd, x, y64, y32 = S.references("W48", (1, 3, 384, 288), S.W48_SEED, S.shapes_key(shapes))
    return _net("W48", sd, dev), sd, x, y64, y32


def _assert_gaps(y64, bound):
    gaps = S.top2_gap(y64)
    print("top-2 gaps: min %.3e over %d joints, bound %.3e, min gap / bound = %.1f" % (float(gaps.min()), gaps.numel(), bound,
                                                                                      float(gaps.min()) / bound))
    assert gaps.numel() == 17 and float(gaps.min()) >= 8 * bound, "precondition: pick another seed (hrnet_scenario.W48_SEED)"


def test_w48_full_size_against_float64(w48, dev):
    net, sd, x, y64, y32 = w48
    bound = S.bound(y64, y32)[0]
    _assert_gaps(y64, bound)                                      # CPU side only
    y = net(x.to(dev))
    assert y.shape == (1, 17, 96, 72)
    worst = S.check("W48 (1, 3, 384, 288)", y, y64, y32)
    kp, conf = predict_hrnet.get_kp_locations_confs_from_heatmaps(y)
    kp64, conf64 = predict_hrnet.get_kp_locations_confs_from_heatmaps(y64)
    assert torch.equal(kp.cpu().double(), kp64.double())
    assert float((conf.cpu().double() - conf64).abs().max()) <= bound
    print("W48 launches per forward: %d" % net.launches_per_forward(1, 384, 288, dev))
    print("worst err/bound  hrnet W48  %.3f" % worst)


def test_predict_hrnet_with_the_device_model(w48, dev):
    net, sd, _, _, _ = w48
    cfg = S.config("W48")
    image = torch.rand(3, 200, 150, generator=torch.Generator().manual_seed(21)).to(dev)
    with torch.no_grad():
        out = predict_hrnet.predict_hrnet(net, cfg, image, object_detect_model=None)
    crop = out["cropped_image"]
    assert crop.shape == (3, 384, 288)
    # the float64 CPU front end: the same crop, normalised as predict_hrnet normalises it, into forward64
    mean = torch.tensor(predict_hrnet._IMAGENET_MEAN, device=dev)[:, None, None]
    std = torch.tensor(predict_hrnet._IMAGENET_STD, device=dev)[:, None, None]
    xin = ((crop - mean) / std)[None].cpu()
    with torch.no_grad():
        y64, y32 = S.forward64(sd, cfg, xin.double()), S.forward64(sd, cfg, xin)
    bound = S.bound(y64, y32)[0]
    _assert_gaps(y64, bound)
    kp64, conf64 = predict_hrnet.get_kp_locations_confs_from_heatmaps(y64)
    want = kp64[0].double() * (cfg.MODEL.IMAGE_SIZE[0] / cfg.MODEL.HEATMAP_SIZE[0])
    assert out["joints2D"].shape == (17, 2) and torch.equal(out["joints2D"].cpu().double(), want)
    err = float((out["joints2Dconfs"].cpu().double() - conf64[0]).abs().max())
    print("predict_hrnet confidences: max|dev - f64| = %.3e  bound %.3e  err/bound = %.3f" % (err, bound, err / bound))
    assert err <= bound
    print("worst err/bound  predict_hrnet confs  %.3f" % (err / bound))
