"""The Winograd kernel's item loop (csrc/conv_wino.hip: one VALU run per chunk, the peeled first chunk on a zero C operand, an
epilogue of wave-uniform branches) against the loop and epilogue it replaced, which the dev library keeps as ablate = 50
(conv_wino_earlier_kernel, csrc/conv_wino_dev.hip): the same
products and sums in the same order, so EQUAL bits -- halo included -- and, independently, within 1e-5 of the output scale of a float64
direct convolution (the tolerance of test_gpu_net.py::test_winograd_conv_kernel).

Cases (the smallest that reach each path):
  * B = 1, 16 x 16, 64 -> 64: one item of eight chunks -- the peeled first chunk, the steady loop, the drain and the last chunk once each;
  * B = 3, 32 x 16, 64 -> 128: a non-square map, two output-channel groups, an odd batch; residual + ReLU and neither;
  * B = 4, 32 x 32, 64 -> 64 = 16 items on THREE workgroups (ablate = 3000 + ablation): they own 6, 5 and 5 items, so the next item's DMAs
    are issued before an item's epilogue five times per workgroup;
  * quad geometry, B = 5, 8 x 8, 128 -> 64 in two K slices (hps_dev_wino_quad_ksplit): the second quad holds one live image; the raw
    partial sums and the output after wino_splitk_epilogue_kernel.
"""
import pytest
import torch
import torch.nn.functional as F

from hierarchicalprobabilistic3dhuman_amd import _capi
from hierarchicalprobabilistic3dhuman_amd.resnet import _ConvBN
from conftest import maxerr

pytestmark = pytest.mark.gpu

P = _capi.ptr
PARENT = 50            # include/hps_dev.h: the eight-wave form with the earlier item loop and epilogue
FILL = 7.0
_CASES = {}


def _case(cfg, dev):
    """Inputs, the device layer and the float64 references of (B, H, W, Cin, Cout); built once per configuration and left unchanged."""
    if cfg in _CASES:
        return _CASES[cfg]
    B, H, W, Cin, Cout = cfg
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(1000 + sum(cfg))
        conv = torch.nn.Conv2d(Cin, Cout, 3, 1, 1, bias=False)
        bn = torch.nn.BatchNorm2d(Cout).eval()
        bn.running_mean.normal_(); bn.running_var.uniform_(0.5, 2); bn.weight.data.uniform_(0.5, 1.5); bn.bias.data.normal_()
        x = torch.randn(B, Cin, H, W)
        res = torch.randn(B, Cout, H, W)
    with torch.no_grad():
        raw = F.conv2d(x.double(), conv.weight.double(), padding=1)
        g = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
        lin = raw * g[None, :, None, None] + (bn.bias.double() - bn.running_mean.double() * g)[None, :, None, None]
        res_relu = torch.relu(lin + res.double())
    cb = _ConvBN(conv.to(dev), bn.to(dev))
    assert cb.wino_u is not None
    xp = F.pad(x.to(dev).permute(0, 2, 3, 1), (0, 0, 1, 1, 1, 1)).contiguous()
    resf = F.pad(res.to(dev).permute(0, 2, 3, 1), (0, 0, 1, 1, 1, 1)).contiguous()
    _CASES[cfg] = dict(cb=cb, xp=xp, resf=resf, raw=raw, lin=lin, res_relu=res_relu)
    return _CASES[cfg]


def _run(c, cfg, fused, ablate=None, slices=1):
    """One launch into a frame of FILL (opad = 1).  ablate None: the product library's entry point; else the dev library's, with that
    ablation.  Returns (output frame, K-slice workspace or None)."""
    B, H, W, Cin, Cout = cfg
    out = torch.full((B, H + 2, W + 2, Cout), FILL, device=c["xp"].device)
    ws = torch.full((slices, B, 8, 8, Cout), FILL, device=out.device) if H == 8 and W == 8 else None
    cb = c["cb"]
    args = (P(c["xp"]), P(cb.wino_u), P(cb.scale), P(cb.shift), P(c["resf"]) if fused else None, P(out), B, H, W, 1, Cin, Cout, 1,
            1 if fused else 0, P(ws))
    if ablate is None:
        _capi.call("hps_conv3x3_winograd", *args, _capi.stream())
    else:
        with _capi.dev_library():
            _capi.call("hps_dev_conv3x3_winograd", *args, ablate, _capi.stream())
    torch.cuda.synchronize()
    return out, ws


def _check_f64(out, c, fused, what):
    want = c["res_relu"] if fused else c["lin"]
    err = maxerr(out[:, 1:-1, 1:-1].permute(0, 3, 1, 2), want)
    scale = max(1.0, float(want.abs().max()))
    print("%s: max|dev - f64| = %.3e = %.3f of the bound 1e-5 x %.3g" % (what, err, err / (1e-5 * scale), scale))
    assert err <= 1e-5 * scale, what
    halo = torch.cat([out[:, 0].flatten(), out[:, -1].flatten(), out[:, :, 0].flatten(), out[:, :, -1].flatten()])
    assert bool((halo == FILL).all()), what + ": halo written"


@pytest.mark.parametrize("fused", [True, False], ids=["residual+relu", "linear"])
@pytest.mark.parametrize("cfg", [(1, 16, 16, 64, 64), (3, 32, 16, 64, 128)])
def test_item_loop_has_the_bits_of_the_earlier_one(cfg, fused, dev):
    c = _case(cfg, dev)
    got, _ = _run(c, cfg, fused)
    parent, _ = _run(c, cfg, fused, ablate=PARENT)
    assert torch.equal(got, parent)
    assert torch.equal(_run(c, cfg, fused, ablate=0)[0], parent)           # the dev library's copy of the product form
    _check_f64(got, c, fused, "%s fused=%d" % (cfg, fused))


@pytest.mark.parametrize("fused", [True, False], ids=["residual+relu", "linear"])
def test_item_hand_over_on_three_workgroups(fused, dev):
    cfg = (4, 32, 32, 64, 64)                                               # 4 images x 4 blocks of 16 x 16 pixels x 1 channel group = 16 items
    c = _case(cfg, dev)
    full, _ = _run(c, cfg, fused)                                           # the product: one item per workgroup
    got, _ = _run(c, cfg, fused, ablate=3000)                               # include/hps_dev.h: 1000 x the cap on the grid + the ablation
    parent, _ = _run(c, cfg, fused, ablate=3000 + PARENT)
    assert torch.equal(got, parent)
    assert torch.equal(got, full)                                           # nor do the bits depend on which workgroup owns an item
    _check_f64(got, c, fused, "%s on 3 workgroups fused=%d" % (cfg, fused))


@pytest.mark.parametrize("fused", [True, False], ids=["residual+relu", "linear"])
def test_quad_geometry_in_two_k_slices(fused, dev):
    cfg = (5, 8, 8, 128, 64)
    c = _case(cfg, dev)
    with _capi.dev_library():
        try:
            _capi.call("hps_dev_wino_quad_ksplit", 2)
            got, ws = _run(c, cfg, fused, ablate=0, slices=2)
            parent, ws_parent = _run(c, cfg, fused, ablate=PARENT, slices=2)
        finally:
            _capi.call("hps_dev_wino_quad_ksplit", 0)
    assert torch.equal(ws, ws_parent)                                       # the raw partial sums Y of both slices, all five images
    assert not bool((ws == FILL).any())
    assert torch.equal(got, parent)
    raw_err = maxerr(ws.sum(0).permute(0, 3, 1, 2), c["raw"])
    raw_scale = max(1.0, float(c["raw"].abs().max()))
    print("raw partial sums: max|slice 0 + slice 1 - f64| = %.3e = %.3f of the bound" % (raw_err, raw_err / (1e-5 * raw_scale)))
    assert raw_err <= 1e-5 * raw_scale
    _check_f64(got, c, fused, "%s two K slices fused=%d" % (cfg, fused))
    # the product's own rule for this layer (one slice), through the product library
    one, ws_one = _run(c, cfg, fused)
    one_parent, ws_one_parent = _run(c, cfg, fused, ablate=PARENT)
    assert torch.equal(one, one_parent) and torch.equal(ws_one, ws_one_parent)
    _check_f64(one, c, fused, "%s one K slice fused=%d" % (cfg, fused))
