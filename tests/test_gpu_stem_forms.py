"""The dev library's stem entries (include/hps_dev.h: hps_dev_stem_winograd, hps_dev_stem_winograd_pooled_nchw; csrc/stem_wino_dev.hip)
against the product's (csrc/stem_wino.hip).

  * ablate = 0 is the product's own launcher: EQUAL bits, halo included, for the plain and for the pooled NCHW-fed entry;
  * form 7 (each channel pair as two 4-byte LDS reads: the same values, the same arithmetic) is the one ablation with valid results:
    EQUAL bits -- the check of the dev kernel's copy of the arithmetic and of the item loop;
  * forms 1..6 (plain) and 8..13 (pooled, NCHW-fed) leave a part of the kernel out: wrong by construction, so only that they launch and
    the device synchronises without an error;
  * every other number is a bad argument.

Cases (32 x 32 is the smallest map the kernel takes: one item):
  * B = 3, 32 x 32: three items -- one full pair of teams and one workgroup whose second team is idle;
  * B = 1, 32 x 64: two blocks in a row -- the split of an item index into (image, block row, block column);
  * B = 515, 32 x 32: 258 pairs on the 256-workgroup grid -- two workgroups hand over to a successor item, the last item is alone.
"""
import pytest
import torch

from hierarchicalprobabilistic3dhuman_amd import _capi
from hierarchicalprobabilistic3dhuman_amd.resnet import _ConvBN

pytestmark = pytest.mark.gpu

P = _capi.ptr
FILL = 7.0
CASES = [(3, 32, 32), (1, 32, 64), (515, 32, 32)]
_CASES = {}


def _plain(c, ablate=None):
    """hps_stem_winograd (ablate None) or hps_dev_stem_winograd into a frame of FILL with a halo of one pixel, bn1 + relu."""
    B, H, W = c["cfg"]
    cb = c["cb"]
    y = torch.full((B, H // 2 + 2, W // 2 + 2, 64), FILL, device=c["x"].device)
    args = (P(c["frames"]), P(cb.stem_u), P(cb.scale), P(cb.shift), P(y), B, H, W, 1, 1)
    if ablate is None:
        _capi.call("hps_stem_winograd", *args, _capi.stream())
    else:
        with _capi.dev_library():
            _capi.call("hps_dev_stem_winograd", *args, ablate, _capi.stream())
    torch.cuda.synchronize()
    return y


def _pooled_nchw(c, ablate=None):
    """hps_stem_winograd_pooled_nchw (ablate None) or hps_dev_stem_winograd_pooled_nchw into a pooled frame of FILL, halo of one pixel."""
    B, H, W = c["cfg"]
    cb = c["cb"]
    y = torch.full((B, H // 4 + 2, W // 4 + 2, 64), FILL, device=c["x"].device)
    side = torch.full((int(_capi.load().hps_stem_pool_side_bytes(B, H, W)) // 4,), float("nan"), device=y.device)
    args = (P(c["x"]), P(cb.stem_u), P(cb.scale), P(cb.shift), P(y), P(side), B, H, W, 1, 1)
    if ablate is None:
        _capi.call("hps_stem_winograd_pooled_nchw", *args, _capi.stream())
    else:
        with _capi.dev_library():
            _capi.call("hps_dev_stem_winograd_pooled_nchw", *args, ablate, _capi.stream())
    torch.cuda.synchronize()
    return y


def _case(cfg, dev):
    """Inputs, the device layer and the product's two outputs of (B, H, W); built once per configuration and left unchanged."""
    if cfg in _CASES:
        return _CASES[cfg]
    B, H, W = cfg
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(11 * B + H + W)
        conv = torch.nn.Conv2d(18, 64, 7, 2, 3, bias=False)
        bn = torch.nn.BatchNorm2d(64).eval()
        bn.running_mean.normal_(); bn.running_var.uniform_(0.5, 2); bn.weight.data.normal_(); bn.bias.data.normal_()      # (negative scales too)
        x = torch.randn(B, 18, H, W)
    c = dict(cfg=cfg, cb=_ConvBN(conv.to(dev), bn.to(dev), cin_pad=20), x=x.to(dev))
    c["frames"] = torch.zeros(int(_capi.load().hps_stem_phase_frames_bytes(B, H, W)) // 4, device=dev)
    _capi.call("hps_stem_phase_split", P(c["x"]), P(c["frames"]), B, 18, H, W, _capi.stream())
    c["plain"] = _plain(c)
    c["pooled"] = _pooled_nchw(c)
    assert (c["plain"][:, 1:-1, 1:-1] != FILL).any() and (c["pooled"][:, 1:-1, 1:-1] != FILL).any()      # (the product wrote something)
    _CASES[cfg] = c
    return c


@pytest.mark.parametrize("cfg", CASES)
def test_dev_entries_without_an_ablation_are_the_product(cfg, dev):
    c = _case(cfg, dev)
    assert torch.equal(_plain(c, 0), c["plain"])
    assert torch.equal(_pooled_nchw(c, 0), c["pooled"])


@pytest.mark.parametrize("cfg", CASES)
def test_form_with_split_lds_reads_has_the_products_bits(cfg, dev):
    c = _case(cfg, dev)
    assert torch.equal(_plain(c, 7), c["plain"])


@pytest.mark.parametrize("ablate", [1, 2, 3, 4, 5, 6, 8, 9, 10, 11, 12, 13])
def test_ablated_forms_launch(ablate, dev):
    c = _case(CASES[0], dev)
    (_plain if ablate < 8 else _pooled_nchw)(c, ablate)          # HPS_OK (a failed call raises) and a clean synchronise; the output is not examined


def test_numbers_that_name_no_form_are_bad_arguments(dev):
    c = _case(CASES[0], dev)
    for ablate in (-1, 8, 14):
        with pytest.raises(_capi.HpsError):
            _plain(c, ablate)
    for ablate in (1, 2, 3, 4, 5, 6, 7, 14):
        with pytest.raises(_capi.HpsError):
            _pooled_nchw(c, ablate)
