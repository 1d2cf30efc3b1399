"""CPU: the reference of the encoder backward tests (encoder_grad_scenario) is what it claims to be, and the new entry points of
csrc/conv_backward.hip exist and validate their arguments on the host."""
import pytest
import torch

import encoder_grad_scenario as ES
from hierarchicalprobabilistic3dhuman_amd import _capi

NEW_SYMBOLS = ("hps_conv_wgrad", "hps_conv_wgrad_slice_pixels", "hps_conv_wgrad_workspace", "hps_conv_dgrad", "hps_relu_gate_pad",
               "hps_relu_gate_workspace", "hps_maxpool3x3s2_backward", "hps_global_avgpool_backward")


def test_new_entry_points_validate_on_the_host():
    """Fails without the feature: the symbols are declared, exported and reject bad arguments before any launch."""
    lib = _capi.load()
    for name in NEW_SYMBOLS:
        assert name in _capi.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.hps_conv_wgrad(*([None] * 4 + [1, 8, 8, 1, 64, 64, 64, 3, 3, 1, 1, 1, None])) == -1 and b"null pointer" in lib.hps_last_error()
    assert lib.hps_conv_dgrad(*([None] * 4 + [1, 8, 8, 64, 64, 3, 3, 1, 1, 1, 1, 64, None])) == -1
    assert lib.hps_relu_gate_pad(*([None] * 4 + [1, 8, 8, 64, 1, 1, None])) == -1
    assert lib.hps_maxpool3x3s2_backward(*([None] * 3 + [1, 8, 8, 64, 1, None])) == -1
    assert lib.hps_global_avgpool_backward(*([None] * 2 + [1, 8, 8, 64, 1, None])) == -1
    p = torch.zeros(4).data_ptr()
    P = _capi._P
    assert lib.hps_conv_wgrad(P(p), P(p), P(p), P(p), 1, 8, 8, 0, 64, 64, 64, 3, 3, 1, 1, 1, None) == -1 and b"halo" in lib.hps_last_error()
    assert lib.hps_conv_dgrad(P(p), P(p), None, P(p), 1, 8, 8, 64, 12, 3, 3, 1, 1, 1, 1, 64, None) == -1 and b"Cout % 8" in lib.hps_last_error()
    # the slice rule depends on the map alone: its pixel count clamped to [128, 512]
    s = lib.hps_conv_wgrad_slice_pixels
    assert (s(1, 1), s(5, 7), s(16, 16), s(24, 24), s(128, 128)) == (128, 128, 256, 512, 512)
    w = lib.hps_conv_wgrad_workspace
    assert w(5, 10, 14, 64, 128, 3, 3, 2, 1) == 2 * 128 * 9 * 64 * 4            # 5 x 5 x 7 = 175 pixels: two slices of 128
    assert w(64, 8, 8, 512, 512, 3, 3, 1, 1) == 32 * 512 * 9 * 512 * 4
    assert lib.hps_relu_gate_workspace(3, 5, 7, 64) == 2 * 64 * 8


def test_pinned_equals_plain_float64_when_no_mask_flips():
    """The fp32 restatement's masks and winners equal the float64 run's on these inputs, and then pinning changes nothing."""
    for name in ("sq64", "tiny32"):
        x, cot = ES.case(name)
        sd = ES.state(ES.CASES[name][0])
        pins32 = ES.self_pins(name)
        with torch.no_grad():
            pins64 = ES.pins_from_maps(ES.forward({k: v.double() if v.is_floating_point() else v for k, v in sd.items()}, x.double())[1])
        n = ES.flips(pins32, pins64)
        print("%s: %d mask / winner flips between the fp32 and the float64 run" % (name, n))
        assert n == 0
        pinned, plain = ES.vjp(sd, x, pins32, cot, torch.float64), ES.vjp(sd, x, None, cot, torch.float64)
        for k in pinned:
            assert torch.equal(pinned[k], plain[k]), k
        g32 = ES.vjp(sd, x, pins32, cot, torch.float32)
        worst = max(float((g32[k] - pinned[k]).abs().max()) / (ES.EPS32 * float(pinned[k].abs().max())) for k in pinned)
        print("%s: worst cpu32 error %.2f x 2^-23 max|g| over %d tensors" % (name, worst, len(pinned)))
        assert worst < 64.0


def test_pinned_float64_gradient_against_central_differences():
    """With the masks and winners held fixed the function is smooth: its autograd gradient equals central differences on a few
    entries of every tensor kind (input, 7x7 / 3x3 / 1x1 convolution weight, BatchNorm weight and bias)."""
    name = "tiny32"
    x, cot = ES.case(name)
    sd32 = ES.state(18)
    pins = ES.self_pins(name)
    g = ES.vjp(sd32, x, pins, cot, torch.float64)
    sd = {k: v.double() if v.is_floating_point() else v for k, v in sd32.items()}
    x64, cot64 = x.double(), cot.double()

    def loss():
        with torch.no_grad():
            return float((cot64 * ES.forward(sd, x64, pins)[0]).sum())

    gen = torch.Generator().manual_seed(3)
    for key in ("input", "conv1.weight", "layer1.0.conv2.weight", "layer2.0.conv1.weight", "layer3.0.downsample.0.weight",
                "layer4.1.conv2.weight", "bn1.weight", "layer2.0.downsample.1.weight", "layer4.1.bn2.weight", "bn1.bias",
                "layer3.1.bn1.bias", "layer4.0.downsample.1.bias"):
        t = x64 if key == "input" else sd[key]
        flat = t.view(-1)
        scale = float(g[key].abs().max())
        for i in torch.randint(0, flat.numel(), (2,), generator=gen).tolist():
            keep, h = float(flat[i]), 1e-4
            flat[i] = keep + h
            up = loss()
            flat[i] = keep - h
            down = loss()
            flat[i] = keep
            fd, an = (up - down) / (2 * h), float(g[key].view(-1)[i])
            # central differences of a function cubic at most in one entry: error h^2 f''' / 6 plus cancellation ~1e-16 |L| / h
            assert abs(fd - an) <= 1e-6 * scale + 1e-7, (key, i, fd, an)


@pytest.mark.parametrize("name", sorted(ES.CASES))
def test_cases_build_and_masks_are_mixed(name):
    """Every case runs through the restatement and gates a real share of its activations either way (a mask of all ones or all
    zeros would pin nothing)."""
    pins = ES.self_pins(name)
    for k, m in pins["mask"].items():
        share = float(m.double().mean())
        assert 0.02 < share < 0.98, (k, share)
