"""Seeded cases and reference gradients of the encoder backward tests (tests/test_encoder_backward_host.py,
tests/test_gpu_encoder_backward.py).

The reference restates the eval-mode ResNet-18 (models/resnet.py:62-78, 202-217) with torch operations in a given dtype, ReLU as
y * mask and the max pool as a gather, with masks and pool winners PINNED to a given run (the device's; on the CPU the fp32
restatement's own).  A plain float64 run is not a valid reference for the gradient: at a pre-activation near 0 it may gate differently
from the fp32 run, and then it differentiates another function.  Pinned masks and winners are constants, so the pinned float64
autograd is the truth for the function the device evaluates -- the argument of the pinned SVD signs in head_grad_scenario.

Weights: the package's ResNet under torch.manual_seed(0) with default initialisation; BatchNorm from Generator().manual_seed(1), per
BatchNorm in module order: running_mean = 0.2 randn, running_var = 0.5 + rand, weight = 0.5 + rand, bias = 0.2 randn.  Inputs rand,
cotangents randn(B, 512).  The accuracy rule is smpl_grad_scenario.bound / check.  References are computed once per case and shared
(callers must not modify them).
"""
import functools

import torch
import torch.nn.functional as F
from torch import nn

from hierarchicalprobabilistic3dhuman_amd.resnet import resnet18
from smpl_grad_scenario import EPS32, bound, check  # noqa: F401  (the accuracy rule, imported and not copied)

BN_EPS = 1e-5
# name -> (in_channels, input shape): square Winograd-eligible maps (32 -> 16 -> 16 / 8 / 4 / 2); non-square (16 x 24 maps take the
# direct kernel); layer4 at 1 x 1 (every tap but the centre lies in the halo); odd maps 5 x 7 and 3 x 4 under the stride-2 layers;
# another channel count and an image the stem's fast paths do not take (the generic stem frame)
CASES = {"sq64": (18, (3, 18, 64, 64)), "wide": (18, (2, 18, 64, 96)), "tiny32": (18, (5, 18, 32, 32)),
         "odd": (18, (1, 18, 40, 56)), "c5": (5, (2, 5, 34, 46))}
BLOCKS = tuple("layer%d.%d" % (l, b) for l in (1, 2, 3, 4) for b in (0, 1))


def randomize_bn(encoder, seed=1):
    """The recipe's BatchNorm statistics and affine parameters, in place."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in encoder.modules():
            if isinstance(m, nn.BatchNorm2d):
                n = m.num_features
                m.running_mean.copy_(0.2 * torch.randn(n, generator=g))
                m.running_var.copy_(0.5 + torch.rand(n, generator=g))
                m.weight.copy_(0.5 + torch.rand(n, generator=g))
                m.bias.copy_(0.2 * torch.randn(n, generator=g))
    return encoder


def make_encoder(in_channels=18):
    """A fresh encoder of the recipe (CPU, eval mode)."""
    torch.manual_seed(0)
    return randomize_bn(resnet18(in_channels=in_channels)).eval()


@functools.lru_cache(maxsize=None)
def state(in_channels=18):
    return {k: v.clone() for k, v in make_encoder(in_channels).state_dict().items()}


def param_names(sd):
    return [k for k in sd if k.endswith(".weight") or k.endswith(".bias")]


@functools.lru_cache(maxsize=None)
def case(name):
    """(fp32 input, cotangent (B, 512)) of a case."""
    _, shape = CASES[name]
    g = torch.Generator().manual_seed(100 + sorted(CASES).index(name))
    return torch.rand(*shape, generator=g), torch.randn(shape[0], 512, generator=g)


def pins_from_maps(maps):
    """ReLU masks and pool winners of a run, from its activation maps (ResNet.activations on the device, or forward() here):
    {"mask": {name: bool map}, "winners": flat indices of each 3x3 / 2 window's first maximum in row-major order (torch's rule)}."""
    maps = {k: v.detach().cpu() for k, v in maps.items()}
    _, idx = F.max_pool2d(maps["stem"].float(), 3, 2, 1, return_indices=True)
    return {"mask": {k: v > 0 for k, v in maps.items() if k != "pool" and not k.endswith(".down")}, "winners": idx}


def flips(pins_a, pins_b):
    """Number of mask entries and pool winners in which two runs differ."""
    n = sum(int((pins_a["mask"][k] != pins_b["mask"][k]).sum()) for k in pins_a["mask"])
    return n + int((pins_a["winners"] != pins_b["winners"]).sum())


def forward(sd, x, pins=None):
    """The encoder restated in the dtype of ``sd`` / ``x``: (features (B, 512), activation maps as ResNet.activations names them).
    pins: masks and winners to use instead of the run's own (ReLU is y * mask, the pool a gather, either way)."""
    dt = x.dtype
    maps = {}

    def conv_bn(x, conv, bn, stride, pad):
        y = F.conv2d(x, sd[conv + ".weight"], None, stride, pad)
        scale = sd[bn + ".weight"] * torch.rsqrt(sd[bn + ".running_var"] + BN_EPS)
        shift = sd[bn + ".bias"] - sd[bn + ".running_mean"] * scale
        return y * scale[None, :, None, None] + shift[None, :, None, None]

    def relu(name, y):
        mask = pins["mask"][name] if pins is not None else y.detach() > 0
        maps[name] = y * mask.to(dt)
        return maps[name]

    y = relu("stem", conv_bn(x, "conv1", "bn1", 2, 3))
    B, C, H, W = y.shape
    idx = pins["winners"] if pins is not None else F.max_pool2d(y.detach(), 3, 2, 1, return_indices=True)[1]
    y = y.flatten(2).gather(2, idx.flatten(2)).view(B, C, idx.shape[2], idx.shape[3])
    maps["pool"] = y
    for name in BLOCKS:
        stride = 2 if name.endswith(".0") and not name.startswith("layer1") else 1
        identity = y
        if (name + ".downsample.0.weight") in sd:
            identity = maps[name + ".down"] = conv_bn(y, name + ".downsample.0", name + ".downsample.1", stride, 0)
        out = relu(name + ".c1", conv_bn(y, name + ".conv1", name + ".bn1", stride, 1))
        y = relu(name + ".c2", conv_bn(out, name + ".conv2", name + ".bn2", 1, 1) + identity)
    return y.mean(dim=(2, 3)), maps


def vjp(sd32, x32, pins, cot, dtype):
    """Gradients (float64 tensors) of <cot, features> by autograd through ``forward`` in ``dtype``: dict over "input" and the
    parameter names."""
    sd = {k: (v.detach().to(dtype).clone() if v.is_floating_point() else v) for k, v in sd32.items()}
    names = param_names(sd)
    for k in names:
        sd[k].requires_grad_(True)
    x = x32.detach().to(dtype).clone().requires_grad_(True)
    feats, _ = forward(sd, x, pins)
    leaves = [x] + [sd[k] for k in names]
    grads = torch.autograd.grad((cot.to(dtype) * feats).sum(), leaves)
    return {k: g.double() for k, g in zip(["input"] + names, grads)}


_REFERENCES = {}


def reference(key, sd32, x32, pins, cot):
    """(g64, g32) for the case ``key`` (any hashable naming weights, input, pinned run and cotangent), computed once."""
    if key not in _REFERENCES:
        cot = cot.detach().cpu()
        _REFERENCES[key] = (vjp(sd32, x32, pins, cot, torch.float64), vjp(sd32, x32, pins, cot, torch.float32))
    return _REFERENCES[key]


@functools.lru_cache(maxsize=None)
def self_pins(name):
    """Masks and winners of the fp32 CPU restatement's own run of a case."""
    x, _ = case(name)
    with torch.no_grad():
        return pins_from_maps(forward(state(CASES[name][0]), x)[1])
