"""Cases and references of the training-mode BatchNorm tests (tests/test_bn_train_host.py, tests/test_gpu_bn_train.py).

The reference restates the encoder as encoder_grad_scenario does (torch operations in a given dtype, ReLU as y * mask, the max pool as
a gather, masks and winners pinned), with every TRAINING layer's BatchNorm as F.batch_norm(..., training=True) and the running buffers
passed in -- torch's own batch statistics, running update (unbiased variance, momentum) and backward through the statistics.  Recipe,
inputs, cotangents and the accuracy rule are encoder_grad_scenario's / smpl_grad_scenario's, imported and not copied.

Cases.  Batch normalisation over a handful of values amplifies the convolution's roundings: the fp32 restatement's own worst-tensor
gradient error against float64 (units of 2^-23 max|g|) is 147 / 143 / 127 for sq64 / wide / c5 (layer4 n = 12 / 12 / 8) but 526 for
tiny32 (n = 5) and 2136 for odd (n = 4); a gradient test on those would check nothing.  GRADIENT_CASES are the three
well-conditioned ones, and CAP keeps the adaptive bound (4 x the restatement's own error) from hiding a failure: the restatement's
own error on a used case must stay <= CAP x 2^-23 max|g|.
"""
import torch
import torch.nn.functional as F

import encoder_grad_scenario as ES
from encoder_grad_scenario import EPS32, bound, check  # noqa: F401

GRADIENT_CASES = ("sq64", "wide", "c5")
CAP = 256.0
BLOCKS = ES.BLOCKS


def layer_keys(sd):
    """{layer name as ResNet._enc_layers(): (conv prefix, bn prefix)} in that order."""
    out = {"stem": ("conv1", "bn1")}
    for name in BLOCKS:
        out[name + ".c1"] = (name + ".conv1", name + ".bn1")
        out[name + ".c2"] = (name + ".conv2", name + ".bn2")
        if (name + ".downsample.0.weight") in sd:
            out[name + ".down"] = (name + ".downsample.0", name + ".downsample.1")
    return out


def forward(sd, x, pins=None, train=None, momentum=None, update=False):
    """(features, maps, stats) in the dtype of ``sd`` / ``x``.  train: the layer names on batch statistics (None: all); momentum:
    {layer name: momentum} (default 0.1); update: F.batch_norm updates sd's running buffers in place (and this function the
    counters), else it works on clones.  stats[name] = (mean, biased var, n) of the training layers' raw maps."""
    dt = x.dtype
    keys = layer_keys(sd)
    train = set(keys) if train is None else set(train)
    maps, stats = {}, {}

    def conv_bn(name, x, stride, pad):
        conv, bn = keys[name]
        z = F.conv2d(x, sd[conv + ".weight"], None, stride, pad)
        if name in train:
            rm, rv = sd[bn + ".running_mean"], sd[bn + ".running_var"]
            if not update:
                rm, rv = rm.detach().clone(), rv.detach().clone()
            else:
                sd[bn + ".num_batches_tracked"] += 1
            stats[name] = (z.detach().mean((0, 2, 3)), z.detach().var((0, 2, 3), unbiased=False), z.numel() // z.shape[1])
            return F.batch_norm(z, rm, rv, sd[bn + ".weight"], sd[bn + ".bias"], True, (momentum or {}).get(name, 0.1), ES.BN_EPS)
        scale = sd[bn + ".weight"] * torch.rsqrt(sd[bn + ".running_var"] + ES.BN_EPS)
        shift = sd[bn + ".bias"] - sd[bn + ".running_mean"] * scale
        return z * scale[None, :, None, None] + shift[None, :, None, None]

    def relu(name, y):
        mask = pins["mask"][name] if pins is not None else y.detach() > 0
        maps[name] = y * mask.to(dt)
        return maps[name]

    y = relu("stem", conv_bn("stem", x, 2, 3))
    B, C = y.shape[:2]
    idx = pins["winners"] if pins is not None else F.max_pool2d(y.detach(), 3, 2, 1, return_indices=True)[1]
    y = y.flatten(2).gather(2, idx.flatten(2)).view(B, C, idx.shape[2], idx.shape[3])
    maps["pool"] = y
    for name in BLOCKS:
        stride = 2 if name.endswith(".0") and not name.startswith("layer1") else 1
        identity = y
        if name + ".down" in keys:
            identity = maps[name + ".down"] = conv_bn(name + ".down", y, stride, 0)
        out = relu(name + ".c1", conv_bn(name + ".c1", y, stride, 1))
        y = relu(name + ".c2", conv_bn(name + ".c2", out, 1, 1) + identity)
    return y.mean(dim=(2, 3)), maps, stats


def cast(sd32, dtype):
    return {k: (v.detach().to(dtype).clone() if v.is_floating_point() else v.clone()) for k, v in sd32.items()}


def vjp(sd32, x32, pins, cot, dtype, train=None):
    """Gradients (float64) of <cot, features> by autograd through ``forward`` in ``dtype``: dict over "input" and the parameter names."""
    sd = cast(sd32, dtype)
    names = ES.param_names(sd)
    for k in names:
        sd[k].requires_grad_(True)
    x = x32.detach().to(dtype).clone().requires_grad_(True)
    feats, _, _ = forward(sd, x, pins, train)
    grads = torch.autograd.grad((cot.to(dtype) * feats).sum(), [x] + [sd[k] for k in names])
    return {k: g.double() for k, g in zip(["input"] + names, grads)}, feats.detach().double()


_REFERENCES = {}


def reference(key, sd32, x32, pins, cot, train=None):
    """((g64, feats64), (g32, feats32)) for ``key`` (any hashable naming weights, input, pinned run, cotangent and training set),
    computed once; callers must not modify it."""
    if key not in _REFERENCES:
        cot = cot.detach().cpu()
        _REFERENCES[key] = (vjp(sd32, x32, pins, cot, torch.float64, train), vjp(sd32, x32, pins, cot, torch.float32, train))
    return _REFERENCES[key]


def own_error(g64, g32):
    """The fp32 restatement's worst-tensor error in units of 2^-23 max|g64| (the figure CAP bounds)."""
    return max(float((g32[k] - g64[k]).abs().max()) / (EPS32 * float(g64[k].abs().max())) for k in g64)


def running_update(running, batch, momentum):
    """running <- (1 - m) running + m batch in float64, rounded once to fp32."""
    return ((1.0 - momentum) * running.double() + momentum * batch.double()).float()
