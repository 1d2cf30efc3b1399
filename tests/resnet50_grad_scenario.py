"""Seeded cases and reference gradients of the Bottleneck encoder's backward tests (tests/test_resnet50_backward_host.py,
tests/test_gpu_resnet50_backward.py).  Extends resnet50_scenario (its cases, weights and encoder builder, imported).

The reference restates the eval-mode Bottleneck encoder (He et al., CVPR 2016, in torchvision's v1.5 form, as resnet50_scenario
describes it) with torch operations in a given dtype, in the manner of encoder_grad_scenario: ReLU as y * mask and the max pool as a
gather, masks and pool winners PINNED to a given run (the device's; on the CPU the fp32 restatement's own).  Pinned masks and winners
are constants, so the pinned float64 autograd is the truth for the function the device evaluates.  Maps are named as
ResNet.activations names them: 'stem', 'pool', 'layerL.j.c1' and '.c2' (after their ReLUs), 'layerL.j.c3' (the block's output),
'layerL.j.down'.

Cases: resnet50_scenario's "small_wino" (layers (2, 2, 1, 1), input (3, 18, 64, 64): Winograd stem and 3x3 layers, layer4 on 2 x 2
maps), "small_generic" ((2, 18, 40, 24): generic stem, odd non-square maps 5 x 3, 3 x 2, 2 x 1 under the stride-2 layers, every layer
direct) and "full" ((3, 4, 6, 3) at (2, 18, 64, 64)).  Cotangents randn(B, 2048).  The accuracy rule is smpl_grad_scenario.bound /
check, imported and not copied: 4 max(max|cpu32 - f64|, 2^-23 max|g64|).  References are computed once per key and shared (callers
must not modify them).

``forward_train`` / ``vjp_train`` / ``reference_train`` are the same on batch statistics, as bn_train_scenario does it for the
BasicBlock encoder: every TRAINING layer's BatchNorm is F.batch_norm(..., training=True) with the running buffers passed in.  On
small_generic layer4 normalises over n = 4 values per channel; the fp32 restatement's own error is then large, and the rule's bound
with it (the tests print that figure).
"""
import functools

import torch
import torch.nn.functional as F

from encoder_grad_scenario import flips, param_names, pins_from_maps  # noqa: F401  (name-agnostic helpers, re-exported)
from resnet50_scenario import BN_EPS, CASES, build_encoder, case as _case, encoder_shapes, layers_of, seeded_state_dict  # noqa: F401
from smpl_grad_scenario import EPS32, bound, check  # noqa: F401  (the accuracy rule, imported and not copied)

GRAD_CASES = ("small_wino", "small_generic", "full")


@functools.lru_cache(maxsize=None)
def case(name):
    """(state dict, fp32 input, cotangent (B, 2048)) of a case."""
    sd, x = _case(name)
    g = torch.Generator().manual_seed(300 + GRAD_CASES.index(name))
    return sd, x, torch.randn(x.shape[0], 2048, generator=g)


def forward(sd, x, pins=None):
    """The encoder restated in the dtype of ``x`` / ``sd``: (features (B, 2048), activation maps).  pins: masks and winners to use
    instead of the run's own (ReLU is y * mask, the pool a gather, either way)."""
    dt = x.dtype
    maps = {}

    def conv_bn(x, conv, bn, stride, pad):
        y = F.conv2d(x, sd[conv + ".weight"], None, stride, pad)
        return F.batch_norm(y, sd[bn + ".running_mean"], sd[bn + ".running_var"], sd[bn + ".weight"], sd[bn + ".bias"], False, 0.0, BN_EPS)

    def relu(name, y):
        mask = pins["mask"][name] if pins is not None else y.detach() > 0
        maps[name] = y * mask.to(dt)
        return maps[name]

    y = relu("stem", conv_bn(x, "conv1", "bn1", 2, 3))
    B, C, H, W = y.shape
    idx = pins["winners"] if pins is not None else F.max_pool2d(y.detach(), 3, 2, 1, return_indices=True)[1]
    y = y.flatten(2).gather(2, idx.flatten(2)).view(B, C, idx.shape[2], idx.shape[3])
    maps["pool"] = y
    for li, blocks in enumerate(layers_of(sd), 1):
        for bi in range(blocks):
            name = "layer%d.%d" % (li, bi)
            stride = 2 if li > 1 and bi == 0 else 1
            identity = y
            if (name + ".downsample.0.weight") in sd:
                identity = maps[name + ".down"] = conv_bn(y, name + ".downsample.0", name + ".downsample.1", stride, 0)
            t = relu(name + ".c1", conv_bn(y, name + ".conv1", name + ".bn1", 1, 0))
            t = relu(name + ".c2", conv_bn(t, name + ".conv2", name + ".bn2", stride, 1))
            y = relu(name + ".c3", conv_bn(t, name + ".conv3", name + ".bn3", 1, 0) + identity)
    return y.mean(dim=(2, 3)), maps


def plain_forward(sd, x):
    """The same network as plain F.conv2d / F.batch_norm / F.relu / F.max_pool2d calls (the restatement's own check)."""
    bn = lambda y, p: F.batch_norm(y, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"], False, 0.0, BN_EPS)
    y = F.max_pool2d(F.relu(bn(F.conv2d(x, sd["conv1.weight"], None, 2, 3), "bn1")), 3, 2, 1)
    for li, blocks in enumerate(layers_of(sd), 1):
        for bi in range(blocks):
            p = "layer%d.%d." % (li, bi)
            stride = 2 if li > 1 and bi == 0 else 1
            t = F.relu(bn(F.conv2d(y, sd[p + "conv1.weight"]), p + "bn1"))
            t = F.relu(bn(F.conv2d(t, sd[p + "conv2.weight"], None, stride, 1), p + "bn2"))
            t = bn(F.conv2d(t, sd[p + "conv3.weight"]), p + "bn3")
            if p + "downsample.0.weight" in sd:
                y = bn(F.conv2d(y, sd[p + "downsample.0.weight"], None, stride), p + "downsample.1")
            y = F.relu(t + y)
    return y.mean(dim=(2, 3))


def _leaves(sd32, x32, dtype):
    sd = {k: (v.detach().to(dtype).clone() if v.is_floating_point() else v) for k, v in sd32.items()}
    names = param_names(sd)
    for k in names:
        sd[k].requires_grad_(True)
    return sd, names, x32.detach().to(dtype).clone().requires_grad_(True)


def vjp(sd32, x32, pins, cot, dtype, fn=None):
    """Gradients (float64 tensors) of <cot, features> by autograd through ``forward`` in ``dtype`` (``fn``: through that function of
    (sd, x) instead): dict over "input" and the parameter names."""
    sd, names, x = _leaves(sd32, x32, dtype)
    feats = forward(sd, x, pins)[0] if fn is None else fn(sd, x)
    grads = torch.autograd.grad((cot.to(dtype) * feats).sum(), [x] + [sd[k] for k in names])
    return {k: g.double() for k, g in zip(["input"] + names, grads)}


_REFERENCES = {}


def reference(key, sd32, x32, pins, cot):
    """(g64, g32) for ``key`` (any hashable naming weights, input, pinned run and cotangent), computed once."""
    if key not in _REFERENCES:
        cot = cot.detach().cpu()
        _REFERENCES[key] = (vjp(sd32, x32, pins, cot, torch.float64), vjp(sd32, x32, pins, cot, torch.float32))
    return _REFERENCES[key]


@functools.lru_cache(maxsize=None)
def self_pins(name):
    """Masks and winners of the fp32 CPU restatement's own run of a case."""
    sd, x, _ = case(name)
    with torch.no_grad():
        return pins_from_maps(forward(sd, x)[1])


# ---- training-mode BatchNorm, as bn_train_scenario does it for the BasicBlock encoder ----
def layer_keys(sd):
    """{layer name as ResNet._enc_layers(): (conv prefix, bn prefix)} in that order."""
    out = {"stem": ("conv1", "bn1")}
    for li, blocks in enumerate(layers_of(sd), 1):
        for bi in range(blocks):
            name = "layer%d.%d" % (li, bi)
            for i in (1, 2, 3):
                out["%s.c%d" % (name, i)] = ("%s.conv%d" % (name, i), "%s.bn%d" % (name, i))
            if (name + ".downsample.0.weight") in sd:
                out[name + ".down"] = (name + ".downsample.0", name + ".downsample.1")
    return out


def forward_train(sd, x, pins=None, train=None, update=False):
    """(features, maps, stats) in the dtype of ``sd`` / ``x``.  train: the layer names on batch statistics (None: all), every such
    BatchNorm as F.batch_norm(..., training=True) with momentum 0.1 -- torch's own batch statistics, running update and backward through
    the statistics; update: the running buffers and counters of ``sd`` move in place, else clones do.  stats[name] = (mean, biased
    var, n) of the training layers' raw maps."""
    dt = x.dtype
    keys = layer_keys(sd)
    train = set(keys) if train is None else set(train)
    maps, stats = {}, {}

    def conv_bn(name, x, stride, pad):
        conv, bn = keys[name]
        z = F.conv2d(x, sd[conv + ".weight"], None, stride, pad)
        rm, rv = sd[bn + ".running_mean"], sd[bn + ".running_var"]
        if name not in train:
            return F.batch_norm(z, rm, rv, sd[bn + ".weight"], sd[bn + ".bias"], False, 0.0, BN_EPS)
        if not update:
            rm, rv = rm.detach().clone(), rv.detach().clone()
        else:
            sd[bn + ".num_batches_tracked"] += 1
        stats[name] = (z.detach().mean((0, 2, 3)), z.detach().var((0, 2, 3), unbiased=False), z.numel() // z.shape[1])
        return F.batch_norm(z, rm, rv, sd[bn + ".weight"], sd[bn + ".bias"], True, 0.1, BN_EPS)

    def relu(name, y):
        mask = pins["mask"][name] if pins is not None else y.detach() > 0
        maps[name] = y * mask.to(dt)
        return maps[name]

    y = relu("stem", conv_bn("stem", x, 2, 3))
    B, C = y.shape[:2]
    idx = pins["winners"] if pins is not None else F.max_pool2d(y.detach(), 3, 2, 1, return_indices=True)[1]
    y = y.flatten(2).gather(2, idx.flatten(2)).view(B, C, idx.shape[2], idx.shape[3])
    maps["pool"] = y
    for li, blocks in enumerate(layers_of(sd), 1):
        for bi in range(blocks):
            name = "layer%d.%d" % (li, bi)
            stride = 2 if li > 1 and bi == 0 else 1
            identity = y
            if name + ".down" in keys:
                identity = maps[name + ".down"] = conv_bn(name + ".down", y, stride, 0)
            t = relu(name + ".c1", conv_bn(name + ".c1", y, 1, 0))
            t = relu(name + ".c2", conv_bn(name + ".c2", t, stride, 1))
            y = relu(name + ".c3", conv_bn(name + ".c3", t, 1, 0) + identity)
    return y.mean(dim=(2, 3)), maps, stats


def plain_forward_train(sd, x):
    """Every BatchNorm on batch statistics as plain F calls (the training restatement's own check)."""
    bn = lambda y, p: F.batch_norm(y, sd[p + ".running_mean"].clone(), sd[p + ".running_var"].clone(), sd[p + ".weight"], sd[p + ".bias"],
                                   True, 0.1, BN_EPS)
    y = F.max_pool2d(F.relu(bn(F.conv2d(x, sd["conv1.weight"], None, 2, 3), "bn1")), 3, 2, 1)
    for li, blocks in enumerate(layers_of(sd), 1):
        for bi in range(blocks):
            p = "layer%d.%d." % (li, bi)
            stride = 2 if li > 1 and bi == 0 else 1
            t = F.relu(bn(F.conv2d(y, sd[p + "conv1.weight"]), p + "bn1"))
            t = F.relu(bn(F.conv2d(t, sd[p + "conv2.weight"], None, stride, 1), p + "bn2"))
            t = bn(F.conv2d(t, sd[p + "conv3.weight"]), p + "bn3")
            if p + "downsample.0.weight" in sd:
                y = bn(F.conv2d(y, sd[p + "downsample.0.weight"], None, stride), p + "downsample.1")
            y = F.relu(t + y)
    return y.mean(dim=(2, 3))


def vjp_train(sd32, x32, pins, cot, dtype, train=None):
    """(gradients dict (float64), features (float64)) of <cot, features> through ``forward_train`` in ``dtype``."""
    sd, names, x = _leaves(sd32, x32, dtype)
    feats, _, _ = forward_train(sd, x, pins, train)
    grads = torch.autograd.grad((cot.to(dtype) * feats).sum(), [x] + [sd[k] for k in names])
    return {k: g.double() for k, g in zip(["input"] + names, grads)}, feats.detach().double()


def reference_train(key, sd32, x32, pins, cot, train=None):
    """((g64, feats64), (g32, feats32)) for ``key``, computed once; callers must not modify it."""
    key = ("train", key)
    if key not in _REFERENCES:
        cot = cot.detach().cpu()
        _REFERENCES[key] = (vjp_train(sd32, x32, pins, cot, torch.float64, train), vjp_train(sd32, x32, pins, cot, torch.float32, train))
    return _REFERENCES[key]


def running_update(running, batch, momentum):
    """running <- (1 - m) running + m batch in float64, rounded once to fp32."""
    return ((1.0 - momentum) * running.double() + momentum * batch.double()).float()


# every distinct 1x1 layer of ResNet-50 on 256 x 256 inputs: (Cin, Cout, stride, input map H = W)
def resnet50_1x1_layers():
    out, inplanes, hw = [], 64, 64
    for li, planes in enumerate((64, 128, 256, 512), 1):
        stride = 1 if li == 1 else 2
        out += [(inplanes, planes, 1, hw), (planes, planes * 4, 1, hw // stride), (inplanes, planes * 4, stride, hw)]     # c1, c3, down of the entry
        hw //= stride
        inplanes = planes * 4
        out.append((inplanes, planes, 1, hw))                                                                             # c1 of the other blocks
    return sorted(set(out))
