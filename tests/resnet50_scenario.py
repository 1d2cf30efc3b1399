"""Seeded weights, cases and the CPU restatement of the Bottleneck encoder for the ResNet-50 tests (tests/test_resnet50_host.py,
tests/test_gpu_resnet50.py, tests/golden/make_resnet50_golden.py).  Nothing here touches a device.

``forward`` is a functional walk over a STATE DICT, written from the architecture (He et al., "Deep Residual Learning for Image
Recognition", CVPR 2016, in torchvision's v1.5 form: the 3x3 convolution of a bottleneck carries the stride): a 7x7 / 2 stem with
BatchNorm and ReLU, a 3x3 / 2 max pool, four stages of bottlenecks -- 1x1, 3x3 / s, 1x1 to four times the width, each with an
eval-mode BatchNorm, the identity or a 1x1 / s convolution + BatchNorm of the block's input added before the last ReLU -- and the
mean over the map.  The dtype is that of ``x``: float64 gives the truth, float32 the CPU evaluation e_cpu32 of the accuracy rule
bound = 4 * max(e_cpu32, 2^-23 max|y64|)  (tests/hrnet_scenario.py: ``bound`` / ``check``, imported here, not copied).

Recipe.  ``seeded_state_dict(shapes, seed)`` is tests/hrnet_scenario.py's: ONE generator in sorted key order, convolution weights
uniform within +- 1 / sqrt(fan_in), BatchNorm running_mean and bias N(0, 0.1), running_var U(0.6, 1.4), weight U(0.7, 1.3) -- every
BatchNorm's four vectors are random, so every fold is exercised (the initial values 1, 0, 0, 1 would test none).  The last
BatchNorm of each block (bn3) then has its weight multiplied by ``BN3_GAIN``: the residual sum of sixteen blocks stays of the order of
its input instead of growing with the depth; and every down-sample's BatchNorm bias is raised by ``DOWN_BIAS``: an entry block's
sum is then positive more often than not, so that clearly fewer than half of the features are clipped to zero by the last ReLU.
"""
import functools

import torch
import torch.nn.functional as F

from hrnet_scenario import EPS32, bound, check, seeded_state_dict as _seeded, shapes_of   # noqa: F401  (re-exported)

BN_EPS = 1e-5
BN3_GAIN = 0.25
DOWN_BIAS = 0.3
SMALL_LAYERS = (2, 2, 1, 1)
FULL_LAYERS = (3, 4, 6, 3)
# name -> (layers, weight seed, input shape, input seed)
CASES = {
    "small_wino": (SMALL_LAYERS, 50, (3, 18, 64, 64), 0),      # Winograd stem, Winograd 3x3 at 16^2 and 8^2, stride-2 direct
    "small_generic": (SMALL_LAYERS, 50, (2, 18, 40, 24), 1),   # generic stem, every layer direct
    "full": (FULL_LAYERS, 51, (2, 18, 64, 64), 2),
    "production": (FULL_LAYERS, 51, (1, 18, 256, 256), 3),     # every Winograd shape; references computed by the test itself
}
HEAD_WIDTHS = (2048, 1024, 10, 6, 3, 256, 128)


def seeded_state_dict(shapes, seed):
    sd = _seeded(shapes, seed)
    for key in sd:
        if key.endswith(".bn3.weight"):
            sd[key] = sd[key] * BN3_GAIN
        elif key.endswith(".downsample.1.bias"):
            sd[key] = sd[key] + DOWN_BIAS
    return sd


def seeded_input(shape, seed):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(2000 + seed))


def layers_of(sd):
    """Blocks per stage, read off the keys."""
    return tuple(1 + max(int(k.split(".")[1]) for k in sd if k.startswith("layer%d." % li)) for li in (1, 2, 3, 4))


def forward(sd, x):
    """The features (B, 2048) of the Bottleneck encoder with weights ``sd`` (any dtype) for ``x`` (B, C, H, W), in x's dtype."""
    dt = x.dtype
    P = lambda key: sd[key].to(dt)
    bn = lambda y, p: F.batch_norm(y, P(p + ".running_mean"), P(p + ".running_var"), P(p + ".weight"), P(p + ".bias"), False, 0.0, BN_EPS)
    y = F.relu(bn(F.conv2d(x, P("conv1.weight"), None, 2, 3), "bn1"))
    y = F.max_pool2d(y, 3, 2, 1)
    for li, blocks in enumerate(layers_of(sd), 1):
        for bi in range(blocks):
            p = "layer%d.%d." % (li, bi)
            stride = 2 if li > 1 and bi == 0 else 1
            t = F.relu(bn(F.conv2d(y, P(p + "conv1.weight")), p + "bn1"))
            t = F.relu(bn(F.conv2d(t, P(p + "conv2.weight"), None, stride, 1), p + "bn2"))
            t = bn(F.conv2d(t, P(p + "conv3.weight")), p + "bn3")
            if p + "downsample.0.weight" in sd:
                y = bn(F.conv2d(y, P(p + "downsample.0.weight"), None, stride), p + "downsample.1")
            y = F.relu(t + y)
    return y.mean(dim=(2, 3))


def encoder_shapes(layers, in_channels=18):
    """{key: (shape, dtype name)} of the Bottleneck encoder's state dict, from the architecture."""
    shapes = {}

    def conv(key, cout, cin, k):
        shapes[key + ".weight"] = ((cout, cin, k, k), "float32")

    def norm(key, c):
        for leaf in ("weight", "bias", "running_mean", "running_var"):
            shapes["%s.%s" % (key, leaf)] = ((c,), "float32")
        shapes[key + ".num_batches_tracked"] = ((), "int64")

    conv("conv1", 64, in_channels, 7)
    norm("bn1", 64)
    inplanes = 64
    for li, (planes, blocks) in enumerate(zip((64, 128, 256, 512), layers), 1):
        for bi in range(blocks):
            p = "layer%d.%d." % (li, bi)
            conv(p + "conv1", planes, inplanes, 1)
            norm(p + "bn1", planes)
            conv(p + "conv2", planes, planes, 3)
            norm(p + "bn2", planes)
            conv(p + "conv3", planes * 4, planes, 1)
            norm(p + "bn3", planes * 4)
            if bi == 0:
                conv(p + "downsample.0", planes * 4, inplanes, 1)
                norm(p + "downsample.1", planes * 4)
            inplanes = planes * 4
    return shapes


@functools.lru_cache(maxsize=None)
def case(name):
    """(sd, x) of a case; built once, shared, not to be modified."""
    layers, wseed, shape, xseed = CASES[name]
    return seeded_state_dict(encoder_shapes(layers, shape[1]), wseed), seeded_input(shape, xseed)


@functools.lru_cache(maxsize=None)
def references(name):
    """(sd, x, y64, y_cpu32) of a case from this module's own CPU runs; computed once, shared, not to be modified."""
    sd, x = case(name)
    with torch.no_grad():
        return sd, x, forward(sd, x.double()), forward(sd, x)


def build_encoder(layers, sd, in_channels=18):
    """The package's Bottleneck encoder with weights ``sd``, on the CPU, in eval mode."""
    from hierarchicalprobabilistic3dhuman_amd.resnet import Bottleneck, ResNet
    enc = ResNet(list(layers), in_channels, block=Bottleneck)
    enc.load_state_dict(sd, strict=True)
    return enc.eval()


def net_config():
    from hierarchicalprobabilistic3dhuman_amd import configs
    cfg = configs.get_cfg_defaults()
    cfg.MODEL.NUM_RESNET_LAYERS = 50
    return cfg


def net_state_dict(net_cls, parents):
    """The whole net's weights of the fixture: the seed-0 default initialisation of ``net_cls`` (ours or the reference's: the same
    values) with the encoder's tensors replaced by the "full" case's seeded ones."""
    torch.manual_seed(0)
    net = net_cls(parents, net_config())
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    enc_sd, _ = case("full")
    for k, v in enc_sd.items():
        assert sd["image_encoder." + k].shape == v.shape and sd["image_encoder." + k].dtype == v.dtype, k
        sd["image_encoder." + k] = v.clone()
    return sd
