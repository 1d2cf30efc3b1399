"""CPU: the ResNet-50 encoder's public surface -- construction, the reference's state-dict layout and seed-0 initial values
(tests/golden/resnet50_keys.json, resnet50_vectors.npz: tests/golden/make_resnet50_golden.py), the scenario's restatement against
the reference's recorded features, what stays refused for a Bottleneck encoder, and the launch plan's shape."""
import copy
import ctypes
import json
import os
import pickle

import numpy as np
import pytest
import torch

import encoder_call_trace as T
import resnet50_scenario as S
from hierarchicalprobabilistic3dhuman_amd import _capi, configs
from hierarchicalprobabilistic3dhuman_amd.poseMF_shapeGaussian_net import PoseMFShapeGaussianNet
from hierarchicalprobabilistic3dhuman_amd.resnet import BasicBlock, Bottleneck, ResNet, resnet18, resnet50

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def keys():
    with open(os.path.join(GOLDEN, "resnet50_keys.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def vectors():
    z = np.load(os.path.join(GOLDEN, "resnet50_vectors.npz"))
    return {k: torch.from_numpy(z[k]) for k in z.files}


def net50():
    torch.manual_seed(0)
    return PoseMFShapeGaussianNet(configs.SMPL_PARENTS, S.net_config())


def test_the_net_constructs_with_the_resnet50_encoder():
    net = net50()
    enc = net.image_encoder
    assert isinstance(enc, ResNet) and enc.block is Bottleneck and Bottleneck.expansion == 4
    assert [len(l) for l in (enc.layer1, enc.layer2, enc.layer3, enc.layer4)] == [3, 4, 6, 3]
    assert net.fc1.in_features == 2048 and net.fc1.out_features == 1024
    assert net.fc_shape.in_features == 1024 and net.fc_embed.in_features == 2048 + 29
    blk = enc.layer2[0]
    assert blk.conv1.stride == (1, 1) and blk.conv2.stride == (2, 2) and blk.conv3.kernel_size == (1, 1)      # the 3x3 carries the stride
    assert blk.downsample[0].stride == (2, 2) and enc.layer1[0].downsample is not None and enc.layer1[1].downsample is None


def test_state_dict_has_the_references_keys_shapes_and_dtypes(keys):
    layout = lambda sd: [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in sd.items()]
    assert layout(resnet50(18).state_dict()) == keys["encoder"]
    assert layout(net50().state_dict()) == keys["net"]
    assert S.shapes_of(resnet50(18).state_dict()) == S.encoder_shapes(S.FULL_LAYERS)


def test_seed_0_initial_weights_are_the_references(vectors):
    torch.manual_seed(0)
    enc = resnet50(in_channels=18)
    for tag, sd in (("encoder", enc.state_dict()), ("net", net50().state_dict())):
        s = torch.tensor([float(v.double().sum()) for v in sd.values()], dtype=torch.float64)
        q = torch.tensor([float((v.double() ** 2).sum()) for v in sd.values()], dtype=torch.float64)
        assert torch.equal(s, vectors["init_%s_sum" % tag]) and torch.equal(q, vectors["init_%s_sumsq" % tag]), tag


@pytest.mark.parametrize("layers", [34, 101, "50"])
def test_other_depths_raise_a_value_error_naming_the_two(layers):
    cfg = S.net_config()
    cfg.MODEL.NUM_RESNET_LAYERS = layers
    with pytest.raises(ValueError, match="18 or 50"):
        PoseMFShapeGaussianNet(configs.SMPL_PARENTS, cfg)


def test_pretrained_weights_are_refused_as_for_resnet18():
    with pytest.raises(NotImplementedError):
        resnet50(18, pretrained=True)
    with pytest.raises(NotImplementedError):
        resnet18(18, pretrained=True)


@pytest.mark.parametrize("name", ["small_wino", "small_generic", "full"])
def test_the_restatement_reproduces_the_references_features(vectors, name):
    """float32 within 2^-20 max|y| of the reference's float32 features, float64 within 2^-45 max|y| of its .double() features."""
    sd, x = S.case(name)
    with torch.no_grad():
        y32, y64 = S.forward(sd, x), S.forward(sd, x.double())
    r32, r64 = vectors[name + "_feats32"], vectors[name + "_feats64"]
    assert y32.dtype == torch.float32 and y64.dtype == torch.float64 and r64.dtype == torch.float64 and y32.shape == r32.shape
    e32, e64 = float((y32 - r32).abs().max()), float((y64 - r64).abs().max())
    print("%s: max|y32 - ref32| = %.3e (bound %.3e)  max|y64 - ref64| = %.3e (bound %.3e)"
          % (name, e32, 2.0 ** -20 * float(r32.abs().max()), e64, 2.0 ** -45 * float(r64.abs().max())))
    assert e32 <= 2.0 ** -20 * float(r32.abs().max())
    assert e64 <= 2.0 ** -45 * float(r64.abs().max())
    # the recipe: finite, mostly alive, and fp32 close enough to float64 that the accuracy rule is tight
    assert np.isfinite(float(r64.abs().max())) and float((r64 == 0).double().mean()) < 0.5
    assert float((r32.double() - r64).abs().max()) <= 64 * S.EPS32 * float(r64.abs().max())


def test_a_reference_checkpoint_loads_strictly_and_copies_keep_the_block(vectors):
    net = net50().eval()
    ckpt = {"best_model_state_dict": S.net_state_dict(PoseMFShapeGaussianNet, configs.SMPL_PARENTS)}
    missing, unexpected = net.load_state_dict(ckpt["best_model_state_dict"], strict=True)
    assert not missing and not unexpected
    assert torch.equal(net.image_encoder.layer3[5].bn3.weight, ckpt["best_model_state_dict"]["image_encoder.layer3.5.bn3.weight"])
    for clone in (copy.deepcopy(net), pickle.loads(pickle.dumps(net))):
        assert clone.image_encoder.block is Bottleneck and clone.image_encoder._prepared is None and not clone.training
        assert all(torch.equal(a, b) for a, b in zip(clone.state_dict().values(), net.state_dict().values()))


def test_training_paths_of_a_bottleneck_encoder_are_refused():
    net = net50().eval()
    enc = net.image_encoder
    x = torch.rand(1, 18, 64, 64)
    assert any(p.requires_grad for p in enc.parameters())
    with pytest.raises(NotImplementedError, match=r"torch\.no_grad\(\)"):         # grad mode on, parameters requiring grad
        enc(x)
    for p in enc.parameters():
        p.requires_grad_(False)
    with pytest.raises(NotImplementedError, match=r"torch\.no_grad\(\)"):         # ... or the input
        enc(x.requires_grad_(True))
    with pytest.raises(NotImplementedError):
        enc.set_batchnorm_training(True)
    with pytest.raises(NotImplementedError):
        net.set_batchnorm_training(True)
    with pytest.raises(NotImplementedError):
        enc.train()
    with pytest.raises(NotImplementedError):
        net.train()
    assert not enc.training and not enc._bn_training
    enc.eval(), enc.train(False), enc.set_batchnorm_training(False)              # what switches nothing on stays allowed


def test_refresh_weights_drops_the_state_of_a_bottleneck_encoder():
    sd, _ = S.case("small_generic")
    enc = S.build_encoder(S.SMALL_LAYERS, sd)
    prep = enc.prepare()
    assert enc._prepared is prep
    enc.refresh_weights()
    assert enc._prepared is None and enc.device_state() == {}


def test_the_training_loop_refuses_a_50_layer_net_at_entry(tmp_path):
    from hierarchicalprobabilistic3dhuman_amd.train_poseMF_shapeGaussian_net import train_poseMF_shapeGaussian_net
    net = net50().eval()
    with pytest.raises(NotImplementedError, match="ResNet-50"):
        train_poseMF_shapeGaussian_net(net, S.net_config(), None, None, None, torch.device("cpu"), None, None, None, None, [],
                                       str(tmp_path), str(tmp_path / "log.pkl"))
    assert not os.listdir(str(tmp_path))                                          # before anything was touched


def test_resnet18_keeps_its_tree_and_its_capabilities():
    torch.manual_seed(0)
    enc = resnet18(18)
    assert enc.block is BasicBlock and not enc._forward_only
    assert [n for n, _, _ in enc._enc_layers()][:6] == ["stem", "layer1.0.c1", "layer1.0.c2", "layer1.1.c1", "layer1.1.c2", "layer2.0.c1"]
    enc.set_batchnorm_training(True)
    enc.train()
    assert enc.training and enc._bn_training
    prep = enc.prepare()
    c1, c2, down = prep["blocks"][2]                      # layer2.0: a block is still the tuple (c1, c2, down)
    assert prep["blocks"][2].convs == [c1, c2] and prep["blocks"][2].down is down and down is not None


def _trace(monkeypatch, name, **switches):
    sd, x = S.case(name)
    enc = S.build_encoder(S.layers_of(sd), sd)
    enc.composite = switches.pop("composite", True)
    if enc.composite:                      # encoder_call_trace's own table of op kinds predates hps_bottleneck_expand_down
        switches.setdefault("fold_downsample", False)
    if "winograd" in switches:
        enc.set_winograd(switches.pop("winograd"))
    if "latency" in switches:
        enc.set_latency_mode(switches.pop("latency"))
    for k, v in switches.items():
        setattr(enc, k, v)
    with T.recording(monkeypatch) as rec, torch.no_grad():
        feats = enc(x)
    assert feats.shape == (x.shape[0], 2048)
    return enc, rec.rows


CONV = "hps_conv2d_bn_act_pad"
# columns of a hps_conv2d_bn_act_pad row (encoder_call_trace.KIND_ENTRY)
X, W_, RES, Y, H, CIN, COUT, KH, STRIDE, PAD, RELU, KSPLIT = 1, 2, 5, 6, 8, 11, 12, 13, 15, 16, 18, 21


def test_layer_names_follow_prepare(monkeypatch):
    sd, _ = S.case("small_generic")
    enc = S.build_encoder(S.SMALL_LAYERS, sd)
    names = [n for n, _, _ in enc._enc_layers()]
    assert names[:9] == ["stem", "layer1.0.c1", "layer1.0.c2", "layer1.0.c3", "layer1.0.down", "layer1.1.c1", "layer1.1.c2", "layer1.1.c3",
                         "layer2.0.c1"]
    assert len(names) == 1 + 3 * 6 + 4 and enc._block_names() == ["layer1.0", "layer1.1", "layer2.0", "layer2.1", "layer3.0", "layer4.0"]
    prep = enc.prepare()
    convs = ResNet._convs(prep)
    assert len(convs) == len(names)
    for (name, conv, _), cb in zip(enc._enc_layers(), convs):
        assert (cb.cout, cb.cin, cb.kh, cb.stride) == (conv.out_channels, conv.in_channels, conv.kernel_size[0], conv.stride[0]), name
    assert enc._layer_maps(40, 24)["layer2.0.c1"] == (10, 6) and enc._layer_maps(40, 24)["layer2.0.c2"] == (5, 3)
    assert enc._layer_maps(40, 24)["layer2.0.down"] == (5, 3) and enc._layer_maps(40, 24)["layer4.0.c3"] == (2, 1)


@pytest.mark.parametrize("composite", [True, False], ids=["one_call", "per_launch"])
def test_the_plan_of_a_bottleneck_encoder(monkeypatch, composite):
    """Per block: the down-sample on the block's input (1x1 / s, no ReLU), c1 (1x1 / 1, ReLU), c2 (3x3 / s, ReLU; Winograd where the
    map allows), c3 (1x1 / 1 + identity, ReLU); every frame is read where the previous launch wrote it."""
    enc, rows = _trace(monkeypatch, "small_wino", composite=composite, fold_downsample=False)
    assert rows[0][0] == "hps_stem_winograd_pooled_nchw" and rows[-1][0] == "hps_global_avgpool_pad" and len(rows) == 24
    y = rows[0][5]                                                     # the pooled frame
    i = 1
    for name, blk in zip(enc._block_names(), [b for l in (enc.layer1, enc.layer2, enc.layer3, enc.layer4) for b in l]):
        s = blk.conv2.stride[0]
        identity = y
        if blk.downsample is not None:
            d = rows[i]
            assert d[0] == CONV and (d[X], d[KH], d[STRIDE], d[PAD], d[RELU], d[RES]) == (y, 1, s, 0, 0, None), name
            assert d[COUT] == blk.conv3.out_channels
            identity = d[Y]
            i += 1
        c1, c2, c3 = rows[i:i + 3]
        i += 3
        assert c1[0] == CONV and (c1[X], c1[KH], c1[STRIDE], c1[PAD], c1[RELU], c1[RES]) == (y, 1, 1, 0, 1, None), name
        if c2[0] == "hps_conv3x3_winograd":
            assert s == 1 and c2[1] == c1[Y] and c2[5] is None and c2[14] == 1 and c2[8] in (16, 8), name      # x, residual, relu, H
            c2y = c2[6]
        else:
            assert c2[0] == CONV and (c2[X], c2[KH], c2[STRIDE], c2[PAD], c2[RELU], c2[RES]) == (c1[Y], 3, s, 1, 1, None), name
            c2y = c2[Y]
        assert c3[0] == CONV and (c3[X], c3[KH], c3[STRIDE], c3[PAD], c3[RELU], c3[RES]) == (c2y, 1, 1, 0, 1, identity), name
        assert c3[KSPLIT] == 1 and c1[KSPLIT] == 1
        y = c3[Y]
    assert i == 23 and rows[-1][1] == y and rows[-1][6] == 2048
    assert sum(r[0] == "hps_conv3x3_winograd" for r in rows) == 3          # layer1.0, layer1.1 (16 x 16), layer2.1 (8 x 8)


def test_no_winograd_and_latency_plans_run_every_layer_direct(monkeypatch):
    _, rows = _trace(monkeypatch, "small_wino", winograd=False)
    assert not any("winograd" in r[0] for r in rows[1:]) and rows[0][0] == "hps_nchw_to_padded_nhwc"
    _, lat = _trace(monkeypatch, "small_wino", latency=True)
    assert not any("winograd" in r[0] for r in lat)
    convs = [r for r in lat if r[0] == CONV][1:]                              # behind the stem
    assert all(r[20] == 5 for r in convs)                                      # 64 x 64 tiles, four stages
    assert all(r[KSPLIT] == 1 for r in convs if r[KH] == 1)                    # the 1x1 layers are never split over K
    _, generic = _trace(monkeypatch, "small_generic")
    assert not any("winograd" in r[0] for r in generic) and len(generic) == 26


def test_struct_mirror_has_the_librarys_size():
    lib = _capi.load()
    assert lib.hps_sizeof_enc_op() == ctypes.sizeof(_capi.EncOp)
    assert [n for n, _ in _capi.EncOp._fields_][-3:] == ["x_down", "ipad_down", "Cin_down"]      # appended at the end
    assert lib.hps_version() == 502 and "hps_bottleneck_expand_down" in _capi.EXPORTED_SYMBOLS


def test_expand_down_rejects_bad_arguments_on_the_host():
    """Null pointers, Cout % 64, Cin % 32, Cmid % 32, stride 3, a split-K request, an unknown variant, tensors beyond the 32-bit lane
    offsets: each refused with a message before any launch (no device here)."""
    lib = _capi.load()
    p = ctypes.c_void_p(64)
    ok = dict(B=2, H=8, W=8, stride=2, tpad=1, xpad=1, opad=1, Cmid=64, Cin=128, Cout=256, variant=0, ksplit=1)
    order = ("B", "H", "W", "stride", "tpad", "xpad", "opad", "Cmid", "Cin", "Cout", "variant", "ksplit")

    def call(ptrs=None, **kw):
        a = dict(ok, **kw)
        return lib.hps_bottleneck_expand_down(*(ptrs or [p] * 9), *[a[k] for k in order], None)

    for i in range(9):
        ptrs = [p] * 9
        ptrs[i] = None
        assert call(ptrs) == -1 and b"null pointer" in lib.hps_last_error(), i
    for kw, msg in ((dict(Cout=96), b"Cout % 64"), (dict(Cin=48), b"Cin % 32"), (dict(Cmid=16), b"Cmid % 32"), (dict(stride=3), b"stride"),
                    (dict(stride=0), b"stride"), (dict(ksplit=2), b"split K"), (dict(variant=4), b"variant"), (dict(H=0), b"H, W"),
                    (dict(opad=-1), b"halos"), (dict(B=4096, H=512, W=512), b"32-bit lane offsets")):
        assert call(**kw) == -1 and msg in lib.hps_last_error(), kw
    ops = (_capi.EncOp * 1)(_capi.EncOp(kind=_capi.ENC_EXPAND_DOWN))                 # through the composite too
    assert lib.hps_encoder_run(ops, 1, None) == -1 and b"hps_bottleneck_expand_down: null pointer" in lib.hps_last_error()
    assert call(B=0) == 0                                                            # nothing to do


def test_fold_downsample_puts_the_entry_blocks_down_sample_into_the_expand_launch(monkeypatch):
    """fold_downsample on: per entry block one hps_bottleneck_expand_down instead of the down-sample's launch and conv3's; it reads c2's
    frame and the block's input, and no frame of the identity exists.  In latency mode as well (no 1x1 layer is split over K); a layer
    with K slices asked for by hand takes the two launches."""
    enc, on = _trace(monkeypatch, "small_wino", composite=False, fold_downsample=True)
    _, off = _trace(monkeypatch, "small_wino", composite=False, fold_downsample=False)
    fused = [r for r in on if r[0] == "hps_bottleneck_expand_down"]
    assert len(fused) == 4 and len(on) == len(off) - 4
    assert [(r[10], r[11], r[12], r[13], r[17], r[18], r[19]) for r in fused] == [(3, 16, 16, 1, 64, 64, 256), (3, 16, 16, 2, 128, 256, 512),
                                                                                 (3, 8, 8, 2, 256, 512, 1024), (3, 4, 4, 2, 512, 1024, 2048)]
    assert all(r[14:17] == [1, 1, 1] and r[20:] == [0, 1] for r in fused)          # halos; automatic tile, no K slices
    i = on.index(fused[0])
    assert fused[0][5] == on[0][5] and fused[0][1] == on[i - 1][6]                   # x = the pooled frame, t = c2's (Winograd) output
    fs = next(iter(enc._frames.values()))
    assert [e["down"] is None for e in fs["blocks"]] == [True, True, True, True, True, True]
    _, lat = _trace(monkeypatch, "small_wino", composite=False, fold_downsample=True, latency=True)
    assert sum(r[0] == "hps_bottleneck_expand_down" for r in lat) == 4 and all(r[20] == 5 for r in lat if r[0] == "hps_bottleneck_expand_down")
    sd, x = S.case("small_generic")
    enc = S.build_encoder(S.SMALL_LAYERS, sd)
    enc.composite = False
    prep = enc.prepare()
    prep["blocks"][2].down.ksplit = 2                                                # layer2.0's down-sample in two K slices, by hand
    with T.recording(monkeypatch) as rec, torch.no_grad():
        enc(x)
    assert sum(r[0] == "hps_bottleneck_expand_down" for r in rec.rows) == 3
    two = [r for r in rec.rows if r[0] == CONV and r[KSPLIT] == 2]
    assert len(two) == 1 and two[0][COUT] == 512 and two[0][RELU] == 0
