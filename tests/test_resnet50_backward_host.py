"""CPU: the Bottleneck encoder's backward opt-in (ResNet.set_differentiable), the 1x1 backward kernels' host-side refusals and
workspace bound (csrc/conv1x1_backward.hip), and resnet50_grad_scenario's restatement against its own sources."""
import copy
import ctypes
import pickle

import pytest
import torch

import resnet50_grad_scenario as GS
import resnet50_scenario as S
from hierarchicalprobabilistic3dhuman_amd import _capi
from hierarchicalprobabilistic3dhuman_amd.resnet import resnet18

NEW_SYMBOLS = ("hps_conv1x1_dgrad", "hps_conv1x1_wgrad", "hps_conv1x1_wgrad_slice_pixels", "hps_conv1x1_wgrad_workspace")


# ---- the restatement against its own sources ----
@pytest.mark.parametrize("name", ["small_wino", "small_generic"])
def test_the_restatement_is_the_scenarios_forward_and_plain_autograd(name):
    """With its own pins the restatement's features equal resnet50_scenario.forward bit for bit; its float64 VJP equals plain
    F.conv2d / F.batch_norm / F.relu / F.max_pool2d autograd in float64 to 2^-40 relative."""
    sd, x, cot = GS.case(name)
    with torch.no_grad():
        feats, maps = GS.forward(sd, x)
        assert torch.equal(feats, S.forward(sd, x))
        pinned, _ = GS.forward(sd, x, GS.self_pins(name))
        assert torch.equal(pinned, feats)
    assert {k for k in maps if k.endswith(".c3")} == {"layer%d.%d.c3" % (l, b) for l, n in enumerate(S.SMALL_LAYERS, 1) for b in range(n)}
    # float64: the pinned run's masks are the float64 run's own here, so both functions are the same function
    sd64 = {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}
    with torch.no_grad():
        pins64 = GS.pins_from_maps(GS.forward(sd64, x.double())[1])
    g_pinned = GS.vjp(sd, x, pins64, cot, torch.float64)
    g_plain = GS.vjp(sd, x, None, cot, torch.float64, fn=GS.plain_forward)
    assert set(g_pinned) == set(g_plain) and "input" in g_pinned and "layer4.0.conv3.weight" in g_pinned
    worst = 0.0
    for k in g_plain:
        rel = float((g_pinned[k] - g_plain[k]).abs().max()) / max(float(g_plain[k].abs().max()), 1e-300)
        worst = max(worst, rel)
        assert rel <= 2.0 ** -40, (k, rel)
    print("%s: worst relative difference of the pinned restatement to plain float64 autograd %.3e" % (name, worst))


@pytest.mark.parametrize("name", ["small_wino", "small_generic"])
def test_the_training_restatement_is_plain_autograd_on_batch_statistics(name):
    """Every BatchNorm on batch statistics: the pinned float64 VJP equals plain F.batch_norm(training=True) autograd to 2^-40 relative;
    update=True moves the buffers as torch does, the default leaves them alone."""
    sd, x, cot = GS.case(name)
    sd64 = {k: v.double() if v.is_floating_point() else v.clone() for k, v in sd.items()}
    with torch.no_grad():
        _, maps, stats = GS.forward_train(sd64, x.double())
        assert all(torch.equal(sd64[k], sd[k].double()) for k in sd if "running" in k)            # no update
    assert len(stats) == 1 + 3 * 6 + 4 and stats["layer4.0.c3"][2] == x.shape[0] * (4 if name == "small_wino" else 2)
    g_pinned, _ = GS.vjp_train(sd, x, GS.pins_from_maps(maps), cot, torch.float64)
    g_plain = GS.vjp(sd, x, None, cot, torch.float64, fn=GS.plain_forward_train)
    worst = 0.0
    for k in g_plain:
        rel = float((g_pinned[k] - g_plain[k]).abs().max()) / max(float(g_plain[k].abs().max()), 1e-300)
        worst = max(worst, rel)
        assert rel <= 2.0 ** -40, (k, rel)
    print("%s training: worst relative difference to plain float64 autograd %.3e" % (name, worst))
    with torch.no_grad():
        GS.forward_train(sd64, x.double(), update=True)
    mean, var, n = stats["layer2.0.down"]
    assert int(sd64["layer2.0.downsample.1.num_batches_tracked"]) == int(sd["layer2.0.downsample.1.num_batches_tracked"]) + 1
    want = 0.9 * sd["layer2.0.downsample.1.running_var"].double() + 0.1 * var * n / (n - 1.0)
    assert float((sd64["layer2.0.downsample.1.running_var"] - want).abs().max()) <= 1e-12 * float(want.abs().max())


# ---- the switch ----
def test_the_switch_is_off_by_default_and_a_property_of_the_model():
    sd, _ = S.case("small_generic")
    enc = S.build_encoder(S.SMALL_LAYERS, sd)
    assert enc._forward_only and enc.gemm_backward is True
    enc.set_differentiable(True)
    assert not enc._forward_only
    for clone in (copy.deepcopy(enc), pickle.loads(pickle.dumps(enc))):
        assert not clone._forward_only and clone.gemm_backward is True
    enc.load_state_dict(sd)
    assert not enc._forward_only                                       # survives load_state_dict
    enc.set_differentiable(False)
    assert enc._forward_only
    with pytest.raises(NotImplementedError, match=r"torch\.no_grad\(\)"):         # today's message comes back
        enc(torch.rand(1, 18, 64, 64))
    prep = enc.prepare()
    enc.refresh_weights()
    assert enc._prepared is None and prep is not None                  # ... and today's refresh: the state is dropped


def test_the_switch_on_a_basic_block_encoder():
    torch.manual_seed(0)
    enc = resnet18(18)
    enc.set_differentiable(True)                                       # always on: a no-op
    enc.set_differentiable()
    assert not enc._forward_only
    with pytest.raises(ValueError, match="always differentiable"):
        enc.set_differentiable(False)
    assert not enc._forward_only


def test_the_switch_opens_the_backward_and_training_batchnorm():
    """With the switch on a forward under grad mode is no longer refused as forward only (on the CPU it gets as far as the refusal of a
    CPU tensor); set_batchnorm_training(True) and then .train() are accepted and _train_flags() names every c3.  With it off, today's
    messages come back."""
    sd, _ = S.case("small_generic")
    enc = S.build_encoder(S.SMALL_LAYERS, sd)
    with pytest.raises(NotImplementedError, match="training-mode BatchNorm"):
        enc.set_batchnorm_training(True)
    enc.set_differentiable(True)
    with pytest.raises(_capi.HpsError):                                # not NotImplementedError: the route is open, the tensor is on the CPU
        enc(torch.rand(1, 18, 40, 24))
    with pytest.raises(RuntimeError, match="set_batchnorm_training"):  # .train() alone: the ResNet-18 behaviour (refused at the forward)
        enc.train()
        enc._train_flags()
    enc.eval()
    enc.set_batchnorm_training(True)
    assert enc._train_flags() is None                                  # nothing is training yet
    enc.train()
    flags = enc._train_flags()
    assert enc.training and all(flags.values()) and len(flags) == 1 + 3 * 6 + 4
    assert {n for n in flags if n.endswith(".c3")} == {"layer%d.%d.c3" % (l, b) for l, n in enumerate(S.SMALL_LAYERS, 1) for b in range(n)}
    enc.layer1.eval()
    flags = enc._train_flags()
    assert not flags["layer1.0.c3"] and not flags["layer1.0.down"] and flags["layer2.0.c3"] and flags["stem"]
    enc._check_training(flags, (2, 18, 40, 24))                        # n = 4 samples per channel in layer4: accepted
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        enc._check_training(flags, (1, 18, 24, 24))                    # layer4 on a 1 x 1 map of one image: torch's own refusal
    for clone in (copy.deepcopy(enc), pickle.loads(pickle.dumps(enc))):
        assert not clone._forward_only and clone._bn_training and clone.training
    enc.eval()
    enc.set_batchnorm_training(False)
    enc.set_differentiable(False)
    with pytest.raises(NotImplementedError, match="training-mode BatchNorm"):
        enc.set_batchnorm_training(True)
    with pytest.raises(NotImplementedError, match="training-mode BatchNorm"):
        enc.train()
    assert not enc.training and not enc._bn_training


def test_the_net_passes_the_switch_through_and_the_loop_refuses_without_it(tmp_path):
    import os
    import test_resnet50_host as H
    from hierarchicalprobabilistic3dhuman_amd.train_poseMF_shapeGaussian_net import train_poseMF_shapeGaussian_net
    net = H.net50().eval()
    assert net.image_encoder._forward_only
    net.set_differentiable_encoder(True)
    assert not net.image_encoder._forward_only
    net.set_batchnorm_training(True)
    net.train()
    assert net.image_encoder.training and net.image_encoder._train_flags()["layer4.2.c3"]
    net.eval()
    net.set_batchnorm_training(False)
    net.set_differentiable_encoder(False)
    with pytest.raises(NotImplementedError, match="runs forward"):     # the present message, before anything was touched
        train_poseMF_shapeGaussian_net(net, S.net_config(), None, None, None, torch.device("cpu"), None, None, None, None, [],
                                       str(tmp_path), str(tmp_path / "log.pkl"))
    assert not os.listdir(str(tmp_path))


def test_the_routing_rules_are_rules_on_the_layer_alone():
    sd, _ = S.case("small_generic")
    enc = S.build_encoder(S.SMALL_LAYERS, sd)
    prep = enc.prepare()
    by_name = dict(zip([n for n, _, _ in enc._enc_layers()], type(enc)._convs(prep)))
    assert not enc._gemm_dgrad(by_name["stem"]) and not enc._gemm_dgrad(by_name["layer1.0.c2"])
    for name, cb in by_name.items():
        if cb.kh == 1:
            assert enc._gemm_dgrad(cb), name
            assert enc._gemm_wgrad(cb) == (cb.cin * cb.cout >= 16384 and (cb.stride == 1 or cb.cout >= 1024)), name
    assert not enc._gemm_wgrad(by_name["layer1.0.c1"]) and enc._gemm_wgrad(by_name["layer1.0.c3"])       # 64 -> 64 stays, 64 -> 256 goes
    assert not enc._gemm_wgrad(by_name["layer2.0.down"]) and enc._gemm_wgrad(by_name["layer3.0.down"])   # 256 -> 512 / 2 is ResNet-18's too
    enc.gemm_backward = False
    assert not any(enc._gemm_dgrad(cb) or enc._gemm_wgrad(cb) for cb in by_name.values())
    torch.manual_seed(0)
    r18 = resnet18(18)                                                  # its three down-samples keep hps_conv_wgrad (their bits are pinned)
    assert not any(r18._gemm_wgrad(cb) for cb in type(r18)._convs(r18.prepare()))


# ---- the kernels' host side ----
def test_symbols_are_declared_and_bound():
    lib = _capi.load()
    assert lib.hps_version() == 502
    for name in NEW_SYMBOLS:
        assert name in _capi.EXPORTED_SYMBOLS and hasattr(lib, name)


def test_conv1x1_backward_rejects_bad_arguments_on_the_host():
    """Null pointers, Cout % 8, a stride other than 1 or 2, Cdx < Cin, other == dx, negative halos, frames of 2^31 pixels: each refused
    with a message before any launch (no device here)."""
    lib = _capi.load()
    p, q = ctypes.c_void_p(64), ctypes.c_void_p(128)
    ok = dict(B=2, H=8, W=8, Cin=64, Cout=128, stride=2, gpad=1, dpad=1, Cdx=64)

    def dgrad(ptrs=None, **kw):
        a = dict(ok, **kw)
        return lib.hps_conv1x1_dgrad(*(ptrs or [p, p, None, q]), *[a[k] for k in ("B", "H", "W", "Cin", "Cout", "stride", "gpad", "dpad", "Cdx")], None)

    for i in (0, 1, 3):
        ptrs = [p, p, None, q]
        ptrs[i] = None
        assert dgrad(ptrs) == -1 and b"hps_conv1x1_dgrad: null pointer" in lib.hps_last_error(), i
    assert dgrad([p, p, q, q]) == -1 and b"alias" in lib.hps_last_error()
    for kw, msg in ((dict(Cout=12), b"Cout % 8"), (dict(stride=3), b"stride"), (dict(stride=0), b"stride"), (dict(Cdx=63), b"Cdx >= Cin"),
                    (dict(gpad=-1), b"gpad"), (dict(H=0), b"geometry"), (dict(B=70000, H=256, W=256, stride=1), b"2^31")):
        assert dgrad(**kw) == -1 and msg in lib.hps_last_error(), kw

    okw = dict(B=2, H=8, W=8, ipad=1, Cx=64, Cin=64, Cout=128, stride=2, gpad=1)

    def wgrad(ptrs=None, **kw):
        a = dict(okw, **kw)
        return lib.hps_conv1x1_wgrad(*(ptrs or [p] * 4), *[a[k] for k in ("B", "H", "W", "ipad", "Cx", "Cin", "Cout", "stride", "gpad")], None)

    for i in range(4):
        ptrs = [p] * 4
        ptrs[i] = None
        assert wgrad(ptrs) == -1 and b"hps_conv1x1_wgrad: null pointer" in lib.hps_last_error(), i
    for kw, msg in ((dict(Cout=12), b"Cout % 8"), (dict(stride=4), b"stride"), (dict(Cx=60), b"Cx >= Cin"), (dict(ipad=-1), b"ipad"),
                    (dict(W=0), b"geometry"), (dict(B=70000, H=256, W=256, stride=1), b"2^31")):
        assert wgrad(**kw) == -1 and msg in lib.hps_last_error(), kw
    w = lib.hps_conv1x1_wgrad_workspace
    assert w(0, 8, 8, 64, 64, 1) == 0 and w(2, 8, 8, 64, 64, 3) == 0 and w(2, 8, 8, 64, 64, 1) == 64 * 64 * 4
    assert lib.hps_conv1x1_wgrad_slice_pixels(0, 64) == 0


def test_the_slice_rule_and_the_workspace_bound_for_the_layer_table():
    """The slice length is a rule on (Cin, Cout) alone: twice their harmonic mean rounded up to 64 pixels, at least 1024.  For every
    1x1 layer of ResNet-50 at B = 72 on 256 x 256 inputs the workspace is no larger than the layer's two operand frames together (the
    header states 0.42 of them), with far fewer slices than hps_conv_wgrad cuts."""
    lib = _capi.load()
    s = lib.hps_conv1x1_wgrad_slice_pixels
    assert s(64, 64) == 1024 and s(64, 256) == 1024 and s(2048, 512) == 1024 and s(512, 2048) == 1024 and s(1024, 2048) == 1408
    assert all(s(a, b) % 64 == 0 for a in (8, 40, 72, 264, 1000) for b in (8, 64, 2048))
    layers = GS.resnet50_1x1_layers()
    assert len(layers) == 15 and (2048, 512, 1, 8) in layers and (1024, 2048, 2, 16) in layers and (64, 64, 1, 64) in layers
    B, worst = 72, 0.0
    for cin, cout, stride, hw in layers:
        ho = (hw - 1) // stride + 1
        ws = lib.hps_conv1x1_wgrad_workspace(B, hw, hw, cin, cout, stride)
        slices = -(-B * ho * ho // s(cin, cout))
        assert ws == slices * cin * cout * 4
        operands = 4 * B * ((hw + 2) ** 2 * cin + (ho + 2) ** 2 * cout)          # the two frames with their halos
        old = lib.hps_conv_wgrad_workspace(B, hw, hw, cin, cout, 1, 1, stride, 0)
        worst = max(worst, ws / operands)
        print("%4d -> %4d / %d on %2d x %2d: %3d slices, workspace %6.2f MB = %.3f of the operands (hps_conv_wgrad: %d slices, %.2f MB)"
              % (cin, cout, stride, hw, hw, slices, ws / 2 ** 20, ws / operands, old // (cin * cout * 4), old / 2 ** 20))
        # at least 1024 pixels a slice against at most 512: half as many slices or fewer (a seventh on layer4's 8 x 8 maps)
        assert ws <= operands and slices * 2 <= old // (cin * cout * 4)
    assert worst <= 0.42
    assert lib.hps_conv1x1_wgrad_workspace(72, 8, 8, 512, 2048, 1) == 5 * 2048 * 512 * 4
    assert lib.hps_conv_wgrad_workspace(72, 8, 8, 512, 2048, 1, 1, 1, 0) == 36 * 2048 * 512 * 4
