"""CPU: the HRNet module's parameter tree, its config defaults, the float64 restatement the GPU tests are held to, the refusals and
the host-side argument validation of the new entry points.  No device is touched.

    state dict       keys, shapes and dtypes of PoseHighResolutionNet(defaults) == the reference's (tests/golden/hrnet_w48_keys.json)
    forward64        tests/hrnet_scenario.forward64 == the reference's float64 heat maps (tests/golden/hrnet_vectors.npz) to
                     1e-10 max|y|: both sides are float64 torch on the CPU running the same operations
"""
import copy
import ctypes
import json
import os
import pickle

import numpy as np
import pytest
import torch

import hrnet_scenario as S
from hierarchicalprobabilistic3dhuman_amd import _capi, configs
from hierarchicalprobabilistic3dhuman_amd.pose2D_hrnet import PoseHighResolutionNet, get_pose_net

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def w48():
    return PoseHighResolutionNet(S.config("W48"))


def test_state_dict_has_the_reference_keys_shapes_and_dtypes(w48):
    want = [(k, tuple(s), d) for k, s, d in json.load(open(os.path.join(GOLDEN, "hrnet_w48_keys.json")))]
    got = [(k, tuple(v.shape), str(v.dtype).replace("torch.", "")) for k, v in w48.state_dict().items()]
    assert len(want) == 1754 and sum(1 for k, _, _ in want if k.endswith("num_batches_tracked")) > 0
    assert dict((k, (s, d)) for k, s, d in got) == dict((k, (s, d)) for k, s, d in want)
    assert [k for k, _, _ in got] == [k for k, _, _ in want]                       # the reference's order too
    assert sum(p.numel() for p in w48.parameters()) == 63595745                    # the reference class's own count
    # a checkpoint with exactly these entries loads strictly
    sd = S.seeded_state_dict({k: (s, d) for k, s, d in want}, 3)
    get_pose_net(S.config("W48"), is_train=False).load_state_dict(sd, strict=True)


@pytest.mark.parametrize("name", sorted(S.GOLDEN_INPUTS))
def test_forward64_reproduces_the_reference_heat_maps(name):
    z = np.load(os.path.join(GOLDEN, "hrnet_vectors.npz"))
    want = torch.from_numpy(z[name])
    net = PoseHighResolutionNet(S.config(name))
    shapes = S.shapes_of(net.state_dict())
    sd, x, y64, y32 = S.references(name, S.GOLDEN_INPUTS[name], 0, S.shapes_key(shapes))
    net.load_state_dict(sd, strict=True)
    assert y64.dtype == torch.float64 and y64.shape == want.shape
    err, scale = float((y64 - want).abs().max()), float(want.abs().max())
    print("%s forward64 vs reference float64: max|diff| = %.3e, max|y| = %.3e" % (name, err, scale))
    assert err <= 1e-10 * scale
    assert y32.dtype == torch.float32 and float((y32.double() - y64).abs().max()) < 1e-4 * scale


def test_config_defaults_equal_the_reference_values():
    c = configs.get_pose2D_hrnet_cfg_defaults()
    assert c.MODEL.NUM_JOINTS == 17 and c.MODEL.IMAGE_SIZE == [288, 384] and c.MODEL.HEATMAP_SIZE == [72, 96]
    e = c["MODEL"]["EXTRA"]
    assert e.PRETRAINED_LAYERS == ["conv1", "bn1", "conv2", "bn2", "layer1", "transition1", "stage2", "transition2", "stage3",
                                   "transition3", "stage4"]
    assert e.FINAL_CONV_KERNEL == 1
    want = {"STAGE2": (1, 2, [4, 4], [48, 96]), "STAGE3": (4, 3, [4, 4, 4], [48, 96, 192]),
            "STAGE4": (3, 4, [4, 4, 4, 4], [48, 96, 192, 384])}
    for name, (mods, branches, blocks, chans) in want.items():
        st = e[name]
        assert (st.NUM_MODULES, st.NUM_BRANCHES, st.BLOCK, st.NUM_BLOCKS, st.NUM_CHANNELS, st.FUSE_METHOD) == \
            (mods, branches, "BASIC", blocks, chans, "SUM")
    assert c.TEST.POST_PROCESS is False and c.TEST.OBJECT_DET_THRESH == 0.95
    c.MODEL.EXTRA.STAGE2.NUM_CHANNELS[0] = 1                     # a fresh object per call
    assert configs.get_pose2D_hrnet_cfg_defaults().MODEL.EXTRA.STAGE2.NUM_CHANNELS == [48, 96]


def test_refusals_fire_without_a_gpu():
    cfg = S.config("NARROW")
    net = PoseHighResolutionNet(cfg)
    x = torch.zeros(1, 3, 32, 32)
    with pytest.raises(RuntimeError, match="eval"):              # a fresh module is in training mode
        net(x)
    net.eval()
    with pytest.raises(RuntimeError, match="requires grad"):
        net(x.clone().requires_grad_(True))
    with pytest.raises(_capi.HpsError, match="no CPU path"):
        net(x)
    bad = S.config("NARROW")
    bad["MODEL"]["EXTRA"]["STAGE3"]["FUSE_METHOD"] = "CAT"
    with pytest.raises(_capi.HpsError, match="FUSE_METHOD"):
        PoseHighResolutionNet(bad)
    bad = S.config("NARROW")
    bad["MODEL"]["EXTRA"]["FINAL_CONV_KERNEL"] = 5
    with pytest.raises(_capi.HpsError, match="FINAL_CONV_KERNEL"):
        PoseHighResolutionNet(bad)
    bad = S.config("NARROW")                                     # an existing branch changes its width between stages
    bad["MODEL"]["EXTRA"]["STAGE3"]["NUM_CHANNELS"] = [32, 32, 64]
    with pytest.raises(_capi.HpsError, match="width of an existing branch"):
        PoseHighResolutionNet(bad)
    ok = S.config("NARROW")
    ok["MODEL"]["EXTRA"]["FINAL_CONV_KERNEL"] = 3
    assert PoseHighResolutionNet(ok).final_layer.padding == (1, 1)


def test_copies_and_reloads_drop_the_prepared_state():
    net = PoseHighResolutionNet(S.config("NARROW")).eval()
    net._prepared = {"stale": 1}
    state = net.device_state()
    for clone in (copy.deepcopy(net), pickle.loads(pickle.dumps(net))):
        assert clone._prepared is None and clone.device_state() == {}
        assert [k for k in clone.state_dict()] == [k for k in net.state_dict()]
    assert net._prepared == {"stale": 1} and net.device_state() is state
    net.load_state_dict(net.state_dict())
    assert net._prepared is None and net.device_state() is not state
    prep = net.prepare()                                          # the fold itself needs no device
    layer = prep[id(net.final_layer)]
    assert layer.w.shape == (1, 32, 16) and bool((layer.w[:, 17:] == 0).all()) and bool((layer.scale == 1).all())
    assert torch.equal(layer.shift, net.final_layer.bias.detach())
    stem = prep[id(net.conv1)]
    assert stem.w.shape == (9, 64, 16) and bool((stem.w[:, :, 3:] == 0).all())


def _problem(**kw):
    p = dict(x=16, w=16, scale=16, shift=16, residual=None, y=16, B=1, H=8, W=8, ipad=1, Cin=16, Cout=16, K=3, stride=1, opad=0, relu=1)
    p.update(kw)
    return _capi.C16Problem(**p)


def test_argument_validation_of_the_new_entry_points_needs_no_gpu():
    lib = _capi.load()
    assert lib.hps_sizeof_c16_problem() == ctypes.sizeof(_capi.C16Problem)
    assert lib.hps_sizeof_hrnet_fuse_args() == ctypes.sizeof(_capi.HrnetFuseArgs)
    assert lib.hps_sizeof_hrnet_op() == ctypes.sizeof(_capi.HrnetOp)

    def conv(n, *problems):
        arr = (_capi.C16Problem * max(len(problems), 1))(*problems)
        return lib.hps_conv2d_bn_act_c16(arr, n, None), lib.hps_last_error()

    assert lib.hps_conv2d_bn_act_c16(None, 1, None) == -1 and b"null pointer" in lib.hps_last_error()
    for kw, msg in (({"x": None}, b"null pointer"), ({"y": None}, b"null pointer"), ({"Cin": 24}, b"Cin % 16"), ({"K": 5}, b"filter size"),
                    ({"K": 2}, b"filter size"), ({"stride": 3}, b"stride"), ({"ipad": 0}, b"halo"), ({"Cout": 0}, b"Cout"),
                    ({"x": 8}, b"aligned")):
        rc, err = conv(1, _problem(**kw))
        assert rc == -1 and msg in err, (kw, err)
    rc, err = conv(5, *[_problem()] * 5)
    assert rc == -1 and b"1 to 4 problems" in err
    rc, err = conv(2, _problem(), _problem(Cin=8))               # every problem of a group is checked before anything is launched
    assert rc == -1 and b"Cin % 16" in err
    assert conv(0)[0] == 0 and conv(1, _problem(B=0))[0] == 0     # nothing to do

    fuse = lambda **kw: _capi.HrnetFuseArgs(**dict(dict(n_terms=1, y=16, opad=1, B=0, H=8, W=8, C=16, relu=1), **kw))
    a = fuse()
    a.term[0] = 16
    assert lib.hps_hrnet_fuse(ctypes.byref(a), None) == 0        # B == 0
    assert lib.hps_hrnet_fuse(None, None) == -1 and b"null pointer" in lib.hps_last_error()
    a = fuse()
    assert lib.hps_hrnet_fuse(ctypes.byref(a), None) == -1 and b"null pointer" in lib.hps_last_error()
    a = fuse(n_terms=5)
    assert lib.hps_hrnet_fuse(ctypes.byref(a), None) == -1 and b"1 to 4 terms" in lib.hps_last_error()
    a = fuse(H=12)
    a.term[0], a.shift[0] = 16, 3
    assert lib.hps_hrnet_fuse(ctypes.byref(a), None) == -1 and b"shift" in lib.hps_last_error()
    a = fuse(C=18)
    a.term[0] = 16
    assert lib.hps_hrnet_fuse(ctypes.byref(a), None) == -1 and b"C % 4" in lib.hps_last_error()

    assert lib.hps_hrnet_pack_input(None, None, 1, 8, 8, 16, 1, None) == -1 and b"null pointer" in lib.hps_last_error()
    assert lib.hps_hrnet_pack_input(16, 16, 1, 8, 8, 3, 1, None) == -1
    assert lib.hps_hrnet_unpack_output(None, None, 1, 8, 8, 17, 0, None) == -1 and b"null pointer" in lib.hps_last_error()
    assert lib.hps_hrnet_run(None, 0, None) == 0
    assert lib.hps_hrnet_run(None, 1, None) == -1 and b"null op list" in lib.hps_last_error()
    ops = (_capi.HrnetOp * 1)(_capi.HrnetOp(kind=99))
    assert lib.hps_hrnet_run(ops, 1, None) == -1 and b"unknown op kind" in lib.hps_last_error()
    ops = (_capi.HrnetOp * 1)(_capi.HrnetOp(kind=_capi.HRNET_CONV, n_problems=1))
    assert lib.hps_hrnet_run(ops, 1, None) == -1 and b"null pointer" in lib.hps_last_error()
