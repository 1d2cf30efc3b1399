"""GPU: the ResNet-50 (Bottleneck) encoder and the net around it.

Encoder features are held to float64: the reference's own ``.double()`` features recorded in tests/golden/resnet50_vectors.npz
(tests/golden/make_resnet50_golden.py) for the small [2, 2, 1, 1] encoder and the full resnet50 on 64 x 64 inputs, the scenario's
own float64 run (tests/resnet50_scenario.py, pinned to the reference by tests/test_resnet50_host.py) at the production geometry.
Rule of the direct route and the latency mode: max|dev - y64| <= 4 max(e_cpu32, 2^-23 max|y64|) (tests/hrnet_scenario.py).  The
Winograd route is held to the same truth with the bound tests/test_gpu_net.py uses for it, 1e-4 max|y64|.  The switches the
project declares bit-identical are compared bit for bit.  The head at the widths of the 50-layer net (2048 features, fc1 1024 wide)
goes by tests/head_forward_scenario.py's rules as they stand; the whole net by the tolerances tests/test_gpu_net.py uses for the
18-layer one.  Every test prints its figures.

Measured on an MI355X, worst err / bound: encoder direct 0.60, latency 0.57, Winograd route 0.0041 (3.4 units of 2^-23 max|y64|);
head at 2048 x 1024 1.96 units of the fp32 rule's 4 (mode), refine 1.43 of the float64 rule's 8; whole net against the reference:
features 4.5e-7 relative, pose_S 4.6e-7, mode 1.5e-6, loc / scale / glob / cam 1.2e-7, pose_F 3.6e-7 (printed, not asserted).
"""
import copy
import os

import numpy as np
import pytest
import torch

import head_forward_scenario as FS
import resnet50_scenario as S
from conftest import maxerr
from hierarchicalprobabilistic3dhuman_amd import configs
from hierarchicalprobabilistic3dhuman_amd.poseMF_shapeGaussian_net import PoseMFShapeGaussianNet
from hierarchicalprobabilistic3dhuman_amd.predict_poseMF_shapeGaussian_net import GraphedInfer, InferencePipeline, infer
from test_gpu_head_forward import forward as head_forward, kernel_weights, refine, run_trunk

pytestmark = pytest.mark.gpu

WINOGRAD_TOL = 1e-4          # tests/test_gpu_net.py: the encoder's features against the reference, relative to max|ref|
_ENCODERS = {}


@pytest.fixture(scope="module")
def vectors():
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resnet50_vectors.npz"))
    return {k: torch.from_numpy(z[k]) for k in z.files}


def encoder_of(name, dev):
    """The case's encoder on the device, shared by the tests (they restore every switch they touch)."""
    sd, _ = S.case(name)
    key = S.CASES[name][:2]
    if key not in _ENCODERS:
        _ENCODERS[key] = S.build_encoder(S.layers_of(sd), sd).to(dev)
    return _ENCODERS[key]


def run(enc, x, **switches):
    """The features with the given switches (winograd=..., latency=..., or an attribute of the encoder) for this call only."""
    winograd, latency = switches.pop("winograd", True), switches.pop("latency", False)
    old = {k: getattr(enc, k) for k in switches}
    try:
        for k, v in switches.items():
            setattr(enc, k, v)
        enc.set_winograd(winograd)
        enc.set_latency_mode(latency)
        with torch.no_grad():
            return enc(x)
    finally:
        for k, v in old.items():
            setattr(enc, k, v)
        enc.set_winograd(True)
        enc.set_latency_mode(False)


def truth(name, vectors):
    """(y64, y_cpu32): the reference's recorded features where the fixture has the case, else the scenario's own CPU runs."""
    if name + "_feats64" in vectors:
        return vectors[name + "_feats64"], vectors[name + "_feats32"]
    return S.references(name)[2:]


def check_winograd(tag, y, y64):
    err, scale = maxerr(y, y64), float(y64.abs().max())
    print("%-40s max|dev - f64| = %.3e  max|y64| = %.3e  in 2^-23 max|y64|: %.2f  err/bound = %.4f"
          % (tag, err, scale, err / (S.EPS32 * scale), err / (WINOGRAD_TOL * scale)))
    assert err == err and err <= WINOGRAD_TOL * scale, (tag, err)
    return err / (WINOGRAD_TOL * scale)


@pytest.mark.parametrize("name", ["small_wino", "small_generic", "full", "production"])
def test_encoder_features_against_float64(dev, vectors, name):
    """Direct route and latency mode by the rule of 4, the default (Winograd) route by 1e-4 max|y64|.  small_wino: Winograd stem,
    Winograd 3x3 at 16^2 and 8^2, stride-2 direct, identity and entry blocks; small_generic: the generic stem, every layer direct;
    full: resnet50 on 64 x 64; production: (1, 18, 256, 256), every Winograd shape.
    Measured err / bound (direct, latency, Winograd): small_wino 0.450, 0.450, 0.0028; small_generic 0.596, 0.569, 0.0041;
    full 0.513, 0.415, 0.0039; production 0.533, 0.398, 0.0023."""
    enc, x = encoder_of(name, dev), S.case(name)[1].to(dev)
    y64, y32 = truth(name, vectors)
    assert enc._forward_only and y64.shape == (x.shape[0], 2048)
    direct = run(enc, x, winograd=False)
    r_direct = S.check("%s direct" % name, direct, y64, y32)
    latency = run(enc, x, latency=True)
    r_latency = S.check("%s latency" % name, latency, y64, y32)
    default = run(enc, x)
    r_wino = check_winograd("%s default (Winograd)" % name, default, y64)
    if name == "small_generic":
        assert torch.equal(default, direct)                      # no layer of it takes a Winograd form
    print("%s err/bound: direct %.3f latency %.3f winograd %.4f" % (name, r_direct, r_latency, r_wino))


@pytest.mark.parametrize("name", ["small_wino", "small_generic"])
def test_switches_that_change_no_bit(dev, name):
    """fold_downsample, composite, fused_pool and stem_reads_nchw on against off, in the default mode, on the direct route and in
    latency mode; a second call repeats the bits (frames are reused: nothing stale leaks)."""
    enc, x = encoder_of(name, dev), S.case(name)[1].to(dev)
    for mode in ({}, {"winograd": False}, {"latency": True}):
        base = run(enc, x, **mode)
        assert torch.equal(run(enc, x, **mode), base), mode
        for switch in ("fold_downsample", "composite", "fused_pool", "stem_reads_nchw"):
            other = run(enc, x, **dict(mode, **{switch: False}))
            assert torch.equal(other, base), (mode, switch, maxerr(other, base))
        both = run(enc, x, **dict(mode, fused_pool=False, stem_reads_nchw=False, composite=False, fold_downsample=False))
        assert torch.equal(both, base), mode


@pytest.mark.parametrize("name", ["small_wino", "small_generic"])
def test_an_images_features_do_not_depend_on_the_batch(dev, name):
    enc, x = encoder_of(name, dev), S.case(name)[1].to(dev)
    big = torch.cat([x, x.flip(0), x * 0.5, x])                  # 12 or 8 images: more than one work item of the 8 x 8 Winograd layers
    for mode in ({}, {"winograd": False}, {"latency": True}):
        whole = run(enc, x, **mode)
        assert torch.equal(run(enc, x[:1].contiguous(), **mode), whole[:1]), mode
        assert torch.equal(run(enc, big, **mode)[:x.shape[0]], whole), mode
        assert torch.equal(run(enc, x[1:].contiguous(), **mode), whole[1:]), mode


def test_filled_stem_frames_feed_the_bottleneck_encoder(dev):
    """stem_frames / FilledStemFrames: the frame-fed stem in front of the Bottleneck blocks gives the features of the NCHW input."""
    from hierarchicalprobabilistic3dhuman_amd import _capi
    enc, x = encoder_of("small_wino", dev), S.case("small_wino")[1].to(dev)
    want = run(enc, x)
    B, C, H, W = x.shape
    with torch.no_grad():
        filled = enc.stem_frames(B, C, H, W, dev)
        assert filled is not None
        _capi.call("hps_stem_phase_split", _capi.ptr(x), _capi.ptr(filled.frames), B, C, H, W, _capi.stream())
        got = enc(filled)
    assert torch.equal(got, want)
    assert enc.stem_frames(2, 18, 40, 24, dev) is None


# ---- the head at the widths of the 50-layer net ------------------------------------------------------------------------------
def head_net(dev):
    if "head" not in _ENCODERS:
        c = FS.case("smpl", "default", 3, 10, S.HEAD_WIDTHS)
        torch.manual_seed(0)
        net = PoseMFShapeGaussianNet(configs.SMPL_PARENTS, S.net_config()).eval()
        missing, unexpected = net.load_state_dict(c["sd"], strict=False)
        assert not unexpected and all(k.startswith("image_encoder.") for k in missing)
        _ENCODERS["head"] = net.to(dev)
    return _ENCODERS["head"]


def test_head_at_the_widths_of_the_50_layer_net(dev):
    """tests/head_forward_scenario.py as it stands with widths (2048, 1024, 10, 6, 3, 256, 128) on the smpl tree at B = 3:
    ``net(x, input_feats=...)`` in the product, per-level, host-SVD and latency forms, hps_head_trunk through the C ABI (NaN padding
    columns and guard row), and hps_head_forward_refine by the float64 rule.
    Measured, in units of max(e_family, 2^-23 max|y64|) (bound 4): pose_F 1.58, pose_U 1.03, pose_S 0.79, pose_V 1.04, mode 1.96,
    loc 0.70, scale 0.62, glob 0.38, cam 0.63; trunk x 0.57, sgc 0.65, embed 0.48; refine 1.43 (pose_S) of 8."""
    c = FS.case("smpl", "default", 3, 10, S.HEAD_WIDTHS)
    assert c["feats"].shape == (3, 2048) and 4 * c["kept"] >= c["candidates"]
    net, feats = head_net(dev), c["feats"].to(dev)
    assert net.levels == FS.levels("smpl") and net.fc1.weight.shape == (1024, 2048)
    product = head_forward(net, feats)
    worst = FS.check("widths 2048x1024 product", product, c)
    forms = {"per-level": head_forward(net, feats, composite_head=False), "host SVD": head_forward(net, feats, svd_mode="host"),
             "latency": head_forward(net, feats, latency=True)}
    for name, form in forms.items():
        for k, v in FS.check("widths 2048x1024 %s" % name, form, c).items():
            worst[k] = max(worst[k], v)
    for k in product:
        assert torch.equal(forms["per-level"][k], product[k]) and torch.equal(forms["host SVD"][k], product[k]), k
    trunk = run_trunk(c, kernel_weights(c["sd"], 23, dev), S.HEAD_WIDTHS, dev)
    FS.check("hps_head_trunk 2048x1024", trunk, c, product["pose_U"])
    for k in ("loc", "scale", "glob", "cam"):
        assert torch.equal(trunk[k], product[k]), k
    out_d, out_f = refine(net, feats, product["pose_U"])
    res = FS.check("widths 2048x1024 refine", out_d, c, product["pose_U"], rule64=True, chain=True)
    for k, v in out_f.items():
        assert torch.equal(v, out_d[k].float()), k
    print("head at 2048x1024 worst in max(e_family, 2^-23 max|y64|): %s; refine in 2^-29 units: %.2f"
          % ({k: round(v, 2) for k, v in worst.items()}, max(res.values())))


# ---- the whole net -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net50(dev):
    net = PoseMFShapeGaussianNet(configs.SMPL_PARENTS, S.net_config()).eval()
    net.load_state_dict(S.net_state_dict(PoseMFShapeGaussianNet, configs.SMPL_PARENTS), strict=True)
    return net.to(dev)


def test_net_at_50_reproduces_the_reference(dev, net50, vectors):
    """(2, 18, 64, 64) against the reference net's recorded outputs, with the tolerances of tests/test_gpu_net.py for the 18-layer
    net; the sign-free outputs only (pose_U / pose_V carry LAPACK's free signs)."""
    x = S.case("full")[1].to(dev)
    with torch.no_grad():
        feats = net50.image_encoder(x)
        pose_F, pose_U, pose_S, pose_V, mode, shape_dist, glob, cam = net50(x)
        again = net50(None, input_feats=feats)
    errs = {"features": maxerr(feats, vectors["full_feats32"]) / float(vectors["full_feats32"].abs().max()),
            "pose_S": maxerr(pose_S, vectors["net_S"]) / max(1.0, float(vectors["net_S"].max())), "mode": maxerr(mode, vectors["net_mode"]),
            "loc": maxerr(shape_dist.loc, vectors["net_shape_loc"]), "scale": maxerr(shape_dist.scale, vectors["net_shape_scale"]),
            "glob": maxerr(glob, vectors["net_glob"]), "cam": maxerr(cam, vectors["net_cam"]), "pose_F": maxerr(pose_F, vectors["net_F"])}
    print("net at 50 against the reference:", {k: "%.2e" % v for k, v in errs.items()})
    assert errs["features"] <= 1e-4 and errs["pose_S"] <= 1e-5 and errs["mode"] <= 1e-5
    assert errs["loc"] <= 1e-4 and errs["scale"] <= 1e-4 and errs["glob"] <= 1e-4 and errs["cam"] <= 1e-4
    # pose_F is printed only: the children's inputs carry the parents' singular-vector signs, which LAPACK leaves free
    assert isinstance(shape_dist, torch.distributions.Normal) and pose_U.shape == (2, 23, 3, 3) and pose_V.shape == (2, 23, 3, 3)
    assert torch.equal(again[0], pose_F) and torch.equal(again[4], mode) and torch.equal(again[7], cam)


def test_infer_pipeline_and_graph_at_50(dev, net50, smpl_gpu):
    """infer at B = 2, N = 4: every key, shape and finite values; InferencePipeline returns its bits for the same seed; GraphedInfer
    at B = 1 equals eager infer for the same Philox key, in both encoder modes."""
    x = S.case("full")[1].to(dev)
    B, N = 2, 4
    out = infer(net50, smpl_gpu, x, num_samples=N, seed=11)
    shapes = {"pose_F": (B, 23, 3, 3), "pose_U": (B, 23, 3, 3), "pose_V": (B, 23, 3, 3), "pose_S": (B, 23, 3), "pose_rotmats_mode": (B, 23, 3, 3),
              "shape_loc": (B, 10), "shape_scale": (B, 10), "glob": (B, 6), "cam": (B, 3), "glob_rotmats": (B, 3, 3),
              "verts_mode": (B, 6890, 3), "joints_mode": (B, 90, 3), "verts_tpose": (B, 6890, 3), "R_samples": (B, N, 23, 3, 3),
              "verts_samples": (B, N, 6890, 3), "joints_samples": (B, N, 90, 3), "unc": (B, 6890)}
    for k, shape in shapes.items():
        assert tuple(out[k].shape) == shape and bool(torch.isfinite(out[k]).all()), k
    out = {k: out[k].clone() for k in shapes}
    pipe = InferencePipeline(net50, smpl_gpu, num_samples=N)
    got = pipe.finish(pipe.submit(x), seed=11)
    torch.cuda.synchronize()
    for k in shapes:
        assert torch.equal(got[k], out[k]), ("InferencePipeline", k)
    try:
        for latency in (False, True):
            net50.set_latency_mode(latency)
            g = GraphedInfer(net50, smpl_gpu, batch=1, num_samples=N, slots=2, input_shape=(18, 64, 64))
            for seed, off in ((11, 0), (12, 1), (11, 0)):
                want = infer(net50, smpl_gpu, x[:1], num_samples=N, seed=seed, image_offset=off)
                got = g(x[:1], seed=seed, image_offset=off)
                for k in ("pose_F", "pose_rotmats_mode", "R_samples", "verts_mode", "verts_samples", "joints_samples", "unc", "cam"):
                    assert torch.equal(got[k], want[k]), ("GraphedInfer", latency, seed, k)
    finally:
        net50.set_latency_mode(False)


def test_checkpoint_round_trip_deepcopy_and_to(dev, net50, vectors):
    """A reference-format checkpoint dict round-trips through load_state_dict(strict=True); a deep copy and a trip through the host
    own their weights and give the same bits."""
    x = S.case("full")[1].to(dev)
    with torch.no_grad():
        want = net50(x)
    ckpt = {"best_model_state_dict": {k: v.cpu().clone() for k, v in net50.state_dict().items()}}
    torch.manual_seed(3)
    fresh = PoseMFShapeGaussianNet(configs.SMPL_PARENTS, S.net_config()).eval().to(dev)
    with torch.no_grad():
        before = fresh.image_encoder(x)
    fresh.load_state_dict(ckpt["best_model_state_dict"], strict=True)
    assert fresh._prepared is None and fresh.image_encoder._prepared is None
    clone = copy.deepcopy(net50)
    moved = copy.deepcopy(net50).cpu().to(dev)
    assert clone.image_encoder._prepared is None and moved.image_encoder._prepared is None
    with torch.no_grad():
        for other in (fresh, clone, moved):
            got = other(x)
            for i in (0, 2, 4, 6, 7):
                assert torch.equal(got[i], want[i]), i
            assert torch.equal(got[5].loc, want[5].loc)
        assert not torch.equal(before, net50.image_encoder(x))             # the load changed the encoder's weights
    assert set(ckpt["best_model_state_dict"]) == set(fresh.state_dict())


def test_grad_mode_is_refused_on_the_device(dev, net50):
    x = S.case("full")[1].to(dev)
    with pytest.raises(NotImplementedError, match=r"torch\.no_grad\(\)"):
        net50(x)
    with torch.no_grad():
        assert net50(x)[0].shape == (2, 23, 3, 3)
