"""CPU: the restatement of the predict front end (tests/predict_frontend_scenario.py) against the reference's recorded outputs
(tests/golden/predict_frontend_vectors.npz), its pixel-space resample against F.grid_sample in float64, the host-side argument
validation of hps_predict_boxes / hps_crop_bilinear / hps_hrnet_keypoints, and the predict loop's ``batched_front_end`` rule."""
import ctypes
import os

import numpy as np
import pytest
import torch

import predict_frontend_scenario as S
from hierarchicalprobabilistic3dhuman_amd import _capi

HERE = os.path.dirname(os.path.abspath(__file__))
SELECTED = {"one_60x45": 0, "wide_45x60": 0, "three_60x80": 1, "tie_60x80": 0}       # every other case: the whole image (-1)


@pytest.fixture(scope="module")
def fixture():
    z = np.load(os.path.join(HERE, "golden", "predict_frontend_vectors.npz"))
    return {k: z[k] for k in z.files}


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.int32)


def _record(case):
    return S.box_record(case.H, case.W, S.case_det(case), S.GOLDEN_IMAGE_SIZE, S.GOLDEN_THRESHOLD, S.GOLDEN_SCALE_FACTOR)


@pytest.mark.parametrize("name", list(S.GOLDEN_CASES))
def test_scenario_against_the_reference_fixture(fixture, name):
    case = S.GOLDEN_CASES[name]
    fx = lambda k: fixture["%s_%s" % (name, k)]
    assert np.array_equal(S.case_image(case), fx("image"))
    rec = _record(case)
    # the box predict_hrnet returns: bit for bit, and the selection
    assert np.array_equal(_bits(rec[0:2]), _bits(fx("bbox_centre")))
    assert np.array_equal(_bits(rec[2]), _bits(fx("bbox_height"))) and np.array_equal(_bits(rec[3]), _bits(fx("bbox_width")))
    assert int(rec[10]) == SELECTED.get(name, -1)
    assert float(rec[11]) == float(torch.max(rec[2], rec[3]) * S.GOLDEN_SCALE_FACTOR)
    # the first crop: the pixel-space float32 form against the reference's float32 output and against float64
    y64, y32 = (S.crop_theta(fx("image"), S.GOLDEN_IMAGE_SIZE, rec, dt) for dt in (torch.float64, torch.float32))
    b = S.bound(y64, y32)[0]
    p32 = S.crop_pixels(fx("image"), S.GOLDEN_IMAGE_SIZE, rec, torch.float32)
    ref = torch.from_numpy(fx("cropped_image"))
    assert float((y32 - ref).abs().max()) <= b                                  # the restated theta route IS the reference's
    worst = S.check("%s crop, pixel-space fp32" % name, p32, y64, y32)
    d = float((p32 - ref).abs().max())
    print("%s: max|pixel32 - reference32| = %.3e = %.3f bounds" % (name, d, d / b))
    assert d <= b
    # key points: integers, exact
    factor = S.GOLDEN_IMAGE_SIZE[0] / S.GOLDEN_HEATMAP_SIZE[0]
    rec2 = S.box_record(S.GOLDEN_IMAGE_SIZE[1], S.GOLDEN_IMAGE_SIZE[0], None, (S.GOLDEN_PROXY,) * 2, 0.0, 1.0, hrnet_fix=False)
    assert rec2[2] == rec2[3] == S.GOLDEN_IMAGE_SIZE[1] and rec2[0] == S.GOLDEN_IMAGE_SIZE[1] / 2 and rec2[1] == S.GOLDEN_IMAGE_SIZE[0] / 2
    idx, joints, confs, crop_j, visib = S.keypoints(fx("heatmaps"), factor, rec2[None], S.GOLDEN_VIS_THRESHOLD)
    assert np.array_equal(_bits(joints[0]), _bits(fx("joints2D"))) and np.array_equal(_bits(confs[0]), _bits(fx("joints2Dconfs")))
    assert float((crop_j[0].double() - torch.from_numpy(fx("proxy_joints2D")).double()).abs().max()) <= 4 * S.EPS32 * S.GOLDEN_PROXY
    # the second crop, from the reference's own first crop
    D = (S.GOLDEN_PROXY, S.GOLDEN_PROXY)
    z64, z32 = (S.crop_theta(ref, D, rec2, dt) for dt in (torch.float64, torch.float32))
    b2 = S.bound(z64, z32)[0]
    q32 = S.crop_pixels(ref, D, rec2, torch.float32)
    worst = max(worst, S.check("%s proxy crop, pixel-space fp32" % name, q32, z64, z32))
    assert float((q32 - torch.from_numpy(fx("proxy_rgb"))).abs().max()) <= b2
    print("worst err/bound  %s  %.3f" % (name, worst))


def test_arg_max_edge_cases_of_the_scenario():
    hm = S.special_heatmaps(17, 5, 7, 0)
    idx, joints, confs, _, visib = S.keypoints(hm, 4.0, None, 0.75)
    n = 35
    assert idx[0, 0] == 0 and idx[0, 1] == n - 1 and idx[0, 2] == n // 3                         # first, last, the first of two equals
    assert confs[0, 3] < 0 and joints[0, 3].tolist() == [0.0, 0.0] and confs[0, 4] == 0 and joints[0, 4].tolist() == [0.0, 0.0]
    assert visib[0, 5] == 1 and visib[0, 6] == 1                                                   # forced by the mask (joints 0-6)
    _, _, _, _, free = S.keypoints(hm, 4.0, None, 0.75, always_visible=0)
    assert confs[0, 5] == 0.75 and free[0, 5] == 0 and free[0, 6] == 1 and free[0, 3] == 0         # AT the threshold is not above it


PROBE = [  # H, W, out (w, h), box centre (v, h), height, width: boxes partly outside; the sizes of the float64 probe
    (1, 1, (8, 8), (0.5, 0.5), 1.0, 1.0),
    (37, 53, (24, 32), (10.0, 40.0), 30.0, 11.0),
    (150, 200, (32, 64), (70.0, 20.0), 160.0, 90.0),
    (1080, 1920, (288, 384), (600.3, 1000.7), 850.2, 310.9),
    (3000, 4000, (288, 384), (1500.0, 2100.0), 3300.0, 900.0),
]


@pytest.mark.parametrize("H,W,out_wh,centre,h,w", PROBE)
def test_pixel_space_formula_against_grid_sample_in_float64(H, W, out_wh, centre, h, w):
    det = (torch.tensor([[centre[1] - w / 2, centre[0] - h / 2, centre[1] + w / 2, centre[0] + h / 2]]), torch.tensor([1]), torch.tensor([0.99]))
    rec = S.box_record(H, W, det, out_wh, 0.8, 1.2)
    img = torch.from_numpy(np.random.RandomState(H).randint(0, 256, (H, W, 3)).astype(np.uint8))
    y64, y32 = (S.crop_theta(img, out_wh, rec, dt) for dt in (torch.float64, torch.float32))
    p64 = S.crop_pixels(img, out_wh, rec, torch.float64)
    d = float((p64 - y64).abs().max())
    print("%dx%d: max|pixel64 - grid_sample64| = %.3e" % (H, W, d))
    assert d <= 1e-9                                                  # two float64 routes to the same sample: ~2^-52 x (position ~ 4000)
    ratio = S.check("%dx%d pixel-space fp32" % (H, W), S.crop_pixels(img, out_wh, rec, torch.float32), y64, y32)
    print("worst err/bound  pixel-space fp32 %dx%d  %.3f" % (H, W, ratio))


# ---------------------------------------------------------------------------------------------------------------------------------
# argument validation: on the host, before any launch (no GPU here)
# ---------------------------------------------------------------------------------------------------------------------------------
def _rejects(entry, args, text):
    lib = _capi.load()
    assert getattr(lib, entry)(ctypes.byref(args), None) == -1, entry
    assert text in lib.hps_last_error(), (entry, lib.hps_last_error())


def test_struct_mirrors_have_the_library_layout():
    lib = _capi.load()
    assert lib.hps_sizeof_predict_boxes_args() == ctypes.sizeof(_capi.PredictBoxesArgs)
    assert lib.hps_sizeof_crop_bilinear_args() == ctypes.sizeof(_capi.CropBilinearArgs)
    assert lib.hps_sizeof_hrnet_keypoints_args() == ctypes.sizeof(_capi.HrnetKeypointsArgs)
    assert lib.hps_version() == 502


def test_predict_boxes_validates_on_the_host():
    lib = _capi.load()
    A = _capi.PredictBoxesArgs
    good = lambda **kw: A(**dict(dict(struct_bytes=ctypes.sizeof(A), B=1, out_w=32, out_h=64, threshold=0.8, scale_factor=1.2, records=64), **kw))
    assert lib.hps_predict_boxes(None, None) == -1 and b"null pointer" in lib.hps_last_error()
    _rejects("hps_predict_boxes", good(struct_bytes=8), b"struct_bytes")
    assert lib.hps_predict_boxes(ctypes.byref(good(B=0)), None) == 0                  # nothing to do
    _rejects("hps_predict_boxes", good(B=_capi.FRONTEND_MAX_IMAGES + 1), b"images per launch")
    _rejects("hps_predict_boxes", good(B=-1), b"images per launch")
    _rejects("hps_predict_boxes", good(records=None), b"null pointer")
    _rejects("hps_predict_boxes", good(records=66), b"aligned")
    _rejects("hps_predict_boxes", good(out_w=0), b"output size")
    _rejects("hps_predict_boxes", good(scale_factor=0.0), b"scale_factor")
    a = good()                                                                      # image 0 has H = W = 0
    _rejects("hps_predict_boxes", a, b"image size")
    a = good()
    a.image[0].H, a.image[0].W, a.image[0].n = 4, 4, -1
    _rejects("hps_predict_boxes", a, b"negative")
    a.image[0].n, a.image[0].boxes = 2, 64
    _rejects("hps_predict_boxes", a, b"labels / scores")
    a.image[0].labels, a.image[0].scores = 68, 64
    _rejects("hps_predict_boxes", a, b"aligned")


def test_crop_bilinear_validates_on_the_host():
    lib = _capi.load()
    A = _capi.CropBilinearArgs
    good = lambda **kw: A(**dict(dict(struct_bytes=ctypes.sizeof(A), B=1, out_w=32, out_h=64, records=64, raw=128), **kw))

    def with_image(a, src=256, H=4, W=4, kind=_capi.FRONTEND_SRC_HWC_U8):
        a.image[0].src, a.image[0].H, a.image[0].W, a.image[0].kind = src, H, W, kind
        return a
    assert lib.hps_crop_bilinear(None, None) == -1 and b"null pointer" in lib.hps_last_error()
    _rejects("hps_crop_bilinear", good(struct_bytes=0), b"struct_bytes")
    assert lib.hps_crop_bilinear(ctypes.byref(good(B=0)), None) == 0
    _rejects("hps_crop_bilinear", good(B=65), b"images per launch")
    _rejects("hps_crop_bilinear", good(raw=None), b"null pointer")
    _rejects("hps_crop_bilinear", good(records=None), b"null pointer")
    _rejects("hps_crop_bilinear", good(raw=130), b"aligned")
    _rejects("hps_crop_bilinear", good(out_h=0), b"output size")
    _rejects("hps_crop_bilinear", good(out_w=40000), b"output size")
    _rejects("hps_crop_bilinear", with_image(good(normalised=512)), b"mean / std")             # std = 0
    _rejects("hps_crop_bilinear", good(), b"image source")
    _rejects("hps_crop_bilinear", with_image(good(), H=0), b"image size")
    _rejects("hps_crop_bilinear", with_image(good(), kind=7), b"source kind")
    _rejects("hps_crop_bilinear", with_image(good(), src=257, kind=_capi.FRONTEND_SRC_CHW_F32), b"float source")


def test_hrnet_keypoints_validates_on_the_host():
    lib = _capi.load()
    A = _capi.HrnetKeypointsArgs
    good = lambda **kw: A(**dict(dict(struct_bytes=ctypes.sizeof(A), B=1, K=17, h=16, w=8, factor=4.0, vis_threshold=0.75, heatmaps=64,
                                      records=128, joints_hrnet=192, confs=256, joints_crop=320, visib=384), **kw))
    assert lib.hps_hrnet_keypoints(None, None) == -1 and b"null pointer" in lib.hps_last_error()
    _rejects("hps_hrnet_keypoints", good(struct_bytes=4), b"struct_bytes")
    assert lib.hps_hrnet_keypoints(ctypes.byref(good(B=0)), None) == 0
    _rejects("hps_hrnet_keypoints", good(B=-2), b"B out of range")
    _rejects("hps_hrnet_keypoints", good(K=0), b"1 to 32 joints")
    _rejects("hps_hrnet_keypoints", good(K=33), b"1 to 32 joints")
    _rejects("hps_hrnet_keypoints", good(h=0), b"heat maps")
    _rejects("hps_hrnet_keypoints", good(h=4096, w=4096), b"heat maps")
    for name in ("heatmaps", "joints_hrnet", "confs", "visib"):
        _rejects("hps_hrnet_keypoints", good(**{name: None}), b"null pointer")
    _rejects("hps_hrnet_keypoints", good(records=None), b"go together")
    _rejects("hps_hrnet_keypoints", good(joints_crop=None), b"go together")
    _rejects("hps_hrnet_keypoints", good(confs=258), b"aligned")
    _rejects("hps_hrnet_keypoints", good(factor=float("inf")), b"not finite")


# ---------------------------------------------------------------------------------------------------------------------------------
# the predict loop's rule
# ---------------------------------------------------------------------------------------------------------------------------------
class _Edge:
    def edge_map_into(self, *a, **k):
        raise AssertionError("not called")


def _device_hrnet():
    import hrnet_scenario as H
    from hierarchicalprobabilistic3dhuman_amd.pose2D_hrnet import PoseHighResolutionNet
    return PoseHighResolutionNet(H.config("NARROW"))


def test_batched_front_end_selection_rule():
    from hierarchicalprobabilistic3dhuman_amd.predict_poseMF_shapeGaussian_net import use_batched_front_end as rule
    hr, plain, edge, cuda = _device_hrnet(), torch.nn.Conv2d(3, 17, 1), _Edge(), torch.device("cuda:0")
    assert rule(None, None, cuda, hr, edge) and rule(True, None, cuda, hr, edge) and rule(None, None, "cuda", hr, edge)
    assert not rule(False, None, cuda, hr, edge)
    assert not rule(None, lambda p: None, cuda, hr, edge)
    assert not rule(None, None, torch.device("cpu"), hr, edge)
    assert not rule(None, None, cuda, plain, edge) and not rule(False, None, cuda, plain, edge)
    assert not rule(None, None, cuda, hr, object())
    for args, text in (((lambda p: None, cuda, hr, edge), "proxy_rep_fn"), ((None, "cpu", hr, edge), "not a GPU"),
                       ((None, cuda, plain, edge), "PoseHighResolutionNet"), ((None, cuda, hr, object()), "edge_map_into")):
        with pytest.raises(_capi.HpsError, match=text):
            rule(True, *args)


def test_a_plain_module_hrnet_keeps_the_per_image_route(tmp_path, monkeypatch):
    """With ``batched_front_end=None`` an injected nn.Module key-point detector gets today's per-image front end (an empty image
    directory: the loop itself needs a device)."""
    from hierarchicalprobabilistic3dhuman_amd import configs, predict_frontend, predict_poseMF_shapeGaussian_net as P
    made = []
    monkeypatch.setattr(P, "_reference_front_end", lambda *a: made.append(a) or (lambda path: None))

    def no_batched(*a, **k):
        raise AssertionError("the batched front end was built")
    monkeypatch.setattr(predict_frontend, "DevicePredictFrontEnd", no_batched)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)                 # no device here; nothing is launched
    os.makedirs(str(tmp_path / "images"))
    net = torch.nn.Identity()
    hrnet_cfg = configs.get_pose2D_hrnet_cfg_defaults()
    for flag in (None, False):
        P.predict_poseMF_shapeGaussian_net(net, configs.get_cfg_defaults(), None, torch.nn.Conv2d(3, 17, 1), hrnet_cfg, _Edge(), "cuda:0",
                                           str(tmp_path / "images"), str(tmp_path / "out"), batched_front_end=flag)
    assert len(made) == 2
    with pytest.raises(_capi.HpsError, match="PoseHighResolutionNet"):
        P.predict_poseMF_shapeGaussian_net(net, configs.get_cfg_defaults(), None, torch.nn.Conv2d(3, 17, 1), hrnet_cfg, _Edge(), "cuda:0",
                                           str(tmp_path / "images"), str(tmp_path / "out"), batched_front_end=True)
