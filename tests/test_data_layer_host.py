"""The data layer without a GPU: the NumPy restatements of cv2.resize / cv2.warpAffine (tests/data_layer_scenario.py) against a float64
ideal bilinear, the datasets' host side (draw order against the reference's own class, params_from, __len__, the square-frame
assertion) and the refusal to prepare a batch without a device.  Agreement with OpenCV ITSELF is checked only where
tests/golden/make_data_layer_golden.py ran with OpenCV installed (the cv2_* arrays); otherwise that test skips."""
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import data_layer_scenario as S
from hierarchicalprobabilistic3dhuman_amd import _capi, data_layer
from hierarchicalprobabilistic3dhuman_amd.on_the_fly_smpl_train_dataset import OnTheFlySMPLTrainDataset
from hierarchicalprobabilistic3dhuman_amd.pw3d_eval_dataset import PW3DEvalDataset
from hierarchicalprobabilistic3dhuman_amd.ssp3d_eval_dataset import SSP3DEvalDataset

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data_layer_vectors.npz")
CFG = NS(DATA=NS(PROXY_REP_SIZE=16, HEATMAP_GAUSSIAN_STD=4.0, BBOX_SCALE_FACTOR=1.2))


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def train_files(tmp_path_factory):
    return S.write_train_files(str(tmp_path_factory.mktemp("train")), marker_textures=True)


# ---------------------------------------------------------------------------------------------------------------------------------
# restatements against the float64 ideal
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", S.RESIZE_TARGETS)
@pytest.mark.parametrize("H,W", S.RESIZE_SOURCES)
def test_resize_restatement_is_within_one_level_of_the_ideal(H, W, T):
    src = S.smooth_image(H * 1000 + W, H, W)
    err = np.abs(S.resize_levels(src, T, T).astype(np.float64) - S.ideal_resize(src, T, T)).max()
    print("resize %dx%d -> %d: max |level - ideal| = %.4f" % (H, W, T, err))
    assert err <= 1.0


@pytest.mark.parametrize("wh", [16, 64])
@pytest.mark.parametrize("H,W", S.CROP_IMAGES)
def test_warp_restatement_is_within_one_level_of_the_ideal(H, W, wh):
    src = S.smooth_image(H * 1000 + W + 7, H, W)
    for name, (centre, side) in S.crop_boxes(H, W).items():
        M = S.crop_matrix(centre, side, 1.2, wh)
        ideal, mask = S.ideal_crop(src, M, wh)
        err = np.abs(S.crop_levels(src, M, wh).astype(np.float64) - ideal)[mask]
        print("warp %dx%d %s -> %d: %d samples, max |level - ideal| = %.4f" % (H, W, name, wh, err.size // 3, err.max() if err.size else 0.0))
        assert err.size == 0 or err.max() <= 1.0


@pytest.mark.parametrize("H,W", [(1, 1), (7, 5), (37, 53)])
def test_resize_to_the_same_size_is_the_identity(H, W):
    src = S.noise_image(5, H, W)
    assert np.array_equal(S.resize_levels(src, W, H), src)


@pytest.mark.parametrize("shift", [(0, 0), (3, -2), (-5, 4)])
def test_warp_by_an_integer_translation_is_a_shifted_copy(shift):
    H, W, wh = 20, 20, 20
    src, seg = S.noise_image(9, H, W), S.noise_image(10, H, W, channels=0)
    dy, dx = shift
    M = np.float32([[1, 0, dx], [0, 1, dy]])
    want = np.zeros_like(src)
    want_seg = np.zeros_like(seg)
    ys, xs = np.arange(H) - dy, np.arange(W) - dx
    oky, okx = (ys >= 0) & (ys < H), (xs >= 0) & (xs < W)
    want[np.ix_(oky, okx)] = src[np.ix_(ys[oky], xs[okx])]
    want_seg[np.ix_(oky, okx)] = seg[np.ix_(ys[oky], xs[okx])]
    assert np.array_equal(S.crop_levels(src, M, wh), want)
    assert np.array_equal(S.crop_nearest(seg, M, wh), want_seg)


def test_half_size_resize_equals_the_area_average():
    """At exactly 2x OpenCV's INTER_LINEAR takes the INTER_AREA route, (a + b + c + d + 2) >> 2: the bilinear formula gives the same."""
    src = S.noise_image(3, 32, 32).astype(np.int64)
    area = (src[0::2, 0::2] + src[0::2, 1::2] + src[1::2, 0::2] + src[1::2, 1::2] + 2) >> 2
    assert np.array_equal(S.resize_levels(src, 16, 16), area)


def test_restatements_against_opencv_itself(golden):
    if not any(k.startswith("cv2_") for k in golden):
        pytest.skip("OpenCV outputs absent: run tests/golden/make_data_layer_golden.py where OpenCV is installed")
    for H, W in S.RESIZE_SOURCES:
        for T in S.RESIZE_TARGETS:
            assert np.array_equal(S.resize_levels(S.noise_image(H * 1000 + W, H, W), T, T), golden["cv2_resize_%dx%d_to%d" % (H, W, T)])
    for H, W in S.CROP_IMAGES:
        rgb, seg = S.noise_image(H * 1000 + W, H, W), S.noise_image(H * 1000 + W + 1, H, W, channels=0)
        for name, (centre, side) in S.crop_boxes(H, W).items():
            M = S.crop_matrix(centre, side, 1.2, 16)
            assert np.array_equal(S.crop_levels(rgb, M, 16), golden["cv2_crop_%dx%d_%s" % (H, W, name)])
            assert np.array_equal(S.crop_nearest(seg, M, 16), golden["cv2_seg_%dx%d_%s" % (H, W, name)])


def test_float_of_a_level_over_255_is_the_float64_route_for_all_levels():
    k = np.arange(256)
    assert np.array_equal((k / 255.).astype(np.float32), k.astype(np.float32) / np.float32(255))


# ---------------------------------------------------------------------------------------------------------------------------------
# the datasets' host side
# ---------------------------------------------------------------------------------------------------------------------------------
def test_draw_order_is_the_references(golden, train_files, monkeypatch):
    monkeypatch.setattr(data_layer, "decode_rgb", lambda path: torch.full((1, 1, 3), int(os.path.basename(path)[3:-4]), dtype=torch.uint8))
    assert golden["bank_sizes"].tolist() == [S.DRAW_N_GREY, S.DRAW_N_NONGREY, S.DRAW_N_BACKGROUNDS]
    ds = OnTheFlySMPLTrainDataset(grey_tex_prob=float(golden["grey_tex_prob"]), img_wh=4, **train_files)
    for seed in S.DRAW_SEEDS:
        for B in S.DRAW_BATCHES:
            torch.manual_seed(seed)
            items = [ds[i % len(ds)] for i in range(B)]
            got = [[int(it["texture_choice"][0]), it["texture_choice"][1], int(it["background"][0, 0, 0])] for it in items]
            assert got == golden["draws_seed%d_B%d" % (seed, B)].tolist(), (seed, B)


def test_train_item_holds_raw_data_only(train_files):
    ds = OnTheFlySMPLTrainDataset(**train_files)
    torch.manual_seed(0)
    item = ds[2]
    assert sorted(item) == ["background", "pose", "texture_choice"]
    assert item["pose"].dtype == torch.float32 and tuple(item["pose"].shape) == (72,)
    assert item["background"].dtype == torch.uint8 and item["background"].dim() == 3 and item["background"].shape[2] == 3
    assert not item["background"].is_cuda and isinstance(item["texture_choice"][1], int)
    assert np.array_equal(item["pose"].numpy(), np.load(train_files["poses_path"])["poses"][2])


@pytest.mark.parametrize("params_from,want", [("all", list(range(7))), ("h36m", [0, 5]), ("up3d", [2]), ("3dpw", [3]), ("amass", [1, 4, 6]),
                                              ("not_amass", [0, 2, 3, 5])])
def test_params_from_filters_as_the_reference(train_files, params_from, want):
    ds = OnTheFlySMPLTrainDataset(params_from=params_from, **train_files)
    poses = np.load(train_files["poses_path"])["poses"]
    assert len(ds) == len(want)
    assert np.array_equal(ds.poses, poses[want])
    assert len(ds.backgrounds_paths) == S.DRAW_N_BACKGROUNDS and all(p.endswith(".jpg") for p in ds.backgrounds_paths)
    with pytest.raises(AssertionError):
        OnTheFlySMPLTrainDataset(params_from="elsewhere", **train_files)


def test_evaluation_datasets_items_and_lengths(tmp_path):
    ssp = SSP3DEvalDataset(S.write_ssp3d_files(str(tmp_path / "ssp3d"), n=3), CFG, visible_joints_threshold=0.5)
    assert len(ssp) == 3
    item = ssp[1]
    labels = np.load(str(tmp_path / "ssp3d" / "labels.npz"))
    assert item["image"].dtype == torch.uint8 and tuple(item["image"].shape) == (48, 48, 3)
    assert item["silhouette"].dtype == torch.uint8 and tuple(item["silhouette"].shape) == (48, 48)
    assert np.array_equal(item["image"].numpy(), S.noise_image(1, 48, 48))                         # PNG: exact
    assert np.array_equal(item["keypoints"].numpy(), labels["joints2D"][1]) and item["keypoints"].dtype == torch.float64
    assert item["fname"] == "frame_01.png" and item["gender"] == "f" and item["pose"].dtype == torch.float32
    assert item["bbox_wh"] == float(labels["bbox_whs"][1])
    pw = PW3DEvalDataset(S.write_pw3d_files(str(tmp_path / "pw3d"), n=3), CFG)
    assert len(pw) == 3
    item = pw[2]
    assert tuple(item["image"].shape) == (33, 33, 3) and item["gender"] == "f" and tuple(item["shape"].shape) == (10,)


def test_a_non_square_frame_trips_the_references_assertion(tmp_path):
    pw = PW3DEvalDataset(S.write_pw3d_files(str(tmp_path / "pw3d"), n=2, non_square=1), CFG)
    pw[0]
    with pytest.raises(AssertionError, match="non-square"):
        pw[1]


def test_preparer_looks_through_subsets(train_files):
    from torch.utils.data import Subset, TensorDataset
    ds = OnTheFlySMPLTrainDataset(**train_files)
    assert data_layer.preparer(ds) == ds.prepare_batch
    assert data_layer.preparer(Subset(Subset(ds, [0, 1]), [0])) == ds.prepare_batch
    assert data_layer.preparer(TensorDataset(torch.zeros(2, 1))) is None
    assert data_layer.passthrough_collate([1, 2]) == [1, 2]


def test_prepare_batch_without_a_device_is_refused(train_files, tmp_path, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    ds = OnTheFlySMPLTrainDataset(**train_files)
    torch.manual_seed(0)
    with pytest.raises(_capi.HpsError, match="no CPU fallback"):
        ds.prepare_batch([ds[0], ds[1]])
    ssp = SSP3DEvalDataset(S.write_ssp3d_files(str(tmp_path / "ssp3d"), n=2), CFG)
    with pytest.raises(_capi.HpsError, match="no CPU fallback"):
        ssp.prepare_batch([ssp[0]])
    pw = PW3DEvalDataset(S.write_pw3d_files(str(tmp_path / "pw3d"), n=2), CFG)
    with pytest.raises(_capi.HpsError, match="no CPU fallback"):
        pw.prepare_batch([pw[0]])
