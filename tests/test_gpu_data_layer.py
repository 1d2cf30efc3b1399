"""GPU: the data-layer kernels (csrc/data_layer.hip) and the three datasets' prepare_batch.

  * hps_texture_gather equals bank[idx] / 255 exactly (1200 x 800 and the 5 x 7 tail path; a repeated index, both ends of both banks);
  * hps_resize_bilinear_u8 and hps_eval_crop_u8 give the levels of tests/data_layer_scenario.py's integer restatements of cv2.resize
    and cv2.warpAffine bit for bit -- both sides are integer arithmetic, no tolerance -- and the joints of float64 NumPy exactly;
  * integer positions: truncation toward zero (SSP-3D) on negative fractions, round half to even (3DPW) on .5 ties;
  * heat maps within 4 max(e_ref32, 2^-23 max|y|) of the float64 formula, e_ref32 the error of the reference's own float32 NumPy;
  * each dataset through a DataLoader (0 and 2 workers): keys, dtypes, shapes, device, agreement with the kernels called piece by
    piece, and a first batch that the second does not overwrite;
  * the evaluation and the training loop fed such a dataset compute what they compute from the same batches as plain tensors.

Agreement with OpenCV itself is not checked here (tests/test_data_layer_host.py has the optional comparison)."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, Dataset, Subset

import data_layer_scenario as S
from hierarchicalprobabilistic3dhuman_amd import configs, data_layer as DL
from hierarchicalprobabilistic3dhuman_amd.on_the_fly_smpl_train_dataset import OnTheFlySMPLTrainDataset
from hierarchicalprobabilistic3dhuman_amd.pw3d_eval_dataset import PW3DEvalDataset
from hierarchicalprobabilistic3dhuman_amd.ssp3d_eval_dataset import SSP3DEvalDataset

pytestmark = pytest.mark.gpu
F255 = np.float32(255)


def cfg_of(wh):
    return NS(DATA=NS(PROXY_REP_SIZE=wh, HEATMAP_GAUSSIAN_STD=4.0, BBOX_SCALE_FACTOR=1.2))


def as_float(levels_hwc):
    """uint8 (..., H, W, 3) levels -> the float32 (..., 3, H, W) the kernels write: level / 255, a true float32 division."""
    a = np.asarray(levels_hwc).astype(np.float32) / F255
    return np.moveaxis(a, -1, -3)


# ---------------------------------------------------------------------------------------------------------------------------------
# the kernels
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Ht,Wt", [(1200, 800), (5, 7)])
def test_texture_gather_is_exact(dev, Ht, Wt):
    rs = np.random.RandomState(Ht)
    grey, nongrey = rs.randint(0, 256, (2, Ht, Wt, 3)).astype(np.uint8), rs.randint(0, 256, (3, Ht, Wt, 3)).astype(np.uint8)
    grey[0, 0, 0], nongrey[2, -1, -1] = (0, 255, 1), (254, 0, 255)
    choices = [(True, 0), (False, 2), (True, 1), (False, 0), (False, 2)]
    out = DL.texture_gather(torch.from_numpy(grey).to(dev), torch.from_numpy(nongrey).to(dev), choices)
    assert out.dtype == torch.float32 and tuple(out.shape) == (5, Ht, Wt, 3)
    want = np.stack([(grey if g else nongrey)[i] for g, i in choices]).astype(np.float32) / F255
    assert np.array_equal(out.cpu().numpy(), want)
    # one bank only, and an index outside its bank is refused on the host
    only = DL.texture_gather(None, torch.from_numpy(nongrey).to(dev), [(False, 1)])
    assert np.array_equal(only.cpu().numpy()[0], nongrey[1].astype(np.float32) / F255)
    with pytest.raises(Exception, match="outside its bank"):
        DL.texture_gather(torch.from_numpy(grey).to(dev), torch.from_numpy(nongrey).to(dev), [(True, 2)])


@pytest.mark.parametrize("T", S.RESIZE_TARGETS)
def test_resize_levels_equal_the_integer_restatement(dev, T):
    sources = [S.noise_image(H * 1000 + W, H, W) for H, W in S.RESIZE_SOURCES]
    out = DL.resize_bilinear_u8([torch.from_numpy(s).to(dev) for s in sources], (T, T)).cpu().numpy()
    assert out.shape == (len(sources), 3, T, T)
    for b, s in enumerate(sources):
        assert np.array_equal(out[b], as_float(S.resize_levels(s, T, T))), S.RESIZE_SOURCES[b]
    # non-square output, and an image alone gives the bits it gives in a batch
    alone = DL.resize_bilinear_u8([torch.from_numpy(sources[4]).to(dev)], (T, 9)).cpu().numpy()
    assert np.array_equal(alone[0], as_float(S.resize_levels(sources[4], T, 9)))


@pytest.mark.parametrize("wh", [16, 67])
@pytest.mark.parametrize("H,W", S.CROP_IMAGES)
def test_crop_equals_the_restatement_and_float64_numpy(dev, H, W, wh):
    rgb, seg = S.noise_image(H * 1000 + W, H, W), S.noise_image(H * 1000 + W + 1, H, W, channels=0)
    boxes = S.crop_boxes(H, W)
    names = list(boxes)
    kps = np.stack([S.crop_keypoints(i, H, W) for i in range(len(names))])
    d_rgb, d_seg = torch.from_numpy(rgb).to(dev), torch.from_numpy(seg).to(dev)
    out = DL.eval_crop_u8([d_rgb] * len(names), [(boxes[n][0][0], boxes[n][0][1], boxes[n][1]) for n in names], 1.2, wh,
                          segs=[d_seg] * len(names), keypoints=torch.from_numpy(kps).to(dev))
    got = {k: v.cpu().numpy() for k, v in out.items()}
    assert got["joints"].dtype == np.float64 and got["positions"].dtype == np.int32 and got["seg"].dtype == np.float32
    negative_fractions = 0
    for b, n in enumerate(names):
        M = S.crop_matrix(boxes[n][0], boxes[n][1], 1.2, wh)
        assert np.array_equal(got["rgb"][b], as_float(S.crop_levels(rgb, M, wh))), n
        assert np.array_equal(got["seg"][b], S.crop_nearest(seg, M, wh).astype(np.float32)), n
        joints = S.crop_joints(M, kps[b][:, :2])
        assert np.array_equal(got["joints"][b], joints), n
        assert np.array_equal(got["positions"][b], joints.astype(np.int16).astype(np.int32)), n
        negative_fractions += int(((joints < 0) & (joints != np.floor(joints))).sum())
    assert negative_fractions > 0                          # truncation toward zero differs from floor on these
    # without silhouettes and key points only the image is written
    bare = DL.eval_crop_u8([d_rgb], [(boxes["inside"][0][0], boxes["inside"][0][1], boxes["inside"][1])], 1.2, wh)
    assert bare["seg"] is None and bare["joints"] is None and np.array_equal(bare["rgb"].cpu().numpy()[0], got["rgb"][names.index("inside")])


def test_positions_truncate_toward_zero_and_round_half_to_even(dev):
    probes = S.POSITION_PROBES
    kp = np.zeros((2, len(probes), 3))
    kp[0, :, :2], kp[1, :, :2] = probes, probes * 4.0
    scale = np.array([[1.0, 1.0], [0.25, 0.25]])
    joints, positions = DL.keypoints_scale_round(torch.from_numpy(kp).to(dev), torch.from_numpy(scale).to(dev))
    want = kp[:, :, :2] * scale[:, None, :]
    assert np.array_equal(joints.cpu().numpy(), want)
    assert np.array_equal(positions.cpu().numpy(), want.round().astype(np.int16).astype(np.int32))
    assert positions.cpu().numpy()[0].tolist()[:5] == [[-1, 1], [-1, -2], [-2, 2], [0, 2], [4, 0]]          # ties go to the even side
    # SSP-3D's route on the same values: a box that maps the image onto itself (16 / 1.25 * 1.25 = 16 exactly), truncation
    img = torch.zeros(16, 16, 3, dtype=torch.uint8, device=dev)
    out = DL.eval_crop_u8([img], [(8.0, 8.0, 12.8)], 1.25, 16, keypoints=torch.from_numpy(kp[:1]).to(dev))
    M = S.crop_matrix((8.0, 8.0), 12.8, 1.25, 16)
    assert np.array_equal(M, np.float32([[1, 0, 0], [0, 1, 0]]))
    assert np.array_equal(out["joints"].cpu().numpy()[0], probes)
    assert out["positions"].cpu().numpy()[0].tolist()[:5] == [[0, 0], [-1, -1], [-2, 2], [0, 1], [3, 0]]


@pytest.mark.parametrize("wh", [16, 19, 256])
def test_heatmaps_against_float64(dev, wh):
    rs = np.random.RandomState(wh)
    positions = rs.randint(-6, wh + 6, (2, S.K, 2)).astype(np.int32)
    positions[0, :3] = [[0, 0], [wh - 1, wh - 1], [-40, wh + 40]]
    kp = np.stack([S.crop_keypoints(3, wh, wh), S.crop_keypoints(4, wh, wh)])
    d_pos, d_kp = torch.from_numpy(positions).to(dev), torch.from_numpy(kp).to(dev)
    worst = 0.0
    for threshold in (None, 0.5):
        got = DL.eval_heatmaps(d_pos, wh, 4.0, keypoints=d_kp, threshold=threshold).cpu().numpy().astype(np.float64)
        for b in range(2):
            y64 = S.heatmaps(positions[b], wh, 4.0, np.float64, kp[b][:, 2], threshold)
            ref32 = S.heatmaps(positions[b], wh, 4.0, np.float32, kp[b][:, 2], threshold)
            assert ref32.dtype == np.float32
            e_ref32 = np.abs(ref32.astype(np.float64) - y64).max()
            bound = 4.0 * max(e_ref32, 2.0 ** -23 * np.abs(y64).max())
            err = np.abs(got[b] - y64).max()
            worst = max(worst, err / bound)
            print("heatmaps wh %d threshold %s image %d: err %.3e e_ref32 %.3e bound %.3e ratio %.3f" % (wh, threshold, b, err, e_ref32, bound, err / bound))
            assert err <= bound
            if threshold is not None:                      # 0.5 is not > 0.5 (joint 7), 0.49 neither (8); joint 0 is always visible
                assert not got[b][7].any() and not got[b][8].any() and got[b][9].any() == ref32[9].any() and got[b][0].any() == ref32[0].any()
    print("heatmaps wh %d worst ratio %.3f" % (wh, worst))


# ---------------------------------------------------------------------------------------------------------------------------------
# the datasets through a DataLoader
# ---------------------------------------------------------------------------------------------------------------------------------
def batches_of(ds, num_workers, batch_size=3):
    torch.manual_seed(11)
    loader = DataLoader(ds, batch_size=batch_size, shuffle=False, num_workers=num_workers, pin_memory=False, collate_fn=DL.passthrough_collate)
    return list(loader)


def run_two_batches(ds, item_batches, dev):
    """prepare_batch on the first two batches; the first batch's tensors must survive the second."""
    first = ds.prepare_batch(item_batches[0])
    kept = {k: v.clone() for k, v in first.items() if torch.is_tensor(v)}
    second = ds.prepare_batch(item_batches[1])
    torch.cuda.synchronize()
    for k, v in kept.items():
        assert v.device.type == "cuda" and torch.equal(first[k], v), k
    return first, second


@pytest.fixture(scope="module")
def train_files(tmp_path_factory):
    return S.write_train_files(str(tmp_path_factory.mktemp("train")))


@pytest.mark.parametrize("num_workers", [0, 2])
def test_train_dataset_batches(dev, train_files, num_workers):
    wh = 16
    ds = OnTheFlySMPLTrainDataset(grey_tex_prob=0.4, img_wh=wh, **train_files)
    item_batches = batches_of(ds, num_workers)
    assert [len(b) for b in item_batches] == [3, 3, 1] and all(not it["background"].is_cuda for b in item_batches for it in b)
    banks = np.load(train_files["textures_path"])
    poses = np.load(train_files["poses_path"])["poses"]
    for items, batch in zip(item_batches[:2], run_two_batches(ds, item_batches, dev)):
        assert sorted(batch) == ["background", "pose", "texture"]
        assert all(v.dtype == torch.float32 and v.device == dev for v in batch.values())
        assert tuple(batch["pose"].shape) == (3, 72) and tuple(batch["texture"].shape) == (3, 1200, 800, 3)
        assert tuple(batch["background"].shape) == (3, 3, wh, wh)
        for i, it in enumerate(items):
            g, idx = it["texture_choice"]
            assert np.array_equal(batch["texture"][i].cpu().numpy(), banks["grey" if g else "nongrey"][idx].astype(np.float32) / F255)
            assert np.array_equal(batch["background"][i].cpu().numpy(), as_float(S.resize_levels(it["background"].numpy(), wh, wh)))
            alone = DL.resize_bilinear_u8([it["background"].to(dev)], (wh, wh))
            assert torch.equal(alone[0], batch["background"][i])
        assert np.array_equal(batch["pose"].cpu().numpy(), np.stack([it["pose"].numpy() for it in items]))
    assert np.array_equal(np.stack([it["pose"].numpy() for it in item_batches[0]]), poses[:3])


@pytest.mark.parametrize("num_workers", [0, 2])
def test_ssp3d_dataset_batches(dev, tmp_path, num_workers):
    wh = 32
    ds = SSP3DEvalDataset(S.write_ssp3d_files(str(tmp_path / "ssp3d"), n=5), cfg_of(wh), visible_joints_threshold=0.5)
    item_batches = batches_of(ds, num_workers)
    assert [len(b) for b in item_batches] == [3, 2]
    for items, batch in zip(item_batches, run_two_batches(ds, item_batches, dev)):
        B = len(items)
        assert sorted(batch) == ["fname", "gender", "heatmaps", "image", "keypoints", "pose", "shape", "silhouette"]
        want = {"image": (B, 3, wh, wh), "heatmaps": (B, 17, wh, wh), "pose": (B, 72), "shape": (B, 10), "silhouette": (B, wh, wh)}
        for k, shape in want.items():
            assert batch[k].dtype == torch.float32 and batch[k].device == dev and tuple(batch[k].shape) == shape, k
        assert batch["keypoints"].dtype == torch.float64 and tuple(batch["keypoints"].shape) == (B, 17, 2)
        assert batch["fname"] == [it["fname"] for it in items] and batch["gender"] == [it["gender"] for it in items]
        for i, it in enumerate(items):
            M = S.crop_matrix(it["bbox_centre"].numpy(), it["bbox_wh"], 1.2, wh)
            kp = it["keypoints"].numpy()
            joints = S.crop_joints(M, kp[:, :2])
            assert np.array_equal(batch["image"][i].cpu().numpy(), as_float(S.crop_levels(it["image"].numpy(), M, wh)))
            assert np.array_equal(batch["silhouette"][i].cpu().numpy(), S.crop_nearest(it["silhouette"].numpy(), M, wh).astype(np.float32))
            assert np.array_equal(batch["keypoints"][i].cpu().numpy(), joints)
            positions = torch.from_numpy(joints.astype(np.int16).astype(np.int32))[None].to(dev)
            piece = DL.eval_heatmaps(positions, wh, 4.0, keypoints=it["keypoints"][None].to(dev), threshold=0.5)
            assert torch.equal(piece[0], batch["heatmaps"][i])
            assert np.array_equal(batch["pose"][i].cpu().numpy(), it["pose"].numpy()) and np.array_equal(batch["shape"][i].cpu().numpy(), it["shape"].numpy())


@pytest.mark.parametrize("num_workers", [0, 2])
def test_pw3d_dataset_batches(dev, tmp_path, num_workers):
    wh = 16
    ds = PW3DEvalDataset(S.write_pw3d_files(str(tmp_path / "pw3d"), n=4), cfg_of(wh), visible_joints_threshold=None)
    item_batches = batches_of(ds, num_workers)
    assert [len(b) for b in item_batches] == [3, 1]
    for items, batch in zip(item_batches, run_two_batches(ds, item_batches, dev)):
        B = len(items)
        assert sorted(batch) == ["fname", "gender", "heatmaps", "image", "pose", "shape"]
        for k, shape in {"image": (B, 3, wh, wh), "heatmaps": (B, 17, wh, wh), "pose": (B, 72), "shape": (B, 10)}.items():
            assert batch[k].dtype == torch.float32 and batch[k].device == dev and tuple(batch[k].shape) == shape, k
        assert batch["gender"] == [it["gender"] for it in items]
        for i, it in enumerate(items):
            side = it["image"].shape[0]
            assert np.array_equal(batch["image"][i].cpu().numpy(), as_float(S.resize_levels(it["image"].numpy(), wh, wh)))
            kp = it["keypoints"].numpy()
            scaled = kp[:, :2] * np.array([wh / float(side), wh / float(side)])                      # pw3d_eval_dataset.py:51-53
            positions = torch.from_numpy(scaled.round().astype(np.int16).astype(np.int32))[None].to(dev)
            assert torch.equal(DL.eval_heatmaps(positions, wh, 4.0)[0], batch["heatmaps"][i])


def test_steady_state_reuses_the_staging_buffers_and_never_waits_for_the_host(dev, train_files, tmp_path):
    """After two warm-up batches (both host slots exist, the banks are resident) a prepare_batch makes no synchronising torch call,
    allocates no staging memory and returns the bits of the first call."""
    datasets = (OnTheFlySMPLTrainDataset(grey_tex_prob=0.4, img_wh=16, **train_files),
                SSP3DEvalDataset(S.write_ssp3d_files(str(tmp_path / "ssp3d"), n=3), cfg_of(32), visible_joints_threshold=0.5),
                PW3DEvalDataset(S.write_pw3d_files(str(tmp_path / "pw3d"), n=3), cfg_of(16), visible_joints_threshold=0.5))
    one = torch.ones((), device=dev)
    for ds in datasets:
        torch.manual_seed(3)
        items = [ds[i] for i in range(3)]
        first = ds.prepare_batch(items)
        ds.prepare_batch(items)
        torch.cuda.synchronize()
        staging = ds._staging
        pointers = (staging.dev.data_ptr(), staging.host[0].data_ptr(), staging.host[1].data_ptr())
        prev = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        try:
            with pytest.raises(RuntimeError):              # the mode is live on this build: a synchronising call is refused
                torch.nonzero(one)
            third = ds.prepare_batch(items)
            fourth = ds.prepare_batch(items)
        finally:
            torch.cuda.set_sync_debug_mode(prev)
        torch.cuda.synchronize()
        assert pointers == (staging.dev.data_ptr(), staging.host[0].data_ptr(), staging.host[1].data_ptr())
        for k, v in first.items():
            if torch.is_tensor(v):
                assert torch.equal(v, third[k]) and torch.equal(v, fourth[k]) and v.data_ptr() != third[k].data_ptr(), k


# ---------------------------------------------------------------------------------------------------------------------------------
# the loops
# ---------------------------------------------------------------------------------------------------------------------------------
class _PlainFrames(Dataset):
    """The reference's item format, from batches already prepared: what any other dataset hands the evaluation loop."""

    def __init__(self, batches):
        self.items = []
        for b in batches:
            for i in range(len(b["fname"])):
                self.items.append({k: (v[i].cpu().clone() if torch.is_tensor(v) else v[i]) for k, v in b.items()})

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


def test_evaluation_from_an_ssp3d_directory_equals_plain_tensors(dev, tmp_path, net_gpu, smpl_gpu):
    from hierarchicalprobabilistic3dhuman_amd import smpl_data, textured_renderer as tr
    from hierarchicalprobabilistic3dhuman_amd.canny_edge_detector import CannyEdgeDetector
    from hierarchicalprobabilistic3dhuman_amd.evaluate_poseMF_shapeGaussian_net import evaluate_pose_MF_shapeGaussian_net
    from hierarchicalprobabilistic3dhuman_amd.smpl_official import SMPL
    from test_gpu_silhouette import _densepose
    cfg = configs.get_cfg_defaults()
    wh = cfg.DATA.PROXY_REP_SIZE
    gendered = {k: SMPL(smpl_data.synthetic_smpl_model(s), gender=g).to(dev) for k, s, g in (("m", 1, "male"), ("f", 2, "female"))}
    det = CannyEdgeDetector(cfg.DATA.EDGE_NMS, cfg.DATA.EDGE_GAUSSIAN_STD, cfg.DATA.EDGE_GAUSSIAN_SIZE, cfg.DATA.EDGE_THRESHOLD).to(dev)
    renderer = tr.TexturedIUVRenderer(dev, 1, img_wh=wh, projection_type="orthographic", render_rgb=False, bin_size=32,
                                      densepose_uv=_densepose(smpl_gpu.num_verts))
    metrics = ["PVE-PA", "PVE-T-SC", "silhouette-IOU", "joints2D-L2E"]
    ds = SSP3DEvalDataset(S.write_ssp3d_files(str(tmp_path / "ssp3d"), n=5), cfg, visible_joints_threshold=0.5)

    def run(dataset):
        return evaluate_pose_MF_shapeGaussian_net(net_gpu, cfg, smpl_gpu, gendered["m"], gendered["f"], det, dev, dataset, metrics, None,
                                                  num_workers=0, pin_memory=False, save_per_frame_metrics=False, num_samples_for_metrics=0,
                                                  batch_size=3, seed=77, silhouette_renderer=renderer)
    got = run(ds)
    plain = _PlainFrames([ds.prepare_batch([ds[i] for i in idx]) for idx in ((0, 1, 2), (3, 4))])
    assert DL.preparer(plain) is None
    want = run(plain)
    through_subset = run(Subset(ds, list(range(5))))
    for m in metrics:
        print("%s %.9g" % (m, got[m]))
        assert np.isfinite(got[m]) and got[m] == want[m] and through_subset[m] == want[m], (m, got[m], want[m])


def test_a_training_step_from_the_dataset_equals_the_step_on_plain_tensors(dev, smpl_gpu, train_files, tmp_path, monkeypatch, capsys):
    import test_gpu_train_loop as TL
    from hierarchicalprobabilistic3dhuman_amd import train_poseMF_shapeGaussian_net as tp
    from hierarchicalprobabilistic3dhuman_amd.train_loss_and_metrics_tracker import TrainingLossesAndMetricsTracker
    cfg = TL.make_cfg()
    cfg.TRAIN.NUM_EPOCHS = 1
    ds = OnTheFlySMPLTrainDataset(params_from="not_amass", grey_tex_prob=0.4, img_wh=TL.W, **train_files)
    assert len(ds) == 4
    seen = []
    real = tp.SyntheticTrainStep.__call__

    def call(self, samples_batch, split):
        state = TL.rng_state()
        loss = real(self, samples_batch, split)
        seen.append((split, {k: v.clone() for k, v in samples_batch.items()}, state, loss.clone()))
        return loss
    w = TL.make_world(dev, smpl_gpu, cfg, metrics=list(TL.METRICS))
    TL.seed_all(9)
    with monkeypatch.context() as m:
        m.setattr(tp.SyntheticTrainStep, "__call__", call)
        tp.train_poseMF_shapeGaussian_net(w["net"], cfg, smpl_gpu, w["edge"], w["renderer"], dev, ds, Subset(ds, [0, 1]), w["criterion"], w["opt"],
                                          w["metrics"], str(tmp_path), str(tmp_path / "log.pkl"))
    assert [s[0] for s in seen] == ["train", "train", "val"]
    split, batch, state, loss = seen[0]
    assert sorted(batch) == ["background", "pose", "texture"] and all(v.device == dev and v.dtype == torch.float32 for v in batch.values())
    assert tuple(batch["texture"].shape) == (2, 1200, 800, 3) and tuple(batch["background"].shape) == (2, 3, TL.W, TL.W)
    # the same step on the same tensors handed over directly, in a fresh world
    w2 = TL.make_world(dev, smpl_gpu, cfg, metrics=list(TL.METRICS))
    net = w2["net"]
    net.set_batchnorm_training(True)
    net.set_differentiable_factors(True)
    tracker = TrainingLossesAndMetricsTracker(w2["metrics"], TL.W, None)
    tracker.initialise_loss_metric_sums()
    step = tp.SyntheticTrainStep(net, cfg, smpl_gpu, w2["edge"], w2["renderer"], dev, w2["criterion"], w2["opt"], tracker)
    net.train()
    TL.restore_rng(state)
    direct = step({k: v.cpu() for k, v in batch.items()}, "train")
    print("loss %.9g direct %.9g" % (float(loss), float(direct)))
    assert bool(torch.isfinite(loss)) and torch.equal(loss, direct)
    capsys.readouterr()
