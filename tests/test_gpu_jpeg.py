"""The device JPEG decoder (csrc/jpeg.hip) on the GPU: byte equality with the NumPy restatement of tests/jpeg_scenario.py and with PIL,
independence of the batch, untouched guard bytes, a file larger than one workgroup's lanes, a truncated file, and the opt-in routes
of the datasets and the predict loop against their host routes."""
import io
import os

import numpy as np
import pytest
import torch

import jpeg_scenario as S

pytestmark = pytest.mark.gpu

GUARD = 64


@pytest.fixture(scope="module")
def decoder():
    from hierarchicalprobabilistic3dhuman_amd import jpeg
    dec = jpeg.DeviceJpegDecoder()
    dec.GUARD = GUARD
    return dec


@pytest.fixture(scope="module")
def encoded():
    """Every case as an EncodedJpeg, in an order that mixes sizes, samplings and tables within a call."""
    from hierarchicalprobabilistic3dhuman_amd import jpeg
    order = np.random.RandomState(3).permutation(len(S.cases()))
    return [jpeg.EncodedJpeg(S.cases()[i][1], name=S.cases()[i][0]) for i in order]


def _host(dec, results):
    """The results of the last call as numpy arrays: one copy of the output buffer."""
    flat = dec.out.cpu().numpy()
    lay = dec.layout
    return [flat[int(lay["out_off"][j]):int(lay["out_off"][j]) + lay["out_bytes"][j]].reshape(tuple(r.shape)) for j, r in enumerate(results)]


@pytest.mark.parametrize("subseq_bits,mode", [(128, "native"), (0, "rgb")])
def test_every_case_in_mixed_batches(decoder, encoded, subseq_bits, mode):
    turbo = S.turbo()
    for b0 in range(0, len(encoded), 64):
        group = encoded[b0:b0 + 64]
        got = _host(decoder, decoder.decode(group, mode=mode, subseq_bits=subseq_bits))
        assert decoder.statuses() == [0] * len(group)
        for e, g in zip(group, got):
            want = S.restated(e.name)["pixels"]
            want = S.as_rgb(want) if mode == "rgb" else want
            assert g.shape == want.shape and np.array_equal(g, want), (e.name, subseq_bits)
            if turbo:
                assert np.array_equal(g, S.pil_pixels(e.data, rgb=mode == "rgb")), (e.name, "PIL")
    decoder.check()


def test_sync_loop_takes_more_than_one_round_and_several_subsequences(decoder, encoded):
    """The cases exercise the scheme: at 128 bits a 131 x 67 quality-100 file has hundreds of subsequences and needs several rounds."""
    big = [e for e in encoded if e.name.startswith("131x67_444_q100")]
    decoder.decode(big, subseq_bits=128)
    rounds = decoder.sync_rounds()
    assert min(rounds) >= 2 and all(e.header.scan_length * 8 // 128 > 300 for e in big if e.name.endswith("none")), rounds


def test_same_bytes_alone_first_and_last(decoder, encoded):
    pick = [e for e in encoded if e.name in ("37x29_420_q75_opt_none", "131x67_422_q100_std_blocks3", "17x33_grey_q30_std_rows1")]
    assert len(pick) == 3
    others = encoded[:20]
    for e in pick:
        alone = _host(decoder, decoder.decode([e], mode="native"))[0].copy()
        first = _host(decoder, decoder.decode([e] + others, mode="native"))[0].copy()
        last = _host(decoder, decoder.decode(others + [e], mode="native"))[-1].copy()
        assert np.array_equal(alone, S.restated(e.name)["pixels"])
        assert np.array_equal(alone, first) and np.array_equal(alone, last), e.name


def _guards_intact(dec, value):
    lay = dec.layout
    work, out = dec.work.cpu().numpy(), dec.out.cpu().numpy()
    for j in range(len(lay["out_bytes"])):
        a = int(lay["out_off"][j]) + lay["out_bytes"][j]
        assert a + GUARD <= int(lay["out_off"][j + 1]) and (out[a:int(lay["out_off"][j + 1])] == value).all(), ("output", j)
        a = int(lay["ws_off"][j]) + lay["ws_bytes"][j]
        assert a + GUARD <= int(lay["ws_off"][j + 1]) and (work[a:int(lay["ws_off"][j + 1])] == value).all(), ("workspace", j)
    assert (out[int(lay["out_off"][-1]):] == value).all() and (work[int(lay["ws_off"][-1]):] == value).all()


def test_guard_bytes_untouched(decoder, encoded):
    group = encoded[100:164]
    decoder.decode(group, mode="native", subseq_bits=128)                    # sizes the buffers
    decoder.work.fill_(0xA5)
    decoder.out.fill_(0xA5)
    got = _host(decoder, decoder.decode(group, mode="native", subseq_bits=128))
    for e, g in zip(group, got):
        assert np.array_equal(g, S.restated(e.name)["pixels"]), e.name
    _guards_intact(decoder, 0xA5)


def test_photograph_larger_than_a_workgroup(decoder):
    """720 x 960, 4:2:0, no restart markers: thousands of subsequences for the 1024 lanes of its workgroup.  Held to the restatement
    and to the largest subsequence length always, and to PIL where it is built on libjpeg-turbo."""
    from hierarchicalprobabilistic3dhuman_amd import jpeg
    data = S.encode(S.picture(720, 960, False, 99), quality=75, sampling="420")
    e = jpeg.EncodedJpeg(data, name="photo.jpg")
    assert e.header.scan_length * 8 // 512 > 1024
    got = decoder.decode([e])[0].cpu().numpy()
    assert decoder.statuses() == [0]
    info = S.walk(data)
    assert np.array_equal(got, S.pixels(info, S.coefficients(info)))
    assert np.array_equal(decoder.decode([e], subseq_bits=4096)[0].cpu().numpy(), got)
    assert np.array_equal(decoder.decode([e], subseq_bits=128)[0].cpu().numpy(), got)
    if S.turbo():
        assert np.array_equal(got, S.pil_pixels(data, rgb=True))


def test_truncated_file_is_reported_and_contained(decoder, encoded):
    from hierarchicalprobabilistic3dhuman_amd import _capi, jpeg
    a, b = [e for e in encoded if e.name in ("64x48_420_q75_std_none", "131x67_444_q100_opt_rows1")]
    victim = [e for e in encoded if e.name == "131x67_420_q100_std_none"][0]
    h = victim.header
    cut = jpeg.EncodedJpeg(victim.data[:h.scan_offset + h.scan_length // 2], name="cut.jpg")
    group = [a, cut, b]
    decoder.decode(group, mode="native", subseq_bits=128)
    decoder.work.fill_(0x5A)
    decoder.out.fill_(0x5A)
    got = _host(decoder, decoder.decode(group, mode="native", subseq_bits=128))
    status = decoder.statuses()
    assert status[0] == 0 and status[2] == 0 and status[1] != 0, status
    _guards_intact(decoder, 0x5A)
    assert np.array_equal(got[0], S.restated(a.name)["pixels"]) and np.array_equal(got[2], S.restated(b.name)["pixels"])
    with pytest.raises(_capi.HpsError, match="cut.jpg"):
        decoder.check()


def test_rejected_arguments(decoder, encoded):
    from hierarchicalprobabilistic3dhuman_amd import _capi, jpeg
    colour = [e for e in encoded if e.name == "16x16_444_q75_std_none"]
    with pytest.raises(_capi.HpsError, match="subseq_bits"):
        decoder.decode(colour, subseq_bits=100)
    with pytest.raises(_capi.HpsError, match="subseq_bits"):
        decoder.decode(colour, subseq_bits=8192)
    with pytest.raises(jpeg.JpegUnsupported):
        decoder.decode(colour, mode="grey")
    with pytest.raises(ValueError):
        decoder.decode(colour, mode="bgr")


# ---------------------------------------------------------------------------------------------------------------------------------
# the opt-in routes: decode="device" of the datasets, image_decoder="device" of the predict loop
# ---------------------------------------------------------------------------------------------------------------------------------
def _jpeg_files(directory, names_sizes, seed):
    """Generated JPEG files of mixed sampling, quality and restart placement; the second is progressive (the host fallback)."""
    os.makedirs(directory, exist_ok=True)
    kinds = [dict(sampling="420", quality=75), dict(sampling="444", quality=90, progressive=True), dict(sampling="422", quality=60, restart="rows1"),
             dict(sampling="420", quality=95, optimize=True), dict(sampling="grey", quality=80)]
    for i, (name, (h, w)) in enumerate(names_sizes):
        kind = dict(kinds[i % len(kinds)])
        grey = kind.pop("sampling") == "grey"
        data = S.encode(S.picture(w, h, grey, seed + i), sampling=kinds[i % len(kinds)]["sampling"] if not grey else "420", **kind)
        with open(os.path.join(directory, name), "wb") as f:
            f.write(data)


def _same_batches(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        if torch.is_tensor(a[k]):
            assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


def test_train_dataset_device_decode_equals_host_decode(tmp_path):
    import data_layer_scenario as DS
    from hierarchicalprobabilistic3dhuman_amd import jpeg
    from hierarchicalprobabilistic3dhuman_amd.on_the_fly_smpl_train_dataset import OnTheFlySMPLTrainDataset
    files = DS.write_train_files(str(tmp_path / "train"))
    bg = files["backgrounds_dir_path"]
    for f in os.listdir(bg):
        if f.endswith(".jpg"):
            os.remove(os.path.join(bg, f))
    _jpeg_files(bg, [("bg_%d.jpg" % i, hw) for i, hw in enumerate([(24, 30), (16, 16), (33, 20), (8, 40), (19, 19)])], 40)
    with pytest.raises(ValueError):
        OnTheFlySMPLTrainDataset(decode="gpu", **files)
    sets = {d: OnTheFlySMPLTrainDataset(grey_tex_prob=0.4, img_wh=16, decode=d, **files) for d in ("host", "device")}
    items = {}
    for d, ds in sets.items():
        torch.manual_seed(5)
        items[d] = [ds[i % len(ds)] for i in range(12)]
    kinds = {type(it["background"]).__name__ for it in items["device"]}
    assert kinds == {"EncodedJpeg", "Tensor"}, kinds                           # the progressive file came back decoded by PIL
    assert all(torch.is_tensor(it["background"]) for it in items["host"])
    for b0 in (0, 6):
        _same_batches(sets["host"].prepare_batch(items["host"][b0:b0 + 6]), sets["device"].prepare_batch(items["device"][b0:b0 + 6]))
    sets["device"]._images.check()


def test_datasets_report_a_truncated_file_by_name(tmp_path):
    import data_layer_scenario as DS
    from torch.utils.data import Subset
    from hierarchicalprobabilistic3dhuman_amd import _capi, data_layer
    from hierarchicalprobabilistic3dhuman_amd.on_the_fly_smpl_train_dataset import OnTheFlySMPLTrainDataset
    files = DS.write_train_files(str(tmp_path / "train"))
    bg = files["backgrounds_dir_path"]
    for f in os.listdir(bg):
        if f.endswith(".jpg"):
            os.remove(os.path.join(bg, f))
    data = S.case_bytes("64x48_420_q75_std_none")
    with open(os.path.join(bg, "whole.jpg"), "wb") as f:
        f.write(data)
    with open(os.path.join(bg, "cut.jpg"), "wb") as f:
        f.write(data[:len(data) * 2 // 3])
    ds = OnTheFlySMPLTrainDataset(grey_tex_prob=0.4, img_wh=16, decode="device", **files)
    data_layer.check_decoded(Subset(ds, [0]))                                # nothing prepared yet: nothing to report
    torch.manual_seed(1)
    items = [ds[i % len(ds)] for i in range(8)]
    assert {os.path.basename(it["background"].name) for it in items} == {"whole.jpg", "cut.jpg"}
    ds.prepare_batch(items)
    with pytest.raises(_capi.HpsError, match="cut.jpg"):
        data_layer.check_decoded(Subset(ds, [0]))
    data_layer.check_decoded(ds)                                             # reported once


def test_pw3d_dataset_device_decode_equals_host_decode(tmp_path):
    import data_layer_scenario as DS
    from hierarchicalprobabilistic3dhuman_amd.pw3d_eval_dataset import PW3DEvalDataset
    root = DS.write_pw3d_files(str(tmp_path / "pw3d"), n=5, sides=(40, 64, 33, 57, 48))
    frames = os.path.join(root, "cropped_frames")
    meta = dict(np.load(os.path.join(root, "3dpw_test.npz")))
    names = ["crop_%02d.jpg" % i for i in range(4)] + ["crop_04.png"]          # four JPEGs (one progressive) and a PNG
    _jpeg_files(frames, list(zip(names[:4], [(40, 40), (64, 64), (33, 33), (57, 57)])), 60)
    meta["imgname"] = np.array(names)
    np.savez(os.path.join(root, "3dpw_test.npz"), **meta)
    cfg = type("C", (), {"DATA": type("D", (), {"PROXY_REP_SIZE": 16, "HEATMAP_GAUSSIAN_STD": 4.0})})
    sets = {d: PW3DEvalDataset(root, cfg, visible_joints_threshold=0.5, decode=d) for d in ("host", "device")}
    items = {d: [ds[i] for i in range(5)] for d, ds in sets.items()}
    assert [type(it["image"]).__name__ for it in items["device"]] == ["EncodedJpeg", "Tensor", "EncodedJpeg", "EncodedJpeg", "Tensor"]
    for sl in (slice(0, 3), slice(3, 5), slice(0, 5)):
        _same_batches(sets["host"].prepare_batch(items["host"][sl]), sets["device"].prepare_batch(items["device"][sl]))
    sets["device"]._images.check()
    with pytest.raises(ValueError):
        PW3DEvalDataset(root, cfg, decode=None)


def test_ssp3d_dataset_device_decode_equals_host_decode(tmp_path):
    import data_layer_scenario as DS
    from hierarchicalprobabilistic3dhuman_amd.ssp3d_eval_dataset import SSP3DEvalDataset
    sizes = ((60, 44), (48, 48), (41, 67), (52, 70), (64, 40))
    root = DS.write_ssp3d_files(str(tmp_path / "ssp3d"), n=5, sizes=sizes)
    # the images become JPEG files under their own names (both decoders go by content); the last stays a PNG, the second is progressive
    _jpeg_files(os.path.join(root, "images"), [("frame_%02d.png" % i, sizes[i]) for i in range(4)], 70)
    cfg = type("C", (), {"DATA": type("D", (), {"PROXY_REP_SIZE": 32, "HEATMAP_GAUSSIAN_STD": 4.0, "BBOX_SCALE_FACTOR": 1.2})})
    sets = {d: SSP3DEvalDataset(root, cfg, visible_joints_threshold=0.5, decode=d) for d in ("host", "device")}
    items = {d: [ds[i] for i in range(5)] for d, ds in sets.items()}
    assert [type(it["image"]).__name__ for it in items["device"]] == ["EncodedJpeg", "Tensor", "EncodedJpeg", "EncodedJpeg", "Tensor"]
    for sl in (slice(0, 3), slice(2, 5)):
        _same_batches(sets["host"].prepare_batch(items["host"][sl]), sets["device"].prepare_batch(items["device"][sl]))
    sets["device"]._images.check()


def test_predict_with_the_device_decoder_delivers_the_same_tensors(tmp_path, dev, net_gpu, smpl_gpu, monkeypatch):
    import hrnet_scenario as HS
    from hierarchicalprobabilistic3dhuman_amd import _capi, configs, predict_poseMF_shapeGaussian_net as P
    from hierarchicalprobabilistic3dhuman_amd.canny_edge_detector import CannyEdgeDetector
    from hierarchicalprobabilistic3dhuman_amd.pose2D_hrnet import PoseHighResolutionNet
    from PIL import Image
    image_dir = str(tmp_path / "images")
    sizes = [("a.jpg", (60, 60)), ("b.jpg", (48, 72)), ("c.jpg", (101, 67)), ("d.jpg", (64, 64)), ("e.jpeg", (80, 56))]
    _jpeg_files(image_dir, sizes, 80)
    Image.fromarray(S.picture(52, 44, False, 7)).save(os.path.join(image_dir, "f.png"))
    # the baseline reads with PIL explicitly (load_rgb_image prefers OpenCV where it is installed, whose libjpeg may round differently)
    monkeypatch.setattr(P, "load_rgb_image", lambda path: np.asarray(Image.open(path).convert("RGB")))
    hcfg = HS.config("SMALL")
    hcfg["MODEL"]["IMAGE_SIZE"], hcfg["MODEL"]["HEATMAP_SIZE"] = [64, 96], [16, 24]
    hrnet = PoseHighResolutionNet(HS.config("SMALL")).eval()
    hrnet.load_state_dict(HS.seeded_state_dict(HS.shapes_of(hrnet.state_dict()), 0), strict=True)
    hrnet = hrnet.to(dev)
    cfg = configs.get_cfg_defaults()
    edge = CannyEdgeDetector(non_max_suppression=cfg.DATA.EDGE_NMS, gaussian_filter_std=cfg.DATA.EDGE_GAUSSIAN_STD,
                             gaussian_filter_size=cfg.DATA.EDGE_GAUSSIAN_SIZE, threshold=cfg.DATA.EDGE_THRESHOLD).to(dev)
    got = {}
    for decoder in ("pil", "device"):
        out = got[decoder] = {}
        torch.manual_seed(11)
        P.predict_poseMF_shapeGaussian_net(net_gpu, cfg, smpl_gpu, hrnet, hcfg, edge, dev, image_dir, str(tmp_path / ("out_" + decoder)),
                                           num_samples=8, batch_size=4, batched_front_end=True, image_decoder=decoder,
                                           result_fn=lambda n, item, out=out: out.__setitem__(n, {k: v.clone() for k, v in item.items() if torch.is_tensor(v)}))
    assert sorted(got["pil"]) == sorted(got["device"]) == sorted([n for n, _ in sizes] + ["f.png"])
    for n in got["pil"]:
        assert sorted(got["pil"][n]) == sorted(got["device"][n])
        for k, v in got["pil"][n].items():
            assert torch.equal(v, got["device"][n][k]), (n, k)
    with pytest.raises(_capi.HpsError, match="per-image route"):
        P.predict_poseMF_shapeGaussian_net(net_gpu, cfg, smpl_gpu, hrnet, hcfg, edge, dev, image_dir, str(tmp_path / "out_x"),
                                           batched_front_end=False, image_decoder="device")
    with pytest.raises(ValueError):
        P.predict_poseMF_shapeGaussian_net(net_gpu, cfg, smpl_gpu, hrnet, hcfg, edge, dev, image_dir, str(tmp_path / "out_y"), image_decoder="cv2")
