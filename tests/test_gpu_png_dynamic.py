"""hps_png_encode with strategy = 1 on the device (csrc/png.hip: one dynamic Huffman block per segment, all five filters) against
tests/png_dynamic_scenario.py.  The yardstick is exact: every file must be the stream include/hps.h documents, which
png_dynamic_scenario.reference_encode_dynamic restates on the host byte for byte, and must read back to the input through the scenario's
reader and through PIL.  Pictures are tiny and go HPS_PNG_MAX_IMAGES to a call."""
import ctypes
import io
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import png_dynamic_scenario as D
import png_scenario as S
from hierarchicalprobabilistic3dhuman_amd import _capi, configs, textured_renderer as tr, visualise

pytestmark = pytest.mark.gpu


def _launch(pictures, strategies):
    """One hps_png_encode call over ``pictures`` (numpy uint8) with a strategy each -> (return code, what to read the files from)."""
    assert 1 <= len(pictures) <= _capi.PNG_MAX_IMAGES and len(strategies) == len(pictures)
    a = _capi.PngEncodeArgs()
    a.struct_bytes, a.num_images = ctypes.sizeof(_capi.PngEncodeArgs), len(pictures)
    keep = []
    for i, (img, strategy) in enumerate(zip(pictures, strategies)):
        H, W = img.shape[:2]
        C = 3 if img.ndim == 3 else 1
        bound = visualise.png_bound(H, W, C)
        px = torch.from_numpy(np.ascontiguousarray(img)).cuda()
        out = torch.full((bound + 64,), 0xA5, dtype=torch.uint8, device="cuda")          # 64 guard bytes behind the capacity
        ws = torch.empty(max(16, _capi.query_workspace(_capi.WS_PNG, H, W, C)), dtype=torch.uint8, device="cuda")
        length = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        keep.append((px, out, ws, length, bound))
        im = a.image[i]
        im.pixels, im.H, im.W, im.C, im.strategy = _capi.ptr(px, torch.uint8), H, W, C, strategy
        im.out, im.capacity = _capi.ptr(out, torch.uint8), bound
        im.length, im.workspace = _capi.ptr(length, torch.int64), _capi.ptr(ws, torch.uint8)
    rc = _capi.load(dev=_capi._use_dev).hps_png_encode(ctypes.byref(a), _capi.stream())
    return rc, keep


def _encode(pictures, strategies=None):
    rc, keep = _launch(pictures, strategies or [1] * len(pictures))
    assert rc == 0, _capi.load(dev=_capi._use_dev).hps_last_error()
    torch.cuda.synchronize()
    files = []
    for px, out, ws, length, bound in keep:
        n = int(length.item())
        assert 0 < n <= bound, (n, bound)
        host = out.cpu().numpy()
        assert (host[bound:] == 0xA5).all(), "bytes written behind the capacity"
        files.append(host[:n].tobytes())
    return files


def _check(name, img, data):
    from PIL import Image
    img = D._picture(img)
    got = S.read_png(data)
    assert got.shape == img.shape and np.array_equal(got, img), name
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(data))), img), name
    assert len(data) <= visualise.png_bound(img.shape[0], img.shape[1], 3 if img.ndim == 3 else 1), name
    assert data == D.reference_encode_dynamic(img), "%s: not the documented strategy-1 stream" % name


def _check_cases(cases):
    files = []
    for i in range(0, len(cases), _capi.PNG_MAX_IMAGES):
        files += _encode([img for _, img in cases[i:i + _capi.PNG_MAX_IMAGES]])
    for (name, img), data in zip(cases, files):
        _check(name, img, data)
    return files


def test_run_lengths_around_the_match_limits(dev):
    _check_cases(S.run_length_cases())


def test_symbols_boundaries_and_the_end_bit_family(dev):
    R, boundary = S.boundary_cases()
    family = [("end_bits_%d" % i, img) for i, img in enumerate(S.end_bit_family())]
    files = _check_cases(S.symbol_cases() + boundary + family)
    kinds = {"dynamic" if D.dynamic_block_info(p) else "other" for data in files for p in S.idat_payloads(data)[1:-1]}
    assert kinds == {"dynamic", "other"}                             # both the dynamic block and the strategy-0 forms were taken


def test_the_new_pictures_filters_and_both_length_limits(dev):
    files = dict(zip([n for n, _ in D.new_pictures()], _check_cases(D.new_pictures())))
    import zlib
    raw = zlib.decompress(b"".join(S.idat_payloads(files["five_filters"])))
    img = D.five_filters()
    assert {raw[y * (img.shape[1] + 1)] for y in range(img.shape[0])} == {0, 1, 2, 3, 4}
    assert max(D.segment_infos(files["fibonacci_literals"])[0]["ll"]) == 15
    assert max(D.segment_infos(files["code_length_limit"])[0]["cl"]) == 7
    assert all(i is not None for i in D.segment_infos(files["photo_like"]))


def test_widest_rows_and_the_one_pixel_picture(dev):
    """One row per segment: the row above and Paeth's upper-left byte come from the staged row of the segment before."""
    cases = dict(S.mixed_cases())
    assert visualise.png_segment_rows(2, 4096, 3) == 1 and visualise.png_segment_rows(2, 12288, 1) == 1
    # a slope up along the row and down from row to row: the upper-left byte is the pixel itself, so Paeth is taken on one-row segments
    # of the widest RGB row; and the widest grey row that follows the mean of left and above, so Average is
    y, x = np.mgrid[0:3, 0:4096]
    slope = np.stack([20 * x - 20 * y + 7 * c for c in range(3)], axis=-1) + np.random.RandomState(12).randint(-1, 2, (3, 4096, 3))
    slope = (slope & 255).astype(np.uint8)
    average = D.five_filters(W=12288)[3:5]
    assert D.filtered_rows5(slope)[1:, 0].tolist() == [4, 4] and D.filtered_rows5(average)[1, 0] == 3
    picked = [(n, cases[n]) for n in ("widest_rgb", "widest_grey", "one_pixel", "narrow_grey", "figure")]
    files = _check_cases(picked + [("widest_slope", slope), ("widest_average", average)])
    assert len(files) == 7


def test_alternating_strategies_in_one_call(dev):
    pictures = [S.figure_like(), S.ramp(9, 301, 1, True), D.photo_like()[:40], S.constant(3, 300, 1), D.five_filters(), S.noise(5, 9, 3, 1),
                D.fibonacci_literals(), S.two_valued(3, 87, 3, 87)]
    strategies = [i % 2 for i in range(8)]
    files = _encode(pictures, strategies)
    for img, strategy, data in zip(pictures, strategies, files):
        if strategy == 0:
            assert data == S.reference_encode(img)
        else:
            alone, = _encode([img])
            assert data == alone == D.reference_encode_dynamic(img)
    flipped = _encode(pictures, [1 - s for s in strategies])
    for img, strategy, data in zip(pictures, strategies, flipped):
        assert data == (D.reference_encode_dynamic(img) if strategy == 0 else S.reference_encode(img))


def test_a_second_identical_call_gives_identical_bytes(dev):
    pictures = [D.photo_like(), S.figure_like(), D.code_length_limit(), S.noise(7, 21, 3, 4)]
    assert _encode(pictures) == _encode(pictures)


def test_strategy_2_is_refused_before_any_launch(dev):
    img = S.figure_like()
    rc, keep = _launch([img, img], [1, 2])
    assert rc == -1
    assert b"strategy" in _capi.load(dev=_capi._use_dev).hps_last_error()
    torch.cuda.synchronize()
    for px, out, ws, length, bound in keep:                          # nothing ran: neither picture's buffers were touched
        assert int(length.item()) == -1 and bool((out == 0xA5).all())


def test_device_png_writer_dynamic(dev, tmp_path):
    pictures = [S.figure_like(), D.photo_like()[:30, :50], S.ramp(9, 301, 1, False)]
    writer = visualise.DevicePngWriter(workers=2, strategy="dynamic")
    try:
        paths = [str(tmp_path / ("p%d.png" % i)) for i in range(len(pictures))]
        writer.write_many([torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in pictures], paths)
        writer.drain()
    finally:
        writer.close()
    for img, path in zip(pictures, paths):
        assert open(path, "rb").read() == D.reference_encode_dynamic(img), path
    assert not [f for f in os.listdir(str(tmp_path)) if f.endswith(".part")]
    with pytest.raises(ValueError, match="strategy"):
        visualise.DevicePngWriter(strategy="zlib")


# ---- through the predict loop (the harness of tests/test_gpu_png.py) ------------------------------------------------------------------------
def test_predict_with_the_dynamic_device_encoder_writes_the_same_pixels(dev, net_gpu, smpl_gpu, tmp_path):
    from PIL import Image
    import test_gpu_predict_vis as T                                 # its toy detector, toy HRNet and DensePose table, by import only
    from hierarchicalprobabilistic3dhuman_amd.canny_edge_detector import CannyEdgeDetector
    from hierarchicalprobabilistic3dhuman_amd import predict_poseMF_shapeGaussian_net as P
    cfg = configs.get_cfg_defaults()
    image_dir = tmp_path / "images"
    os.makedirs(str(image_dir))
    rs = np.random.RandomState(5)
    sizes = {"a": (60, 60), "b": (48, 72)}
    for name, (h, w) in sizes.items():
        base = rs.rand(h // 4, w // 4, 3)
        np.save(str(image_dir / (name + ".npy")), (np.kron(base, np.ones((4, 4, 1))) * 255).astype(np.uint8))
    hrnet, detector = T._ToyHRNet().to(dev), T._ToyDetector().to(dev)
    hrnet_cfg = NS(MODEL=NS(IMAGE_SIZE=[288, 384], HEATMAP_SIZE=[72, 96]))
    edge = CannyEdgeDetector(non_max_suppression=cfg.DATA.EDGE_NMS, gaussian_filter_std=cfg.DATA.EDGE_GAUSSIAN_STD,
                             gaussian_filter_size=cfg.DATA.EDGE_GAUSSIAN_SIZE, threshold=cfg.DATA.EDGE_THRESHOLD).to(dev)
    renderer = tr.TexturedIUVRenderer(dev, 1, img_wh=T.WH, projection_type="orthographic", render_rgb=True, bin_size=32,
                                      densepose_uv=T._densepose(smpl_gpu.num_verts))

    def run(encoder, **kw):
        save_dir = tmp_path / ("out_" + encoder)
        torch.manual_seed(11)
        P.predict_poseMF_shapeGaussian_net(net_gpu, cfg, smpl_gpu, hrnet, hrnet_cfg, edge, dev, str(image_dir), str(save_dir),
                                           object_detect_model=detector, visualise_wh=T.WH, visualise_uncropped=True, visualise_samples=True,
                                           num_samples=12, batch_size=1, vis_renderer=renderer, **kw)
        return save_dir

    pil_dir, device_dir = run("pil"), run("dynamic", png_encoder="device-dynamic")
    assert sorted(os.listdir(str(pil_dir))) == sorted(os.listdir(str(device_dir)))
    dynamic_segments = 0
    for name, (h, w) in sizes.items():
        for suffix, shape in (("", (2 * T.WH, 4 * T.WH, 3)), ("_uncrop", (h, w, 3)), ("_samples", (3 * T.WH, 6 * T.WH, 3))):
            want = np.asarray(Image.open(str(pil_dir / (name + suffix + ".png"))))
            data = open(str(device_dir / (name + suffix + ".png")), "rb").read()
            got = S.read_png(data)
            assert got.shape == shape and np.array_equal(got, want), name + suffix
            assert np.array_equal(np.asarray(Image.open(io.BytesIO(data))), want), name + suffix
            dynamic_segments += sum(1 for p in S.idat_payloads(data)[1:-1] if p[0] & 6 == 4)         # BTYPE = 10
    assert dynamic_segments > 0
    assert not [f for f in os.listdir(str(device_dir)) if f.endswith(".part")]
    with pytest.raises(ValueError, match="png_encoder"):
        run("other", png_encoder="zlib")
