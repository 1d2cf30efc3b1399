"""hps_png_encode on the device (csrc/png.hip) against tests/png_scenario.py.  The yardstick is exact: every file is read back by the
scenario's own reader and by PIL, both must give the input picture byte for byte, and no file is longer than hps_png_bound.  The file
itself must be the stream include/hps.h documents (png_scenario.reference_encode restates it on the host).  Pictures are tiny and go
HPS_PNG_MAX_IMAGES to a call."""
import ctypes
import io
import os
import zlib
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import png_scenario as S
from hierarchicalprobabilistic3dhuman_amd import _capi, configs, textured_renderer as tr, visualise

pytestmark = pytest.mark.gpu


def _encode(pictures):
    """One hps_png_encode call over ``pictures`` (numpy uint8) -> the files' bytes."""
    assert 1 <= len(pictures) <= _capi.PNG_MAX_IMAGES
    a = _capi.PngEncodeArgs()
    a.struct_bytes, a.num_images = ctypes.sizeof(_capi.PngEncodeArgs), len(pictures)
    keep = []
    for i, img in enumerate(pictures):
        H, W = img.shape[:2]
        C = 3 if img.ndim == 3 else 1
        bound = visualise.png_bound(H, W, C)
        px = torch.from_numpy(np.ascontiguousarray(img)).cuda()
        out = torch.full((bound + 64,), 0xA5, dtype=torch.uint8, device="cuda")          # 64 guard bytes behind the capacity
        ws = torch.empty(max(16, _capi.query_workspace(_capi.WS_PNG, H, W, C)), dtype=torch.uint8, device="cuda")
        length = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        keep.append((px, out, ws, length, bound))
        im = a.image[i]
        im.pixels, im.H, im.W, im.C = _capi.ptr(px, torch.uint8), H, W, C
        im.out, im.capacity = _capi.ptr(out, torch.uint8), bound
        im.length, im.workspace = _capi.ptr(length, torch.int64), _capi.ptr(ws, torch.uint8)
    _capi.call("hps_png_encode", ctypes.addressof(a), _capi.stream())
    torch.cuda.synchronize()
    files = []
    for px, out, ws, length, bound in keep:
        n = int(length.item())
        assert 0 < n <= bound, (n, bound)
        host = out.cpu().numpy()
        assert (host[bound:] == 0xA5).all(), "bytes written behind the capacity"
        files.append(host[:n].tobytes())
    return files


def _encode_all(pictures):
    files = []
    for i in range(0, len(pictures), _capi.PNG_MAX_IMAGES):
        files += _encode(pictures[i:i + _capi.PNG_MAX_IMAGES])
    return files


def _check(name, img, data):
    from PIL import Image
    got = S.read_png(data)
    assert got.shape == img.shape and np.array_equal(got, img), name
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(data))), img), name
    assert len(data) <= visualise.png_bound(img.shape[0], img.shape[1], 3 if img.ndim == 3 else 1), name


def _check_cases(cases, exact_stream=True):
    files = _encode_all([img for _, img in cases])
    for (name, img), data in zip(cases, files):
        _check(name, img, data)
        if exact_stream:
            assert data == S.reference_encode(img), "%s: not the documented stream" % name
    return files


def test_run_lengths_around_the_match_limits(dev):
    cases = S.run_length_cases()
    files = _check_cases(cases)
    lengths = set()
    for data in files:
        for p in S.idat_payloads(data)[1:-1]:
            tokens, _ = S.fixed_block_tokens(p)
            for t in tokens or []:
                if t[0] == "match":
                    assert t[2] == 1 and 3 <= t[1] <= 258
                    lengths.add(t[1])
    assert {3, 4, 5, 6, 7, 257, 258}.issubset(lengths), sorted(lengths)


def test_both_literal_lengths_all_symbols_noise_and_ramps(dev):
    cases = S.symbol_cases()
    files = dict(zip([n for n, _ in cases], _check_cases(cases)))
    # noise takes the stored fallback; the ramps take Sub and Up
    assert all(S.fixed_block_tokens(p)[0] is None for p in S.idat_payloads(files["noise_c1"])[1:-1])
    for name, want in (("ramp_h_c1", 1), ("ramp_v_c1", 2)):
        raw = zlib.decompress(b"".join(S.idat_payloads(files[name])))
        W = dict(cases)[name].shape[1]
        assert {raw[y * (W + 1)] for y in range(1, 9)} == {want}, name


def test_every_byte_value_is_coded_as_a_literal(dev):
    """All 256 literal codes, 8-bit and 9-bit, through the fixed block: a picture whose first segment holds every byte value behind a run
    (the run makes the fixed block shorter than the stored one)."""
    img = np.concatenate([np.zeros((1, 600), dtype=np.uint8), S.all_bytes(1, 1, 5)[:, :256].reshape(1, 256)], axis=1)
    data, = _check_cases([("literals", img)])
    tokens, _ = S.fixed_block_tokens(S.idat_payloads(data)[1])
    assert tokens is not None
    seen = {t[1] for t in tokens if t[0] == "lit"}
    assert len(seen) >= 250 and min(seen) < 144 <= max(seen)


def test_segment_boundaries(dev):
    R, cases = S.boundary_cases()
    assert R == visualise.png_segment_rows(1, 5, 1)
    files = _check_cases(cases)
    for (name, img), data in zip(cases, files):
        assert len(S.idat_payloads(data)) == 2 + -(-img.shape[0] // R), name
    # a wider picture with two rows per segment and a last segment of one row
    W = 2048
    assert visualise.png_segment_rows(5, W, 3) == 2
    _check_cases([("two_rows_per_segment", S.repeating_rows(5, W, 3, 8)), ("two_rows_noise", S.noise(3, W, 3, 9))])


def test_segments_end_on_every_bit_offset(dev):
    family = [("end_bits_%d" % i, img) for i, img in enumerate(S.end_bit_family())]
    noise = [("noise_w%d" % w, S.noise(3, w, 1, w)) for w in range(1, 9)]
    files = _check_cases(family + noise)
    offsets = set()
    for data in files:
        offsets |= set(S.segment_end_bits(data))
    assert offsets == set(range(8)), offsets


def test_several_pictures_of_different_sizes_in_one_call(dev):
    cases = S.mixed_cases()
    files = _check_cases(cases)
    sizes = dict(zip([n for n, _ in cases], [len(f) for f in files]))
    assert sizes["figure"] < 64 * 128 * 3 // 2                      # a flat background with ellipses compresses


def test_determinism_alone_and_in_a_batch(dev):
    pictures = [S.noise(5, 9, 3, 1), S.constant(3, 300, 1), S.figure_like(), S.ramp(9, 301, 1, True)]
    first, second = _encode(pictures), _encode(pictures)
    assert first == second
    alone, = _encode([pictures[2]])
    assert alone == first[2]
    assert _encode([pictures[3], pictures[0], pictures[2]])[2] == alone


def test_matches_are_really_used(dev):
    img = S.constant(256, 256, 3)
    data, = _check_cases([("constant", img)])
    assert len(data) < img.size // 8, len(data)


# ---- DevicePngWriter ------------------------------------------------------------------------------------------------------------------
def test_device_png_writer(dev, tmp_path):
    pictures = [S.figure_like(), S.noise(7, 21, 3, 4), S.ramp(9, 301, 1, False), S.constant(3, 5, 1)[:, :, None]]
    writer = visualise.DevicePngWriter(workers=2)
    try:
        paths = [str(tmp_path / ("p%d.png" % i)) for i in range(len(pictures))]
        tensors = [torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in pictures]
        writer.write(tensors[0], paths[0])
        writer.write_many(tensors[1:], paths[1:])
        for round_ in range(3):                                      # more pictures than 2 x workers: the writer throttles, buffers are reused
            writer.write_many(tensors[:3], [str(tmp_path / ("r%d_%d.png" % (round_, i))) for i in range(3)])
        writer.drain()
        assert sorted(os.listdir(str(tmp_path))) == sorted(["p%d.png" % i for i in range(4)] + ["r%d_%d.png" % (r, i) for r in range(3) for i in range(3)])
        for i, (img, path) in enumerate(zip(pictures, paths)):
            data = open(path, "rb").read()
            _check(path, img[:, :, 0] if img.ndim == 3 and img.shape[2] == 1 else img, data)
        for r in range(3):
            for i in range(3):
                assert open(str(tmp_path / ("r%d_%d.png" % (r, i))), "rb").read() == open(paths[i], "rb").read()
        # an error on a worker surfaces in drain; the good file of the same call is still written
        writer.write_many(tensors[:2], [str(tmp_path / "missing_dir" / "x.png"), str(tmp_path / "after.png")])
        with pytest.raises(OSError):
            writer.drain()
        assert (tmp_path / "after.png").exists() and not [f for f in os.listdir(str(tmp_path)) if f.endswith(".part")]
        with pytest.raises(_capi.HpsError):
            writer.write(torch.zeros(4, 4, 2, dtype=torch.uint8, device="cuda"), str(tmp_path / "c2.png"))
        with pytest.raises(_capi.HpsError):
            writer.write(torch.zeros(4, 4, 3, dtype=torch.uint8), str(tmp_path / "cpu.png"))
    finally:
        writer.close()


# ---- through the predict loop ---------------------------------------------------------------------------------------------------------
def test_predict_with_the_device_encoder_writes_the_same_pixels(dev, net_gpu, smpl_gpu, tmp_path):
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

    pil_dir, device_dir = run("pil"), run("device", png_encoder="device")
    assert sorted(os.listdir(str(pil_dir))) == sorted(os.listdir(str(device_dir)))
    for name, (h, w) in sizes.items():
        for suffix, shape in (("", (2 * T.WH, 4 * T.WH, 3)), ("_uncrop", (h, w, 3)), ("_samples", (3 * T.WH, 6 * T.WH, 3))):
            want = np.asarray(Image.open(str(pil_dir / (name + suffix + ".png"))))
            data = open(str(device_dir / (name + suffix + ".png")), "rb").read()
            got = S.read_png(data)
            assert got.shape == shape and np.array_equal(got, want), name + suffix
            assert np.array_equal(np.asarray(Image.open(io.BytesIO(data))), want), name + suffix
    assert not [f for f in os.listdir(str(device_dir)) if f.endswith(".part")]
    with pytest.raises(ValueError, match="png_encoder"):
        run("other", png_encoder="zlib")
