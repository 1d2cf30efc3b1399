"""hps_jpeg_encode on the device (csrc/jpeg_encode.hip) against PIL (libjpeg-turbo) and tests/jpeg_encode_scenario.py.  The yardstick
is exact: the device's file equals PIL's ``save(format="JPEG", quality=q, subsampling=s)`` byte for byte, whole file, and ``*length``
is its length.  Where PIL is not built on libjpeg-turbo the NumPy restatement of include/hps.h's rules stands in (it is held to PIL
by tests/test_jpeg_encode_scenario_host.py).  Pictures are tiny and go HPS_JPEG_ENC_MAX_IMAGES to a call."""
import ctypes
import io
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import jpeg_encode_scenario as E
from hierarchicalprobabilistic3dhuman_amd import _capi, configs, jpeg, textured_renderer as tr, visualise

pytestmark = pytest.mark.gpu

SENTINEL, GUARD = 0xA5, 64


def _expected(px, quality, sampling):
    return E.pil_encode(px, quality, sampling) if E.turbo() else E.restate(px, quality, sampling)["data"]


def _channels(px):
    return 3 if px.ndim == 3 else 1


def _encode(items):
    """One hps_jpeg_encode call over ``items`` = [(numpy uint8 picture, quality, sampling name)] -> the files' bytes.  ``out`` is
    filled with a sentinel first and has exactly the bound as its capacity: every byte from *length to 64 bytes behind the capacity
    must be unchanged."""
    assert 1 <= len(items) <= _capi.JPEG_ENC_MAX_IMAGES
    a = _capi.JpegEncodeArgs()
    a.struct_bytes, a.num_images = ctypes.sizeof(_capi.JpegEncodeArgs), len(items)
    keep = []
    for i, (img, quality, sampling) in enumerate(items):
        H, W = img.shape[:2]
        C, s = _channels(img), E.SAMPLING_CODE[sampling]
        bound = jpeg.encode_bound(H, W, C, s)
        px = torch.from_numpy(np.array(img, copy=True, order="C")).cuda()
        out = torch.full((bound + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
        ws = torch.empty(max(16, _capi.query_workspace(_capi.WS_JPEG_ENC, H, W, _capi.jpeg_enc_d2(C, s))), dtype=torch.uint8, device="cuda")
        length = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        keep.append((px, out, ws, length, bound))
        im = a.image[i]
        im.pixels, im.H, im.W, im.C, im.quality, im.sampling = _capi.ptr(px, torch.uint8), H, W, C, quality, s
        im.out, im.capacity = _capi.ptr(out, torch.uint8), bound
        im.length, im.workspace = _capi.ptr(length, torch.int64), _capi.ptr(ws, torch.uint8)
    _capi.call("hps_jpeg_encode", ctypes.addressof(a), _capi.stream())
    torch.cuda.synchronize()
    files = []
    for px, out, ws, length, bound in keep:
        n = int(length.item())
        assert 0 < n <= bound, (n, bound)
        host = out.cpu().numpy()
        assert (host[n:] == SENTINEL).all(), "bytes written behind the file's end"
        files.append(host[:n].tobytes())
    return files


def _encode_all(items):
    files = []
    for i in range(0, len(items), _capi.JPEG_ENC_MAX_IMAGES):
        files += _encode(items[i:i + _capi.JPEG_ENC_MAX_IMAGES])
    return files


def _assert_same(name, got, want):
    if got != want:
        at = next((i for i, (x, y) in enumerate(zip(got, want)) if x != y), min(len(got), len(want)))
        raise AssertionError("%s: %d bytes against %d, first difference at byte %d" % (name, len(got), len(want), at))


def test_files_equal_pil_byte_for_byte_on_the_case_list(dev):
    """1 x 1 ... 250 x 130 across grey, 4:4:4, 4:2:2 and 4:2:0 at qualities 30 and 95 (1, 75 and 100 on some), dummy columns and rows,
    the extreme-category pictures, the stuffing pictures, the zero-run pictures, constant pictures, every final padding."""
    cases = E.cases()
    files = _encode_all([(px, quality, sampling) for _, px, quality, sampling in cases])
    for (name, px, quality, sampling), data in zip(cases, files):
        _assert_same(name, data, E.restated(name)["data"])
        _assert_same(name + " (PIL)", data, _expected(px, quality, sampling))


def test_a_picture_over_several_workgroups_of_every_kernel(dev):
    """384 x 512 RGB: 4 608 blocks under 4:2:0 (24 workgroups of 192), 9 216 under 4:4:4; greyscale 3 072."""
    rgb = E.picture(512, 384, False, 77)
    assert rgb.shape == (384, 512, 3)
    items = [(rgb, 95, "420"), (rgb, 95, "444"), (rgb, 30, "422"), (np.ascontiguousarray(rgb[:, :, 1]), 100, "grey")]
    for (px, quality, sampling), data in zip(items, _encode(items)):
        _assert_same("384x512 %s q%d" % (sampling, quality), data, _expected(px, quality, sampling))


def test_independence_and_repeatability(dev):
    items = [(E.picture(33, 17, False, 1), 30, "420"), (E.picture(250, 130, True, 2), 95, "grey"), (E.stuffing(), 100, "grey"),
             (E.picture(40, 24, False, 3), 75, "444"), (E.picture(24, 24, False, 4), 95, "422")]
    first, second = _encode(items), _encode(items)
    assert first == second
    for k in (0, 1, 4):
        alone, = _encode([items[k]])
        assert alone == first[k], k
    mixed = _encode([items[4], items[2], items[0]])
    assert mixed == [first[4], first[2], first[0]]
    for (px, quality, sampling), data in zip(items, first):
        _assert_same("%s q%d" % (sampling, quality), data, _expected(px, quality, sampling))


def test_round_trip_through_the_device_decoder(dev):
    from PIL import Image
    items = [(E.picture(131, 67, False, 5), 95, "420"), (E.picture(50, 9, True, 6), 30, "grey"), (E.picture(37, 29, False, 7), 75, "420")]
    files = _encode(items)
    encoded = [jpeg.EncodedJpeg(data, name="case%d" % i) for i, data in enumerate(files)]          # jpeg.parse: in the device profile
    for e, (px, _, sampling) in zip(encoded, items):
        assert (e.height, e.width, e.ncomp) == (px.shape[0], px.shape[1], _channels(px))
        assert (e.header.hs, e.header.vs) == ((2, 2) if sampling == "420" else (1, 1))
    decoder = jpeg.DeviceJpegDecoder()
    pixels = decoder.decode(encoded, mode="native")
    decoder.check()
    for data, got in zip(files, pixels):
        want = np.asarray(Image.open(io.BytesIO(data)))
        assert got.shape == want.shape and np.array_equal(got.cpu().numpy(), want)


def test_bad_arguments_launch_nothing(dev):
    H = W = 16
    bound = jpeg.encode_bound(H, W, 3, 2)
    px = torch.zeros(H, W, 3, dtype=torch.uint8, device="cuda")
    out = torch.full((bound + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    ws = torch.empty(_capi.query_workspace(_capi.WS_JPEG_ENC, H, W, _capi.jpeg_enc_d2(3, 2)), dtype=torch.uint8, device="cuda")
    length = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    lib = _capi.load()

    def call(**kw):
        a = _capi.JpegEncodeArgs()
        a.struct_bytes, a.num_images = ctypes.sizeof(_capi.JpegEncodeArgs), 1
        im = a.image[0]
        im.pixels, im.H, im.W, im.C, im.quality, im.sampling = px.data_ptr(), H, W, 3, 95, 2
        im.out, im.capacity, im.length, im.workspace = out.data_ptr(), bound, length.data_ptr(), ws.data_ptr()
        for k, v in kw.items():
            setattr(im, k, v)
        return lib.hps_jpeg_encode(ctypes.byref(a), _capi.stream())

    for kw in (dict(C=2), dict(H=0), dict(W=8193), dict(quality=0), dict(quality=101), dict(sampling=3), dict(capacity=bound - 1),
               dict(out=out.data_ptr() + 8)):
        assert call(**kw) == -1, kw
        assert lib.hps_last_error().startswith(b"bad argument"), kw
    torch.cuda.synchronize()
    assert int(length.item()) == -1 and bool((out == SENTINEL).all())
    assert call() == 0                                                            # the same arguments, unchanged, are accepted
    torch.cuda.synchronize()
    n = int(length.item())
    assert out[:n].cpu().numpy().tobytes() == _expected(np.zeros((H, W, 3), np.uint8), 95, "420")


# ---- DeviceJpegWriter -----------------------------------------------------------------------------------------------------------------
def test_device_jpeg_writer(dev, tmp_path):
    pictures = [E.picture(128, 64, False, 8), E.picture(21, 7, False, 9), E.picture(301, 9, True, 10), E.constant(3, 5, 1)[:, :, None]]
    writer = visualise.DeviceJpegWriter(workers=2, quality=90, subsampling="420")
    want = [_expected(p[:, :, 0] if p.ndim == 3 and p.shape[2] == 1 else p, 90, "420" if p.ndim == 3 and p.shape[2] == 3 else "grey")
            for p in pictures]
    try:
        paths = [str(tmp_path / ("p%d.jpg" % i)) for i in range(len(pictures))]
        tensors = [torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in pictures]
        writer.write(tensors[0], paths[0])
        writer.write_many(tensors[1:], paths[1:])
        for round_ in range(3):                                      # more pictures than 2 x workers: the writer throttles, buffers are reused
            writer.write_many(tensors[:3], [str(tmp_path / ("r%d_%d.jpg" % (round_, i))) for i in range(3)])
        writer.drain()
        assert sorted(os.listdir(str(tmp_path))) == sorted(["p%d.jpg" % i for i in range(4)] + ["r%d_%d.jpg" % (r, i) for r in range(3) for i in range(3)])
        for i, path in enumerate(paths):
            _assert_same(path, open(path, "rb").read(), want[i])
        for r in range(3):
            for i in range(3):
                _assert_same("r%d_%d" % (r, i), open(str(tmp_path / ("r%d_%d.jpg" % (r, i))), "rb").read(), want[i])
        assert sum(len(v) for v in writer._free.values()) <= 2 * writer.workers + 3          # slots are reused, not made per picture
        # an error on a worker surfaces in drain; the good file of the same call is still written
        writer.write_many(tensors[:2], [str(tmp_path / "missing_dir" / "x.jpg"), str(tmp_path / "after.jpg")])
        with pytest.raises(OSError):
            writer.drain()
        _assert_same("after.jpg", open(str(tmp_path / "after.jpg"), "rb").read(), want[1])
        assert not [f for f in os.listdir(str(tmp_path)) if f.endswith(".part")]
        with pytest.raises(_capi.HpsError):
            writer.write(torch.zeros(4, 4, 2, dtype=torch.uint8, device="cuda"), str(tmp_path / "c2.jpg"))
        with pytest.raises(_capi.HpsError):
            writer.write(torch.zeros(4, 4, 3, dtype=torch.uint8), str(tmp_path / "cpu.jpg"))
    finally:
        writer.close()
    with pytest.raises(ValueError, match="subsampling"):
        visualise.DeviceJpegWriter(subsampling="411")


def test_device_jpeg_encoder_returns_device_tensors(dev):
    pictures = [E.picture(40, 24, False, 11), E.picture(40, 24, False, 12), E.picture(9, 7, True, 13)]
    enc = jpeg.DeviceJpegEncoder(quality=75, subsampling="422")
    pairs = enc.encode([torch.from_numpy(p).cuda() for p in pictures])
    assert all(out.is_cuda and length.is_cuda and length.dtype == torch.int64 for out, length in pairs)
    for p, (out, length) in zip(pictures, pairs):
        n = int(length.item())
        _assert_same("encoder", out[:n].cpu().numpy().tobytes(), _expected(p, 75, "422" if p.ndim == 3 else "grey"))


# ---- through the predict loop ---------------------------------------------------------------------------------------------------------
def test_predict_writes_jpeg_pictures_equal_to_pil(dev, net_gpu, smpl_gpu, tmp_path):
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

    def run(tag, **kw):
        save_dir = tmp_path / ("out_" + tag)
        torch.manual_seed(11)
        P.predict_poseMF_shapeGaussian_net(net_gpu, cfg, smpl_gpu, hrnet, hrnet_cfg, edge, dev, str(image_dir), str(save_dir),
                                           object_detect_model=detector, visualise_wh=T.WH, visualise_uncropped=True, visualise_samples=True,
                                           num_samples=12, batch_size=1, vis_renderer=renderer, **kw)
        return save_dir

    def pil_jpeg(pixels, quality):
        buf = io.BytesIO()
        Image.fromarray(pixels).save(buf, "JPEG", quality=quality)
        return buf.getvalue()

    png_dir, jpg_dir, q75_dir = run("png"), run("jpeg", picture_format="jpeg"), run("q75", picture_format="jpeg", picture_quality=75)
    suffixes = ("", "_uncrop", "_samples")
    for d in (jpg_dir, q75_dir):
        assert sorted(os.listdir(str(d))) == sorted([n + s + ".jpg" for n in sizes for s in suffixes] + [n + ".pt" for n in sizes])
    assert sorted(os.listdir(str(png_dir))) == sorted([n + s + ".png" for n in sizes for s in suffixes] + [n + ".pt" for n in sizes])
    for name in sizes:
        for suffix in suffixes:
            pixels = np.asarray(Image.open(str(png_dir / (name + suffix + ".png"))))
            for d, quality in ((jpg_dir, 95), (q75_dir, 75)):
                data = open(str(d / (name + suffix + ".jpg")), "rb").read()
                want = pil_jpeg(pixels, quality) if E.turbo() else E.restate(pixels, quality, "420")["data"]
                _assert_same("%s%s q%d" % (name, suffix, quality), data, want)
        want, got = torch.load(str(png_dir / (name + ".pt"))), torch.load(str(jpg_dir / (name + ".pt")))
        assert sorted(want) == sorted(got)
        for k in want:
            assert torch.equal(torch.as_tensor(want[k]), torch.as_tensor(got[k])), (name, k)
