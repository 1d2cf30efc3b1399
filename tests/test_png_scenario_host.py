"""No GPU: the PNG yardsticks of tests/png_scenario.py are held to PIL and zlib, and hps_png_encode's host side -- argument checks, the
bound, the segment rule -- is called through the C ABI with a null stream (nothing is launched: every check comes before)."""
import ctypes
import io
import struct
import zlib

import numpy as np
import pytest

import png_scenario as S
from hierarchicalprobabilistic3dhuman_amd import _capi

SIZES = [(1, 1), (1, 2), (2, 1), (3, 5), (7, 4), (16, 16), (33, 9), (40, 70)]


def _pictures():
    for i, (h, w) in enumerate(SIZES):
        for C in (1, 3):
            yield S.noise(h, w, C, i) if i % 2 else S.ramp(h, w, C, True)


def _pil_bytes(img, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format="PNG", **kw)
    return buf.getvalue()


def test_reader_returns_pil_pixels_on_pil_files():
    from PIL import Image
    for img in _pictures():
        for level in (0, 1, 9):                                    # PIL picks its filters adaptively: all five types occur over the set
            data = _pil_bytes(img, compress_level=level)
            got = S.read_png(data)
            assert got.shape == img.shape and np.array_equal(got, img)
            assert np.array_equal(got, np.asarray(Image.open(io.BytesIO(data))))


def test_reader_undoes_all_five_filter_types():
    """Files whose rows carry a chosen filter type, filtered here independently of the reader's code path (forward filters)."""
    img = S.noise(6, 11, 3, 9)
    H, W, C = img.shape
    flat = img.reshape(H, -1).astype(np.int64)
    rows = bytearray()
    for y in range(H):
        ft = y % 5
        prev = flat[y - 1] if y else np.zeros(W * C, dtype=np.int64)
        line = []
        for x in range(W * C):
            a = flat[y, x - C] if x >= C else 0
            c = prev[x - C] if x >= C else 0
            pred = [0, a, prev[x], (a + prev[x]) // 2, S._paeth(int(a), int(prev[x]), int(c))][ft]
            line.append((flat[y, x] - pred) & 255)
        rows += bytes([ft]) + bytes(line)
    data = S.SIGNATURE + S._chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)) + S._chunk(b"IDAT", zlib.compress(bytes(rows))) + S._chunk(b"IEND", b"")
    from PIL import Image
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(data))), img)
    assert np.array_equal(S.read_png(data), img)


@pytest.mark.parametrize("rows_per_segment", [1, 16])
def test_reader_and_pil_take_a_segmented_multi_idat_file(rows_per_segment):
    from PIL import Image
    for img in _pictures():
        data = S.segmented_zlib_png(img, rows_per_segment)
        assert len(S.idat_payloads(data)) == 2 + -(-img.shape[0] // rows_per_segment)
        assert np.array_equal(S.read_png(data), img)
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(data))), img)


def _flip(data, byte, bit=0):
    out = bytearray(data)
    out[byte] ^= 1 << bit
    return bytes(out)


def test_reader_rejects_single_bit_damage():
    img = S.figure_like(20, 30)
    data = S.segmented_zlib_png(img, 4)
    assert np.array_equal(S.read_png(data), img)
    # chunk layout: signature 8, IHDR 25, the header chunk 14, then the first segment chunk
    first = 8 + 25 + 14
    n, = struct.unpack(">I", data[first:first + 4])
    with pytest.raises(S.PngError, match="CRC"):
        S.read_png(_flip(data, first + 8 + n + 3))                   # a bit of the segment chunk's CRC
    with pytest.raises(S.PngError, match="CRC"):
        S.read_png(_flip(data, first + 8 + n // 2, 5))               # a bit of a data byte: the chunk's CRC no longer matches
    # the same data bit with the chunk's CRC made right again: the deflate stream or the Adler-32 must catch it
    payload = bytearray(data[first + 8:first + 8 + n])
    payload[n // 2] ^= 1 << 5
    mended = data[:first] + S._chunk(b"IDAT", bytes(payload)) + data[first + 12 + n:]
    with pytest.raises(S.PngError):
        S.read_png(mended)
    # a bit of the Adler-32, with the closing chunk's CRC made right: zlib must refuse
    tail = len(data) - 12 - 18
    assert data[tail + 4:tail + 10] == b"IDAT\x03\x00"
    adler = bytearray(data[tail + 8:tail + 14])
    adler[3] ^= 1
    with pytest.raises(S.PngError, match="IDAT data"):
        S.read_png(data[:tail] + S._chunk(b"IDAT", bytes(adler)) + data[tail + 18:])
    with pytest.raises(S.PngError, match="CRC"):
        S.read_png(_flip(data, tail + 11))                           # the same bit with the CRC left alone
    with pytest.raises(S.PngError):
        S.read_png(data[:8 + 25] + data[8 + 25 + 14:])              # the zlib header chunk dropped


def test_the_documented_stream_is_a_valid_png_on_the_host():
    """reference_encode restates include/hps.h's stream; PIL and the reader decode it, it stays under the bound, and the token reader
    finds the segment ends where the encoder put them -- on all eight bit offsets over the family made for that."""
    from PIL import Image
    offsets = set()
    pictures = [p for _, p in S.symbol_cases() + S.boundary_cases()[1] + S.run_length_cases()[::7]] + S.end_bit_family()
    for img in pictures:
        data, ends = S.reference_encode(img, with_end_bits=True)
        assert np.array_equal(S.read_png(data), img) and np.array_equal(np.asarray(Image.open(io.BytesIO(data))), img)
        assert len(data) <= S.bound(img.shape[0], img.shape[1], 3 if img.ndim == 3 else 1)
        assert S.segment_end_bits(data) == [e % 8 for e in ends if e is not None]
    for img in S.end_bit_family():
        offsets |= set(S.segment_end_bits(S.reference_encode(img)))
    assert offsets == set(range(8))


# ---- the library's host side ----------------------------------------------------------------------------------------------------------
def _args(n=1, H=4, W=5, C=3, capacity=None, struct_bytes=None, **null):
    lib = _capi.load()
    a = _capi.PngEncodeArgs()
    a.struct_bytes = ctypes.sizeof(_capi.PngEncodeArgs) if struct_bytes is None else struct_bytes
    a.num_images = n
    for i in range(min(n, _capi.PNG_MAX_IMAGES)):
        im = a.image[i]
        im.H, im.W, im.C = H, W, C
        bound = lib.hps_png_bound(H, W, C)
        im.capacity = (bound if bound > 0 else 1 << 20) if capacity is None else capacity
        for k in ("pixels", "out", "length", "workspace"):          # never dereferenced: every check comes before the launch
            setattr(im, k, None if null.get(k) else ctypes.c_void_p(4096))
    return lib, a


def _refused(lib, a, text):
    rc = lib.hps_png_encode(ctypes.byref(a), None)
    assert rc == -1, rc
    assert text in lib.hps_last_error(), lib.hps_last_error()


def test_encode_refuses_bad_arguments_before_any_launch():
    lib, a = _args()
    assert lib.hps_sizeof_png_encode_args() == ctypes.sizeof(_capi.PngEncodeArgs)
    assert lib.hps_png_encode(None, None) == -1 and b"null pointer" in lib.hps_last_error()
    _refused(*_args(struct_bytes=ctypes.sizeof(_capi.PngEncodeArgs) - 8), b"struct_bytes")
    for k in ("pixels", "out", "length", "workspace"):
        _refused(*_args(**{k: True}), b"null pointer")
    _refused(*_args(C=2), b"C is 1 (greyscale) or 3 (RGB)")
    _refused(*_args(C=4), b"C is 1 (greyscale) or 3 (RGB)")
    _refused(*_args(H=0), b"H and W are at least 1")
    _refused(*_args(W=0), b"H and W are at least 1")
    _refused(*_args(W=-3), b"H and W are at least 1")
    _refused(*_args(W=4097), b"W C <= 12288")
    _refused(*_args(W=12289, C=1), b"W C <= 12288")
    _refused(*_args(H=32769, W=1, C=1), b"H <= 32768")
    bound = lib.hps_png_bound(4, 5, 3)
    _refused(*_args(capacity=bound - 1), b"capacity is below hps_png_bound")
    _refused(*_args(n=_capi.PNG_MAX_IMAGES + 1), b"num_images in [1, HPS_PNG_MAX_IMAGES]")
    _refused(*_args(n=0), b"num_images in [1, HPS_PNG_MAX_IMAGES]")
    assert _capi.PNG_MAX_IMAGES >= 4


def test_bound_and_segment_rows():
    lib = _capi.load()
    for H, W, C in ((0, 1, 1), (1, 0, 3), (1, 1, 2), (1, 4097, 3), (32769, 1, 1)):
        assert lib.hps_png_bound(H, W, C) == -1 and b"hps_png_bound" in lib.hps_last_error()
        assert lib.hps_png_segment_rows(H, W, C) == -1 and b"hps_png_segment_rows" in lib.hps_last_error()
        assert lib.hps_query_workspace(_capi.WS_PNG, H, W, C) == -1 and b"HPS_WS_PNG" in lib.hps_last_error()
    sizes = [1, 2, 3, 5, 8, 63, 64, 65, 100, 257, 1000, 1365, 1366, 2730, 2731, 4096]
    for C in (1, 3):
        grid = np.array([[lib.hps_png_bound(H, W, C) for W in sizes] for H in sizes], dtype=np.int64)
        assert (np.diff(grid, axis=0) > 0).all() and (np.diff(grid, axis=1) > 0).all()          # monotone in H and in W
        for i, H in enumerate(sizes):
            for j, W in enumerate(sizes):
                assert grid[i, j] >= H * W * C + H                                                # at least the raw (filtered) size
                assert grid[i, j] == S.bound(H, W, C)
                R = lib.hps_png_segment_rows(H, W, C)
                assert R == S.segment_rows(H, W, C) and 1 <= R <= 64 and R * (1 + W * C) <= max(16384, 1 + W * C)
                assert lib.hps_query_workspace(_capi.WS_PNG, H, W, C) >= -(-H // R) * (R * (1 + W * C) + 17)
    assert lib.hps_png_segment_rows(2, 4096, 3) == 1 and lib.hps_png_bound(2, 4096, 3) == 77 + 2 * 12289 + 34
    assert lib.hps_png_segment_rows(1536, 3072, 3) == 1 and lib.hps_png_segment_rows(1024, 2048, 3) == 2
    # the bound holds for the documented stream even where nothing compresses
    for img in (S.noise(70, 1, 1, 1), S.noise(9, 37, 3, 2), S.noise(2, 4096, 3, 3)):
        assert len(S.reference_encode(img)) <= lib.hps_png_bound(img.shape[0], img.shape[1], 3 if img.ndim == 3 else 1)


def test_predict_refuses_an_unknown_png_encoder():
    from hierarchicalprobabilistic3dhuman_amd.predict_poseMF_shapeGaussian_net import predict_poseMF_shapeGaussian_net
    with pytest.raises(ValueError, match="png_encoder"):
        predict_poseMF_shapeGaussian_net(None, None, None, None, None, None, "cpu", "/nonexistent", "/nonexistent", png_encoder="zlib")
