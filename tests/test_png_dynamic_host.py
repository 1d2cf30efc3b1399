"""No GPU: the strategy-1 stream of hps_png_encode as tests/png_dynamic_scenario.py restates it (include/hps.h documents it) -- it decodes,
its codes keep deflate's length limits and are complete, the limiting pictures do reach the limits, and its size is held to the host's
zlib under Z_RLE on the same filtered rows and, for the photograph-like picture, to PIL's compress_level=1."""
import ctypes
import io
import zlib

import numpy as np
import pytest

import png_dynamic_scenario as D
import png_scenario as S
from hierarchicalprobabilistic3dhuman_amd import _capi

CASES = D.all_cases()


def _encoded():
    """Every case's restated file, made once: name -> (picture, file, [(kind, end_bit)] per segment)."""
    if not _encoded.cache:
        for name, img in CASES:
            data, kinds = D.reference_encode_dynamic(img, with_kinds=True)
            _encoded.cache[name] = (D._picture(img), data, kinds)
    return _encoded.cache


_encoded.cache = {}


def _pil_size(img, level=1):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format="PNG", compress_level=level)
    return len(buf.getvalue())


def _unlimited_depth(counts):
    return max(D.huffman_depths(sorted(c for c in counts if c)))


def test_case_names_are_unique_and_every_kind_of_segment_occurs():
    assert len({n for n, _ in CASES}) == len(CASES)
    kinds = {k for _, _, ks in _encoded().values() for k, _ in ks}
    assert kinds == {"dynamic", "fixed", "stored"}, kinds


def test_the_restated_files_decode_through_the_reader_and_pil():
    from PIL import Image
    for name, (img, data, _) in _encoded().items():
        got = S.read_png(data)
        assert got.shape == img.shape and np.array_equal(got, img), name
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(data))), img), name
        assert len(data) <= S.bound(img.shape[0], img.shape[1], 3 if img.ndim == 3 else 1), name


def test_code_lengths_keep_their_limits_and_the_codes_are_complete():
    seen = 0
    for name, (img, data, kinds) in _encoded().items():
        infos = D.segment_infos(data)
        assert [i is not None for i in infos] == [k == "dynamic" for k, _ in kinds], name
        for info in infos:
            if info is None:
                continue
            seen += 1
            assert max(info["ll"]) <= 15 and max(info["cl"]) <= 7, name
            assert info["hdist"] == 1 and info["dist"] == [1], name                  # one distance code of length 1
            assert info["ll"][-1] != 0 and info["ll"][256] != 0, name                # HLIT trimmed to the last used symbol
            assert info["hclen"] == max(4, max(k for k in range(19) if info["cl"][D.CL_ORDER[k]]) + 1), name
            for lens in (info["ll"], info["cl"]):
                if sum(1 for v in lens if v) >= 2:
                    assert D.kraft(lens) == (1 << 15, 1 << 15), name
            assert all(t[0] == "lit" or (t[2] == 1 and 3 <= t[1] <= 258) for t in info["tokens"]), name
    assert seen >= 30


def test_the_dynamic_blocks_end_on_every_bit_offset():
    """Measured from the files, over the end-bit family and every other case: the family was made for the fixed code, under which its
    single segments stay (a dynamic code's header costs them more than it saves), so the dynamic blocks' ends come from the rest."""
    fixed, dynamic = set(), set()
    for name, (img, data, kinds) in _encoded().items():
        for info, payload in zip(D.segment_infos(data), S.idat_payloads(data)[1:-1]):
            if info is not None:
                dynamic.add(info["end_bit"] % 8)
            elif name.startswith("end_bits_"):
                fixed.add(S.fixed_block_tokens(payload)[1] % 8)
    assert dynamic == set(range(8)), dynamic
    assert fixed == set(range(8)), fixed


def test_the_five_filter_picture_shows_all_five_filter_bytes():
    img = D.five_filters()
    raw = zlib.decompress(b"".join(S.idat_payloads(_encoded()["five_filters"][1])))
    rb = img.shape[1] + 1
    assert {raw[y * rb] for y in range(img.shape[0])} == {0, 1, 2, 3, 4}
    # ties go to the lowest type: a constant first row is as cheap under Sub as under Paeth, and the row below as cheap under Up as under Paeth
    rows = D.filtered_rows5(S.constant(3, 8, 1))
    assert rows[:, 0].tolist() == [1, 2, 2]
    assert D.filtered_rows5(np.zeros((2, 4), dtype=np.uint8))[:, 0].tolist() == [0, 0]


def test_the_limiting_pictures_reach_their_limits():
    """An unlimited Huffman code on the same counts is deeper than deflate allows; the documented construction stops at the limit."""
    for name, alphabet, limit in (("fibonacci_literals", "ll", 15), ("code_length_limit", "cl", 7)):
        img, data, kinds = _encoded()[name]
        assert [k for k, _ in kinds] == ["dynamic"], name                            # one segment, a dynamic block
        info, = D.segment_infos(data)
        if alphabet == "ll":
            counts = D.segment_histogram(info["tokens"])
        else:
            counts = [info["cl_symbols"].count(s) for s in range(19)]
        assert _unlimited_depth(counts) > limit, (name, _unlimited_depth(counts))
        assert max(info[alphabet]) == limit, name
        assert D.kraft(info[alphabet]) == (1 << 15, 1 << 15), name
    # the other alphabet of each picture is not at its limit: the two limits are reached separately
    assert max(D.segment_infos(_encoded()["fibonacci_literals"][1])[0]["cl"]) < 7
    assert max(D.segment_infos(_encoded()["code_length_limit"][1])[0]["ll"]) < 15


def test_size_against_zlib_rle_on_the_same_filtered_rows():
    """At most 1.01 x the host's zlib (Z_RLE: dynamic Huffman, distance-1 matches) per segment in the same container, plus 4 bytes per
    segment."""
    for name, (img, data, kinds) in _encoded().items():
        R = S.segment_rows(img.shape[0], img.shape[1], 3 if img.ndim == 3 else 1)
        yard = D.rle_yardstick(D.filtered_rows5(img), R, img)
        assert np.array_equal(S.read_png(yard), img), name
        assert len(data) <= 1.01 * len(yard) + 4 * len(kinds), (name, len(data), len(yard), len(kinds))


def test_size_against_pil():
    """The photograph-like picture is smaller than PIL's compress_level=1 file (23 706 against 26 329 bytes: 0.900; strategy 0: 44 532).
    The figure_like ratios are recorded only (pytest -s shows them): 1.216 at 64 x 128 (3 796 against 3 121 bytes) and 1.534 at 256 x 512,
    seed 5 (126 569 against 82 506) -- zlib finds LZ matches in the periodic sine texture, this tokeniser only runs."""
    img = D.photo_like()
    assert img.shape == (96, 160, 3)
    ours, pil = len(_encoded()["photo_like"][1]), _pil_size(img)
    print("\nphoto_like: strategy 1 %d bytes, strategy 0 %d, PIL compress_level=1 %d: ratio %.3f" % (ours, len(S.reference_encode(img)), pil, ours / pil))
    for shape in ((64, 128, 3), (256, 512, 5)):
        fig = S.figure_like(*shape)
        a, b = len(D.reference_encode_dynamic(fig)), _pil_size(fig)
        print("figure_like%r: strategy 1 %d bytes, strategy 0 %d, PIL compress_level=1 %d: ratio %.3f" % (shape, a, len(S.reference_encode(fig)), b, a / b))
    assert ours < 1.0 * pil, (ours, pil)


def test_the_code_length_sequence_rule():
    assert D.code_length_tokens([0] * 2 + [5]) == [(0, 0, 0), (0, 0, 0), (5, 0, 0)]
    assert D.code_length_tokens([0] * 3 + [5]) == [(17, 3, 0), (5, 0, 0)]
    assert D.code_length_tokens([0] * 10 + [5]) == [(17, 3, 7), (5, 0, 0)]
    assert D.code_length_tokens([0] * 11 + [5]) == [(18, 7, 0), (5, 0, 0)]
    assert D.code_length_tokens([0] * 138 + [5]) == [(18, 7, 127), (5, 0, 0)]
    assert D.code_length_tokens([0] * 140 + [5]) == [(18, 7, 127), (0, 0, 0), (0, 0, 0), (5, 0, 0)]
    assert D.code_length_tokens([0] * 141 + [5]) == [(18, 7, 127), (17, 3, 0), (5, 0, 0)]
    assert D.code_length_tokens([7] * 3) == [(7, 0, 0)] * 3
    assert D.code_length_tokens([7] * 4) == [(7, 0, 0), (16, 2, 0)]
    assert D.code_length_tokens([7] * 7 + [1]) == [(7, 0, 0), (16, 2, 3), (1, 0, 0)]
    assert D.code_length_tokens([7] * 9) == [(7, 0, 0), (16, 2, 3), (7, 0, 0), (7, 0, 0)]
    assert D.code_length_tokens([7] * 10) == [(7, 0, 0), (16, 2, 3), (16, 2, 0)]


def test_limited_lengths_on_small_alphabets():
    assert D.limited_lengths([0, 9, 0], 7) == [0, 1, 0]
    assert D.limited_lengths([4, 0, 4], 7) == [1, 0, 1]
    assert D.limited_lengths([1, 1, 1], 7) == [1, 2, 2]                              # ties: the lower index takes the shorter code
    assert D.limited_lengths([1, 1, 2, 4, 8], 3) == [3, 3, 3, 3, 1]                  # 4 4 3 2 1 unlimited; the repair keeps the sum at 1
    rs = np.random.RandomState(0)
    for _ in range(50):
        counts = (rs.geometric(rs.uniform(0.001, 0.3), rs.randint(2, 287)) - 1).tolist()
        if sum(1 for c in counts if c) < 2:
            continue
        for limit in (15, 9):
            lens = D.limited_lengths(counts, limit)
            assert max(lens) <= limit and D.kraft(lens) == (1 << 15, 1 << 15)
            assert all((a > 0) == (c > 0) for a, c in zip(lens, counts))
            order = sorted((s for s in range(len(counts)) if counts[s]), key=lambda s: (-counts[s], s))
            assert all(lens[a] <= lens[b] for a, b in zip(order, order[1:]))        # a more frequent symbol never has the longer code


# ---- the library's host side and the Python interface ----------------------------------------------------------------------------------
def _args(strategy):
    lib = _capi.load()
    a = _capi.PngEncodeArgs()
    a.struct_bytes, a.num_images = ctypes.sizeof(_capi.PngEncodeArgs), 2
    for i in range(2):
        im = a.image[i]
        im.H, im.W, im.C = 4, 5, 3
        im.capacity = lib.hps_png_bound(4, 5, 3)
        im.strategy = strategy if i == 1 else 0
        for k in ("pixels", "out", "length", "workspace"):          # never dereferenced: every check comes before the launch
            setattr(im, k, ctypes.c_void_p(4096))
    return lib, a


@pytest.mark.parametrize("strategy", [2, -1, 256])
def test_an_unknown_strategy_is_refused_before_any_launch(strategy):
    lib, a = _args(strategy)
    assert lib.hps_png_encode(ctypes.byref(a), None) == -1
    assert b"strategy" in lib.hps_last_error(), lib.hps_last_error()


def test_the_struct_keeps_its_size_and_the_strategy_its_place():
    lib = _capi.load()
    assert lib.hps_sizeof_png_encode_args() == ctypes.sizeof(_capi.PngEncodeArgs)
    assert _capi.PngImage.strategy.offset == _capi.PngImage.C.offset + 4 and ctypes.sizeof(_capi.PngImage) == 56
    assert _capi.PngEncodeArgs().image[0].strategy == 0


def test_predict_accepts_device_dynamic_and_still_refuses_zlib():
    from hierarchicalprobabilistic3dhuman_amd.predict_poseMF_shapeGaussian_net import predict_poseMF_shapeGaussian_net
    with pytest.raises(ValueError, match="png_encoder"):
        predict_poseMF_shapeGaussian_net(None, None, None, None, None, None, "cpu", "/nonexistent", "/nonexistent", png_encoder="zlib")
    with pytest.raises(Exception) as e:                              # past the argument check: it fails on the missing directory instead
        predict_poseMF_shapeGaussian_net(None, None, None, None, None, None, "cpu", "/nonexistent", "/nonexistent", png_encoder="device-dynamic")
    assert not (isinstance(e.value, ValueError) and "png_encoder" in str(e.value)), e.value


def test_the_writer_refuses_an_unknown_strategy():
    from hierarchicalprobabilistic3dhuman_amd import visualise
    with pytest.raises(ValueError, match="strategy"):
        visualise.DevicePngWriter(strategy="zlib")
    assert visualise.DevicePngWriter.STRATEGIES == {"fixed": 0, "dynamic": 1}
