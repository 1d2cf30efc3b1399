"""Host side of the device JPEG encoder: the NumPy restatement of tests/jpeg_encode_scenario.py against PIL's bytes, the corners its
case list must reach (asserted from the restatement's own symbol stream), hps_jpeg_encode_bound, the predict loop's argument checks,
and the library's shared encode source (csrc/jpeg_encode.h) run on the CPU under the address and undefined-behaviour sanitizers by a
stand-alone program (tests/jpeg_encode_host_check.cpp).  Nothing here needs a GPU, and the tests preload nothing and leave the
environment as it is."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_encode_scenario as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _channels(px):
    return 3 if px.ndim == 3 else 1


def test_restatement_equals_pil_byte_for_byte():
    if not E.turbo():
        pytest.skip("PIL is not built on libjpeg-turbo: its defaults are not the ones restated here")
    assert len(E.cases()) == 96
    for name, px, quality, sampling in E.cases():
        got, want = E.restated(name)["data"], E.pil_encode(px, quality, sampling)
        assert got == want, "%s: %d bytes against %d" % (name, len(got), len(want))


def test_case_list_reaches_the_coders_corners():
    every = {name: E.restated(name) for name, _, _, _ in E.cases()}
    symbols = lambda name: every[name]["symbols"]
    assert any(s[0] == "zrl" for r in every.values() for s in r["symbols"])
    assert any(r["blocks_without_eob"] for r in every.values())
    # the extreme picture: an AC value of 10 bits (|AC| = 924) and a DC difference of 11 bits (a step of 2040)
    ac = [s for s in symbols("extreme_grey_q100") if s[0] == "ac"]
    dc = [s for s in symbols("extreme_grey_q100") if s[0] == "dc"]
    assert max(s[2] for s in ac) == 10 and max(abs(s[3]) for s in ac) == 924
    assert max(s[1] for s in dc) == 11 and max(abs(s[2]) for s in dc) == 2040
    assert any(s[0] == "dc" and s[1] == 11 for s in symbols("extreme_420_q100"))
    # stuffing: 64 x 64 binary noise at quality 100
    assert every["stuffing_grey_q100"]["stuffed"] >= 100 and every["stuffing_444_q100"]["stuffed"] >= 100
    # dummy columns (1: 24 and 40 are no multiples of 16) and dummy rows (2: neither are 24 and 8) under 4:2:0, columns only under 4:2:2
    assert every["24x24_420_q95"]["dummy"] == {1, 2} and every["40x8_420_q95"]["dummy"] == {1, 2} and every["24x24_422_q95"]["dummy"] == {1}
    assert every["16x16_420_q95"]["dummy"] == set() and every["33x17_420_q95"]["dummy"] == {1, 2}
    assert not every["24x24_444_q95"]["dummy"] and not every["24x24_grey_q95"]["dummy"]
    # the final padding: none, and every length from 1 to 7 bits
    assert {r["pad_bits"] for r in every.values()} == set(range(8))
    # qualities below 50 and 100, every sampling, the smallest picture
    names = set(every)
    for sampling in E.SAMPLINGS:
        assert {"1x1_%s_q30" % sampling, "16x16_%s_q100" % sampling, "17x33_%s_q1" % sampling, "250x130_%s_q95" % sampling} <= names
    # a constant picture is the shortest scan: one DC symbol in the first block of each component, EOB everywhere
    c = every["constant_grey_q95"]
    assert all(s[0] in ("dc", "eob") for s in c["symbols"]) and sum(s[0] == "dc" and s[1] > 0 for s in c["symbols"]) == 1


def test_encode_bound_holds_and_refuses():
    from hierarchicalprobabilistic3dhuman_amd import _capi, jpeg
    lib = _capi.load()
    assert lib.hps_sizeof_jpeg_encode_args() == ctypes.sizeof(_capi.JpegEncodeArgs)
    for name, px, quality, sampling in E.cases():
        H, W = px.shape[:2]
        bound = jpeg.encode_bound(H, W, _channels(px), E.SAMPLING_CODE[sampling])
        assert bound >= len(E.restated(name)["data"]), name
        blocks = E.restated(name)["coefs"].shape[0]
        assert bound == E.noise_bound_bytes(blocks, _channels(px)), name
        assert _capi.query_workspace(_capi.WS_JPEG_ENC, H, W, _capi.jpeg_enc_d2(_channels(px), E.SAMPLING_CODE[sampling])) >= 128 * blocks
    # noise at quality 100: what compresses worst
    rs = np.random.RandomState(3)
    for shape, sampling in (((64, 64), "grey"), ((48, 40, 3), "444"), ((33, 47, 3), "420")):
        px = rs.randint(0, 256, shape).astype(np.uint8)
        data = E.pil_encode(px, 100, sampling)
        assert jpeg.encode_bound(px.shape[0], px.shape[1], _channels(px), sampling if sampling != "grey" else 0) >= len(data)
    assert jpeg.encode_bound(8, 8, 1, 7) == jpeg.encode_bound(8, 8, 1, 0)       # the sampling of a greyscale picture is ignored
    for H, W, C, s in ((0, 1, 1, 0), (1, 0, 3, 0), (1, 1, 2, 0), (8193, 1, 1, 0), (1, 8193, 3, 2), (8, 8, 3, 3), (8, 8, 3, -1)):
        assert lib.hps_jpeg_encode_bound(H, W, C, s) == -1 and b"hps_jpeg_encode_bound" in lib.hps_last_error()
        assert lib.hps_query_workspace(_capi.WS_JPEG_ENC, H, W, C + (s << 8)) == -1
        with pytest.raises(_capi.HpsError):
            jpeg.encode_bound(H, W, C, s)
    assert lib.hps_jpeg_encode_bound(8192, 8192, 3, 0) > 0


def test_bad_arguments_are_refused_on_the_host():
    """Everything hps_jpeg_encode refuses is refused before any launch, so also without a GPU."""
    from hierarchicalprobabilistic3dhuman_amd import _capi
    lib = _capi.load()

    def args(**kw):
        a = _capi.JpegEncodeArgs()
        a.struct_bytes, a.num_images = ctypes.sizeof(_capi.JpegEncodeArgs), 1
        im = a.image[0]
        im.pixels, im.out, im.length, im.workspace = 4096, 8192, 16384, 32768
        im.H, im.W, im.C, im.quality, im.sampling = 8, 8, 3, 95, 2
        im.capacity = lib.hps_jpeg_encode_bound(8, 8, 3, 2)
        for k, v in kw.items():
            setattr(a if k in ("struct_bytes", "num_images") else im, k, v)
        return a

    assert lib.hps_jpeg_encode(None, None) == -1
    for kw, word in ((dict(C=2), b"C is"), (dict(H=0), b"H and W"), (dict(W=8193), b"H and W"), (dict(quality=0), b"quality"),
                     (dict(quality=101), b"quality"), (dict(sampling=3), b"sampling"), (dict(capacity=lib.hps_jpeg_encode_bound(8, 8, 3, 2) - 1), b"capacity"),
                     (dict(out=8192 + 8), b"aligned"), (dict(pixels=4097), b"aligned"), (dict(workspace=32768 + 4), b"aligned"),
                     (dict(length=16384 + 4), b"8-byte"), (dict(out=None), b"null"), (dict(length=None), b"null"),
                     (dict(struct_bytes=8), b"struct_bytes"), (dict(num_images=0), b"num_images"), (dict(num_images=9), b"num_images")):
        assert lib.hps_jpeg_encode(ctypes.byref(args(**kw)), None) == -1, kw
        assert word in lib.hps_last_error(), (kw, lib.hps_last_error())


def test_predict_refuses_an_unknown_picture_format_and_jpeg_with_a_png_encoder():
    from hierarchicalprobabilistic3dhuman_amd.predict_poseMF_shapeGaussian_net import predict_poseMF_shapeGaussian_net
    with pytest.raises(ValueError, match="picture_format"):
        predict_poseMF_shapeGaussian_net(None, None, None, None, None, None, "cpu", "/nonexistent", "/nonexistent", picture_format="webp")
    with pytest.raises(ValueError, match="picture_format.*png_encoder"):
        predict_poseMF_shapeGaussian_net(None, None, None, None, None, None, "cpu", "/nonexistent", "/nonexistent", picture_format="jpeg",
                                         png_encoder="device")


def _build_host_check(exe):
    """The stand-alone program with the sanitizers' runtimes linked STATICALLY, so that it runs under whatever the environment preloads
    (a shared ASan runtime insists on being the first library).  clang++ links them statically by default, g++ with -static-lib*san."""
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
             "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "hierarchicalprobabilistic3dhuman_amd", "csrc"),
             os.path.join(ROOT, "tests", "jpeg_encode_host_check.cpp"), "-o", str(exe)]
    tried = []
    for cand in (os.environ.get("CXX"), "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++", "g++"):
        cxx = shutil.which(cand) if cand else None
        if not cxx:
            continue
        version = subprocess.run([cxx, "--version"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True).stdout
        static = [] if "clang" in version else ["-static-libasan", "-static-libubsan"]
        r = subprocess.run([cxx] + static + flags, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode == 0:
            return cxx
        tried.append("%s: %s" % (cxx, r.stdout[-500:]))
    raise AssertionError("no host C++ compiler built the sanitizer program (CXX, clang++, g++):\n" + "\n".join(tried))


def test_shared_encode_source_under_sanitizers(tmp_path):
    """csrc/jpeg_encode.h compiled for the host with -fsanitize=address,undefined: every case's whole file, built block after block,
    equals the restatement's bytes, with no sanitizer report."""
    exe = tmp_path / "jpeg_encode_host_check"
    _build_host_check(exe)
    lines = []
    for name, px, quality, sampling in E.cases():
        pixels, expected = tmp_path / (name + ".raw"), tmp_path / (name + ".jpg")
        pixels.write_bytes(np.ascontiguousarray(px).tobytes())
        expected.write_bytes(E.restated(name)["data"])
        lines.append("%s %s %d %d %d %d %d" % (pixels, expected, px.shape[0], px.shape[1], _channels(px), quality, E.SAMPLING_CODE[sampling]))
    manifest = tmp_path / "manifest.txt"
    manifest.write_text("\n".join(lines) + "\n")
    r = subprocess.run([str(exe), str(manifest)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert r.stdout.strip().splitlines()[-1].split() == ["files", "96", "failures", "0"]
