"""Host side of the device JPEG decoder: the NumPy restatement of tests/jpeg_scenario.py against PIL, hps_jpeg_parse's three answers,
and the library's shared decode source (csrc/jpeg_decode.h) run on the CPU under the address and undefined-behaviour sanitizers by a
stand-alone program (tests/jpeg_host_check.cpp).  Nothing here needs a GPU, and the tests preload nothing and leave the environment as it is."""
import io
import os
import pickle
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_scenario as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_equals_pil_byte_for_byte():
    if not S.turbo():
        pytest.skip("PIL is not built on libjpeg-turbo: its defaults are not the ones restated here")
    assert len(S.cases()) == 648
    for name, data in S.cases():
        got, want = S.restated(name)["pixels"], S.pil_pixels(data)
        assert got.shape == want.shape and np.array_equal(got, want), name
    name, data = S.cases()[0]
    assert np.array_equal(S.as_rgb(S.restated(name)["pixels"]), S.pil_pixels(data, rgb=True))


def test_parse_reads_the_header():
    import ctypes
    from hierarchicalprobabilistic3dhuman_amd import _capi, jpeg
    lib = _capi.load()
    assert lib.hps_sizeof_jpeg_header() == ctypes.sizeof(_capi.JpegHeader)
    assert lib.hps_sizeof_jpeg_decode_args() == ctypes.sizeof(_capi.JpegDecodeArgs)
    assert _capi.query_workspace(_capi.WS_JPEG, *_capi.jpeg_ws_dims(jpeg.parse(S.cases()[5][1]))) > 0
    with pytest.raises(_capi.HpsError):
        _capi.query_workspace(_capi.WS_JPEG, 100, 8 + (9000 << 32), 3 + (2 << 8) + (2 << 16))
    for name, data in S.cases()[::7]:
        info, h = S.restated(name)["info"], jpeg.parse(data)
        assert (h.width, h.height, h.ncomp, h.hs, h.vs, h.restart_interval) == (
            info["width"], info["height"], len(info["comps"]), info["comps"][0][0], info["comps"][0][1], info["ri"]), name
        assert data[h.scan_offset:h.scan_offset + h.scan_length] == info["scan"], name
        assert h.num_blocks == S.restated(name)["coefs"].shape[0] and h.file_bytes == len(data)
        for c, comp in enumerate(info["comps"]):
            assert list(h.quant[c]) == comp[2].tolist()
            assert list(h.dc[c].bits) == comp[3][0] and list(h.dc[c].vals)[:len(comp[3][1])] == comp[3][1]
            assert list(h.ac[c].bits) == comp[4][0] and list(h.ac[c].vals)[:len(comp[4][1])] == comp[4][1]
    e = pickle.loads(pickle.dumps(jpeg.EncodedJpeg(data, name="x.jpg")))
    assert e.data == data and bytes(e.header) == bytes(jpeg.parse(data)) and e.name == "x.jpg"


def _pil_file(pixels, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(pixels).save(buf, "JPEG", **kw)
    return buf.getvalue()


def test_parse_refuses_what_is_outside_the_profile():
    from PIL import Image
    from hierarchicalprobabilistic3dhuman_amd import jpeg
    rgb = S.picture(40, 24, False, 5)
    with pytest.raises(jpeg.JpegUnsupported, match="progressive"):
        jpeg.parse(S.encode(rgb, progressive=True))
    buf = io.BytesIO()
    Image.fromarray(np.concatenate([rgb, rgb[:, :, :1]], 2), "CMYK").save(buf, "JPEG")
    with pytest.raises(jpeg.JpegUnsupported, match="4 components"):
        jpeg.parse(buf.getvalue())
    # 4:2:0 rewritten so that Cb is sampled 2x1: chroma other than 1x1
    data = bytearray(S.encode(rgb, sampling="420"))
    sof = data.index(b"\xff\xc0")
    assert data[sof + 11] == 0x22 and data[sof + 14] == 0x11
    data[sof + 14] = 0x21
    with pytest.raises(jpeg.JpegUnsupported, match="sampling"):
        jpeg.parse(bytes(data))
    with pytest.raises(jpeg.JpegUnsupported, match="Adobe transform 0"):
        jpeg.parse(_pil_file(rgb, keep_rgb=True))                             # RGB stored as it is, marked by an Adobe segment
    big = S.encode(S.picture(2048, 1536, False, 1), quality=100, sampling="444")      # more entropy-coded data than the device takes
    assert len(big) > (1 << 22)
    with pytest.raises(jpeg.JpegUnsupported, match="entropy-coded data"):
        jpeg.parse(big)
    # greyscale asked of a colour file: no header problem, the caller's (encode_file) to refuse
    assert jpeg.parse(S.encode(rgb)).ncomp == 3


def test_parse_names_malformed_files():
    from hierarchicalprobabilistic3dhuman_amd import jpeg
    data = S.case_bytes("37x29_420_q75_std_none")
    with pytest.raises(ValueError, match="SOI"):
        jpeg.parse(b"\x89PNG\r\n\x1a\n" + data)
    for marker in (b"\xff\xdb", b"\xff\xc4", b"\xff\xc0", b"\xff\xda"):
        at = data.index(marker)
        for cut in (at + 2, at + 3, at + 6):                                  # inside the marker segment
            with pytest.raises(ValueError, match="past the file|ends"):
                jpeg.parse(data[:cut])
    # a scan that selects a table nobody defined
    sos = data.index(b"\xff\xda")
    bad = bytearray(data)
    bad[sos + 6] = 0x33
    with pytest.raises(ValueError, match="not defined"):
        jpeg.parse(bytes(bad))
    # Huffman counts that overflow the code space
    dht = data.index(b"\xff\xc4")
    bad = bytearray(data)
    bad[dht + 5] = 3                                                          # three codes of length 1
    with pytest.raises(ValueError, match="overflow"):
        jpeg.parse(bytes(bad))
    # a file cut inside its entropy-coded data still parses: the device reports it through its status word
    h = jpeg.parse(data)
    cut = jpeg.parse(data[:h.scan_offset + h.scan_length // 2])
    assert cut.scan_length == h.scan_length // 2


def _build_host_check(exe):
    """The stand-alone program with the sanitizers' runtimes linked STATICALLY, so that it runs under whatever the environment preloads
    (a shared ASan runtime insists on being the first library).  clang++ links them statically by default, g++ with -static-lib*san."""
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
             "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "hierarchicalprobabilistic3dhuman_amd", "csrc"),
             os.path.join(ROOT, "tests", "jpeg_host_check.cpp"), "-o", str(exe)]
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


def test_shared_decode_source_under_sanitizers(tmp_path):
    """csrc/jpeg_decode.h compiled for the host with -fsanitize=address,undefined: every case decodes to the restatement's coefficients,
    and 4 damaged copies of each (1296 cuts, 1296 byte flips) decode to an end with no sanitizer report."""
    exe = tmp_path / "jpeg_host_check"
    _build_host_check(exe)
    lines = []
    for i, (name, data) in enumerate(S.cases()):
        path = tmp_path / (name + ".jpg")
        path.write_bytes(data)
        lines.append("%s %016x 4 %d" % (path, S.restated(name)["checksum"], 77 + i))
    manifest = tmp_path / "manifest.txt"
    manifest.write_text("\n".join(lines) + "\n")
    r = subprocess.run([str(exe), str(manifest)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:]
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[:2] == ["files", "648"] and last[2:4] == ["damaged", "2592"] and last[-2:] == ["failures", "0"]
    assert int(last[7]) > 1000                                                # the damage is seen: most copies end with a status
