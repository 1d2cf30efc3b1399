"""Time per image of writing the three predict pictures as PNG files, on one MI355X: visualise.PngWriter (bytes to the host, PIL on four
threads -- the yardstick, untouched) against visualise.DevicePngWriter (hps_png_encode on the device, only the file crosses) with
strategy "fixed" and with strategy "dynamic".

    python tools/png_encode_time.py [--out profiles/png_encode_time.txt] [--commit ID]

tools/predict_vis_time.py's scene and its three pictures at visualise_wh = 512: the eight-panel figure (1024 x 2048), the body over a
720 x 960 photograph, the 3 x 6 sample sheet (1536 x 3072).  The pictures are composed once; a round is, per writer, the host clock from
the finished device pictures to drained files in a temporary directory.  The three writers alternate round by round in one process:
3 warm-up rounds, then ``--rounds`` timed ones; median and quartiles.  Also recorded: the library's launches per image, the device
time of the library call alone under either strategy, the bytes copied to the host, and each picture's file sizes beside PIL's
compress_level=1 size.  The output is appended to ``--out``."""
import argparse
import ctypes
import os
import sys
import tempfile
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from hierarchicalprobabilistic3dhuman_amd import _capi, configs, textured_renderer as tr, visualise  # noqa: E402
import render_scenario as S  # noqa: E402


def pictures(dev):
    """The three pictures of tools/predict_vis_time.py's device route, as device tensors."""
    wh, D, H, W, N = 512, 256, 720, 960, 12
    cfg = configs.get_cfg_defaults()
    scene = S.make_scene(**dict(S.CASES["w256_smpl_b2"], W=wh, projection="orthographic"))
    dp = (torch.from_numpy(scene.verts_uv)[None], torch.from_numpy(scene.verts_iuv)[None], torch.from_numpy(scene.verts_map), torch.from_numpy(scene.faces)[None])
    vis = visualise.PredictVisualiser(tr.TexturedIUVRenderer(dev, 1, img_wh=wh, projection_type="orthographic", render_rgb=True, densepose_uv=dp), cfg, wh)
    g = torch.Generator().manual_seed(7)
    flip = torch.tensor([1.0, -1.0, -1.0])
    V = scene.V
    mode = torch.from_numpy(scene.vertices[0]) * flip
    result = {"verts_mode": mode.to(dev), "verts_tpose": (torch.from_numpy(scene.vertices[1]) * flip).to(dev),
              "unc": (0.25 * torch.rand(V, generator=g)).to(dev), "cam": torch.tensor([0.9, 0.0, 0.2], device=dev),
              "verts_samples": (mode[None] + 0.02 * torch.randn(N, V, 3, generator=g)).to(dev),
              "joints_samples": (0.4 * torch.randn(N, 90, 3, generator=g)).to(dev)}
    smooth = lambda c, h, w: F.interpolate(torch.rand(1, c, h // 16, w // 16, generator=g), size=(h, w), mode="bilinear", align_corners=False)
    crop = smooth(3, D, D).to(dev)
    proxy = ((torch.rand(1, 18, D, D, generator=g) < 0.05).float() * 0.5).to(dev)
    joints2D = (torch.rand(1, 17, 2, generator=g) * D).to(dev)
    photo = (smooth(3, H, W)[0].permute(1, 2, 0) * 255).to(torch.uint8).contiguous()
    image = (photo.permute(2, 0, 1).float() / 255.0).to(dev)
    centre, side = torch.tensor([380.0, 470.0], device=dev), torch.tensor([560.0], device=dev)
    with torch.no_grad():
        fig = vis.figure(result, crop, proxy, joints2D).clone()
        un = vis.uncropped(image, centre, side).clone()
        sheet = vis.samples_figure(result, crop, proxy).clone()
    torch.cuda.synchronize()
    return [("figure", fig), ("uncrop", un), ("samples", sheet)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_encode_time.txt"))
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--commit", default="working tree")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    from PIL import Image
    dev = torch.device("cuda", torch.cuda.current_device())
    pics = pictures(dev)
    tmp = tempfile.mkdtemp(prefix="png_encode_time_")
    writers = {"pil": visualise.PngWriter(), "device": visualise.DevicePngWriter(), "dynamic": visualise.DevicePngWriter(strategy="dynamic")}
    path = lambda route, name: os.path.join(tmp, "%s_%s.png" % (route, name))

    def pil():
        for name, t in pics:
            writers["pil"].write(t, path("pil", name))
        writers["pil"].drain()

    def on_device(route):
        def fn():
            writers[route].write_many([t for _, t in pics], [path(route, name) for name, _ in pics])
            writers[route].drain()
        return fn

    routes = {"pil": pil, "device": on_device("device"), "dynamic": on_device("dynamic")}
    seen = {}
    original = _capi.call
    for route in ("device", "dynamic"):
        seen[route] = []
        _capi.call = lambda entry, *a: (seen[route].append(entry), original(entry, *a))[1]
        try:
            routes[route]()
        finally:
            _capi.call = original
    for _ in range(3):
        for fn in routes.values():
            fn()
    t = {k: [] for k in routes}
    for _ in range(args.rounds):
        for k, fn in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            t[k].append((time.perf_counter() - t0) * 1e3)
    # the library call alone: device events around windows of 20 calls on a writer's own buffers, the two strategies window by window
    dw = writers["device"]
    slots = [dw._slot((int(t.shape[0]), int(t.shape[1]), int(t.shape[2])), t.device) for _, t in pics]
    calls = {}
    for route, strategy in (("device", 0), ("dynamic", 1)):
        a = calls[route] = _capi.PngEncodeArgs()
        a.struct_bytes, a.num_images = ctypes.sizeof(_capi.PngEncodeArgs), len(pics)
        for im, slot, (_, tensor) in zip(a.image, slots, pics):
            im.pixels, (im.H, im.W, im.C), im.strategy = _capi.ptr(tensor, torch.uint8), slot.key, strategy
            im.out, im.capacity = _capi.ptr(slot.out, torch.uint8), slot.bound
            im.length, im.workspace = _capi.ptr(slot.length, torch.int64), _capi.ptr(slot.workspace, torch.uint8)
    kernel_ms = {route: [] for route in calls}
    for _ in range(1 + 9):
        for route, a in calls.items():
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(20):
                _capi.call("hps_png_encode", ctypes.addressof(a), _capi.stream())
            stop.record()
            stop.synchronize()
            kernel_ms[route].append(start.elapsed_time(stop) / 20)
    kernel_ms = {route: np.percentile(v[1:], [0, 50, 100]) for route, v in kernel_ms.items()}
    for w in writers.values():
        w.close()
    q = {k: np.percentile(v, [25, 50, 75]) for k, v in t.items()}
    iqr = {k: q[k][2] - q[k][0] for k in q}
    sizes, same = [], True
    for name, tensor in pics:
        raw = tensor.cpu().numpy()
        a, b, c = (os.path.getsize(path(route, name)) for route in ("pil", "device", "dynamic"))
        same = same and all(np.array_equal(np.asarray(Image.open(path(route, name))), raw) for route in ("pil", "device", "dynamic"))
        sizes.append((name, tuple(raw.shape), raw.size, a, b, c))
    raw_total, dev_total, dyn_total = sum(s[2] for s in sizes), sum(s[4] for s in sizes), sum(s[5] for s in sizes)
    wins = {k: q[k][1] < q["pil"][1] - (iqr["pil"] + iqr[k]) for k in ("device", "dynamic")}
    launches = lambda route: "%s = %d launches" % (", ".join("%d x %s" % (seen[route].count(e), e) for e in sorted(set(seen[route]))), 2 * seen[route].count("hps_png_encode"))
    lines = ["Writing the three predict pictures of one image as PNG files on one MI355X (gfx950), visualise_wh = 512: tools/png_encode_time.py,",
             "commit: %s.  Host clock from the finished device pictures to drained files; %d rounds of each writer, alternating," % (args.commit, args.rounds),
             "after 3 warm-up rounds; median (quartiles).", "",
             "  PngWriter        (PIL, compress_level 1, four host threads)          %9.2f ms  (%.2f .. %.2f)" % (q["pil"][1], q["pil"][0], q["pil"][2]),
             "  DevicePngWriter  (hps_png_encode, strategy fixed, one call per image)   %6.2f ms  (%.2f .. %.2f)" % (q["device"][1], q["device"][0], q["device"][2]),
             "  DevicePngWriter  (hps_png_encode, strategy dynamic, one call per image) %6.2f ms  (%.2f .. %.2f)" % (q["dynamic"][1], q["dynamic"][0], q["dynamic"][2]), "",
             "  PngWriter / DevicePngWriter fixed, medians     %6.2f" % (q["pil"][1] / q["device"][1]),
             "  PngWriter / DevicePngWriter dynamic, medians   %6.2f" % (q["pil"][1] / q["dynamic"][1]),
             "  DevicePngWriter dynamic / fixed, medians       %6.2f" % (q["dynamic"][1] / q["device"][1]),
             "  a device writer's median is lower than PIL's by more than the sum of the two interquartile ranges: fixed (%.2f + %.2f ms) %s, dynamic (%.2f + %.2f ms) %s"
             % (iqr["pil"], iqr["device"], "yes" if wins["device"] else "NO", iqr["pil"], iqr["dynamic"], "yes" if wins["dynamic"] else "NO"), "",
             "libhps calls per image: fixed %s; dynamic %s" % (launches("device"), launches("dynamic")),
             "hps_png_encode alone, the three pictures in one call (device events around 20 calls, median of 9 windows, fastest .. slowest; the two",
             "strategies window by window): fixed %.3f ms (%.3f .. %.3f), dynamic %.3f ms (%.3f .. %.3f), dynamic / fixed %.2f"
             % (kernel_ms["device"][1], kernel_ms["device"][0], kernel_ms["device"][2], kernel_ms["dynamic"][1], kernel_ms["dynamic"][0], kernel_ms["dynamic"][2],
                kernel_ms["dynamic"][1] / kernel_ms["device"][1]),
             "bytes copied to the host per image: PngWriter %d (the raw pictures), DevicePngWriter fixed %d, dynamic %d (the files) + %d (their lengths)"
             % (raw_total, dev_total, dyn_total, 8 * len(sizes)), "",
             "file sizes in bytes (every file decodes to the picture's bytes: %s):" % ("yes" if same else "NO"),
             "  %-8s %-16s %10s %12s %12s %12s %14s %16s" % ("picture", "shape", "raw", "PIL level 1", "fixed", "dynamic", "dynamic / PIL", "dynamic / fixed")]
    for name, shape, raw, a, b, c in sizes:
        lines.append("  %-8s %-16s %10d %12d %12d %12d %14.2f %16.2f" % (name, "x".join(map(str, shape)), raw, a, b, c, c / a, c / b))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:                                   # appended: the file keeps the records of earlier commits
        f.write(("\n" if os.path.getsize(args.out) else "") + text)


if __name__ == "__main__":
    main()
