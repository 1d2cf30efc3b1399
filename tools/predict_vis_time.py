"""Time per image of the three predict pictures at visualise_wh = 512 on one MI355X: the eight-panel figure, the body over a 720 x 960
photograph and the 3 x 6 sample sheet, from an SMPL-sized mesh (13 774 faces over 7 829 DensePose vertices, tests/render_scenario.py's
w256_smpl_b2 at 512 x 512, orthographic), a 256 x 256 crop and proxy representation, 12 samples.

    python tools/predict_vis_time.py [--out profiles/predict_vis_time.txt] [--commit ID] [--keep DIR]

Two routes over the same inputs, in one process, alternating round by round, each with and without the PNG encode:
  device     visualise.PredictVisualiser: per picture one hps_vis_views, one hps_render over all views, one hps_vis_compose (and one
             hps_vis_uncrop); bytes to page-locked memory; PIL on PngWriter's four threads, drained at the end of the image.
  composed   the same pictures put together the reference's way (predict/predict_poseMF_shapeGaussian_net.py:187-333) from this package's
             own pieces: one TexturedIUVRenderer.forward() per view (fourteen, plus eighteen for the sheet), the flips as torch matrix
             products, batch_add_rgb_background, F.interpolate, a .cpu().numpy() copy of every float image, numpy tiling and rounding,
             PIL encodes one after the other.  Where the reference calls cv2.warpAffine (not available) it uses F.grid_sample with the
             same affine map.  This route is the yardstick.
Whole images, host work included: a host clock around work that ends in a device synchronise (the composed route is mostly host work).
3 warm-up rounds of everything, then ``--rounds`` timed rounds of each; median and quartiles.  libhps calls are counted by wrapping
_capi.call (hps_render is three launches, every hps_vis_* one; torch's own launches are not counted)."""
import argparse
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from hierarchicalprobabilistic3dhuman_amd import _capi, configs, textured_renderer as tr, visualise  # noqa: E402
from hierarchicalprobabilistic3dhuman_amd.image_utils import batch_add_rgb_background  # noqa: E402
from hierarchicalprobabilistic3dhuman_amd.sampling_utils import joints2D_error_sorted_verts_sampling  # noqa: E402
import render_scenario as S  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predict_vis_time.txt"))
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--commit", default="working tree")
    ap.add_argument("--keep", default=None, help="directory that keeps one image's pictures of both routes")
    ap.add_argument("--tmp", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    from PIL import Image
    dev = torch.device("cuda", torch.cuda.current_device())
    wh, D, H, W, N = 512, 256, 720, 960, 12
    cfg = configs.get_cfg_defaults()
    scene = S.make_scene(**dict(S.CASES["w256_smpl_b2"], W=wh, projection="orthographic"))
    dp = (torch.from_numpy(scene.verts_uv)[None], torch.from_numpy(scene.verts_iuv)[None], torch.from_numpy(scene.verts_map), torch.from_numpy(scene.faces)[None])
    make = lambda: tr.TexturedIUVRenderer(dev, 1, img_wh=wh, projection_type="orthographic", render_rgb=True, densepose_uv=dp)
    vis = visualise.PredictVisualiser(make(), cfg, wh)
    one = make()                                                                       # the composed route's renderer, one view per call
    g = torch.Generator().manual_seed(7)
    flip = torch.tensor([1.0, -1.0, -1.0])
    V = scene.V
    mode = torch.from_numpy(scene.vertices[0]) * flip                                  # upright after the pictures' own flip
    result = {"verts_mode": mode.to(dev), "verts_tpose": (torch.from_numpy(scene.vertices[1]) * flip).to(dev),
              "unc": (0.25 * torch.rand(V, generator=g)).to(dev), "cam": torch.tensor([0.9, 0.0, 0.2], device=dev),
              "verts_samples": (mode[None] + 0.02 * torch.randn(N, V, 3, generator=g)).to(dev),
              "joints_samples": (0.4 * torch.randn(N, 90, 3, generator=g)).to(dev)}
    smooth = lambda c, h, w: F.interpolate(torch.rand(1, c, h // 16, w // 16, generator=g), size=(h, w), mode="bilinear", align_corners=False)
    crop = smooth(3, D, D).to(dev)                                                     # smooth like a photograph: noise would not compress
    proxy = ((torch.rand(1, 18, D, D, generator=g) < 0.05).float() * 0.5).to(dev)
    joints2D = (torch.rand(1, 17, 2, generator=g) * D).to(dev)
    photo = (smooth(3, H, W)[0].permute(1, 2, 0) * 255).to(torch.uint8).contiguous()
    image = (photo.permute(2, 0, 1).float() / 255.0).to(dev)
    centre, side = torch.tensor([380.0, 470.0], device=dev), torch.tensor([560.0], device=dev)
    import tempfile
    tmp = args.tmp or args.keep or tempfile.mkdtemp(prefix="predict_vis_time_")
    os.makedirs(tmp, exist_ok=True)
    writer = visualise.PngWriter()
    lights = vis.lights
    fixed_t, fixed_s = torch.tensor([vis.fixed_cam_t], device=dev), torch.tensor([[vis.fixed_scale] * 2], device=dev)
    lut = vis.lut
    Rx = torch.diag(torch.tensor([1.0, -1.0, -1.0])).to(dev)
    Ry = torch.tensor([[0.0, 0.0, -1.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0]], device=dev)

    def device(encode, tag="device"):
        fig = vis.figure(result, crop, proxy, joints2D)
        if encode:
            writer.write(fig, os.path.join(tmp, tag + ".png"))
        un = vis.uncropped(image, centre, side)
        if encode:
            writer.write(un, os.path.join(tmp, tag + "_uncrop.png"))
        sheet = vis.samples_figure(result, crop, proxy)
        if encode:
            writer.write(sheet, os.path.join(tmp, tag + "_samples.png"))
            writer.drain()
        torch.cuda.synchronize()

    def save(arr, path, encode):
        u8 = np.clip(np.rint(arr * 255.0), 0, 255).astype(np.uint8)                    # cv2.imwrite of a float image
        if encode:
            Image.fromarray(u8).save(path, format="PNG", compress_level=1)
        return u8

    def composed(encode, tag="composed"):
        cam = result["cam"][None]
        scale, cam_t = cam[:, [0, 0]], torch.cat([cam[:, 1:], torch.full((1, 1), 2.5, device=dev)], dim=-1)
        v0 = result["verts_mode"][None] @ Rx.T
        v90 = v0 @ Ry.T
        v180 = v90 @ Ry.T
        v270 = v180 @ Ry.T
        t0 = result["verts_tpose"][None] @ Rx.T
        t90 = t0 @ Ry.T
        idx = (result["unc"].double().clamp(0.0, 0.2) / 0.2 * 256.0).long().clamp(max=255)
        colours = lut[idx][None]
        plain = torch.full((1, V, 3), 0.7, device=dev)
        render = lambda v, c, t, s: one(vertices=v, cam_t=t, orthographic_scale=s, lights_rgb_settings=lights, verts_features=c)
        out = render(v0, colours, cam_t, scale)
        body_rgb_planar = out["rgb_images"].permute(0, 3, 1, 2).contiguous().clone()     # the renderer's buffers are reused by the next call
        body_iuv_planar = out["iuv_images"].permute(0, 3, 1, 2).contiguous().clone()
        crop_big = F.interpolate(crop, size=(wh, wh), mode="bilinear", align_corners=False)
        body = batch_add_rgb_background(crop_big, body_rgb_planar, body_iuv_planar[:, 0].round()).cpu().numpy()[0].transpose(1, 2, 0)
        side_views = [render(v, c, fixed_t, fixed_s)["rgb_images"].cpu().numpy()[0]
                      for v, c in ((v90, colours), (v180, colours), (v270, colours), (t0, plain), (t90, plain))]
        fig = np.zeros((2 * wh, 4 * wh, 3), dtype=np.float32)
        fig[:wh, :wh] = crop_big.cpu().numpy()[0].transpose(1, 2, 0)
        p = F.interpolate(proxy[:, :].sum(dim=1, keepdim=True), size=(wh, wh), mode="bilinear", align_corners=False)[0, 0].cpu().numpy()
        p = np.stack([p] * 3, axis=-1)
        rr, cc = np.indices((wh, wh))
        for x, y in joints2D[0].cpu().numpy().astype(np.float64):
            p[(cc - int(x * wh / D)) ** 2 + (rr - int(y * wh / D)) ** 2 <= 9] = (255.0, 0.0, 0.0)
        fig[wh:, :wh] = p
        fig[:wh, wh:2 * wh], fig[wh:, wh:2 * wh], fig[:wh, 2 * wh:3 * wh], fig[wh:, 2 * wh:3 * wh] = body, side_views[0], side_views[1], side_views[2]
        fig[:wh, 3 * wh:], fig[wh:, 3 * wh:] = side_views[3], side_views[4]
        save(fig, os.path.join(tmp, tag + ".png"), encode)
        # the body over the photograph: utils/image_utils.py:197-201's map, sampled by F.grid_sample in place of cv2.warpAffine
        m = side / wh
        tx, ty = centre[1] - m * (wh * 0.5), centre[0] - m * (wh * 0.5)
        gx = ((torch.arange(W, device=dev) - tx) / m + 0.5) / wh * 2 - 1
        gy = ((torch.arange(H, device=dev) - ty) / m + 0.5) / wh * 2 - 1
        grid = torch.stack([gx[None, :].expand(H, W), gy[:, None].expand(H, W)], dim=-1)[None]
        un_rgb = F.grid_sample(body_rgb_planar, grid, mode="bilinear", padding_mode="zeros", align_corners=False).cpu().numpy()[0].transpose(1, 2, 0)
        un_seg = F.grid_sample(body_iuv_planar[:, :1], grid, mode="nearest", padding_mode="zeros", align_corners=False).cpu().numpy()[0, 0]
        back = (un_seg == 0)[:, :, None]
        un = un_rgb * 255 * np.logical_not(back) + photo.numpy() * back
        save(un / 255.0, os.path.join(tmp, tag + "_uncrop.png"), encode)
        # the sample sheet
        best = joints2D_error_sorted_verts_sampling(result["verts_samples"], result["joints_samples"], proxy[:, 1:], cam)[:8]
        s0 = torch.cat([v0, best @ Rx.T], dim=0)
        s90 = torch.cat([v90, (best @ Rx.T) @ Ry.T], dim=0)
        sheet = np.zeros((3 * wh, 6 * wh, 3), dtype=np.float32)
        for i in range(9):
            o = render(s0[[i]], plain, cam_t, scale)
            front = batch_add_rgb_background(crop_big, o["rgb_images"].permute(0, 3, 1, 2).contiguous(), o["iuv_images"][:, :, :, 0].round())
            front = front.cpu().numpy()[0].transpose(1, 2, 0)
            beside = render(s90[[i]], plain, fixed_t, fixed_s)["rgb_images"].cpu().numpy()[0]
            for k, img in ((2 * i, front), (2 * i + 1, beside)):
                sheet[(k // 6) * wh:(k // 6 + 1) * wh, (k % 6) * wh:(k % 6 + 1) * wh] = img
        save(sheet, os.path.join(tmp, tag + "_samples.png"), encode)
        torch.cuda.synchronize()

    routes = {"device": lambda: device(False), "device + PNG": lambda: device(True),
              "composed": lambda: composed(False), "composed + PNG": lambda: composed(True)}
    # libhps calls per image
    calls = {}
    original = _capi.call
    for name in ("device", "composed"):
        seen = []
        _capi.call = lambda entry, *a, _seen=seen: (_seen.append(entry), original(entry, *a))[1]
        try:
            with torch.no_grad():
                routes[name]()
        finally:
            _capi.call = original
        calls[name] = seen
    with torch.no_grad():
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
        if args.keep:
            device(True)
            composed(True)
    # the two routes' pictures, compared: bytes that differ by more than 1
    with torch.no_grad():
        device(True, "cmp_device")
        composed(True, "cmp_composed")
    diffs = []
    for suffix in ("", "_uncrop", "_samples"):
        a = np.asarray(Image.open(os.path.join(tmp, "cmp_device%s.png" % suffix))).astype(np.int64)
        b = np.asarray(Image.open(os.path.join(tmp, "cmp_composed%s.png" % suffix))).astype(np.int64)
        diffs.append("%s %.4f %%" % (suffix or "figure", 100.0 * float((np.abs(a - b) > 1).mean())))
    writer.close()
    q = {k: np.percentile(v, [25, 50, 75]) for k, v in t.items()}
    count = lambda seen: ", ".join("%d x %s" % (seen.count(e), e) for e in sorted(set(seen)))
    launches = lambda seen: sum(3 if e == "hps_render" else 1 for e in seen)
    lines = ["The three predict pictures per image on one MI355X (gfx950), visualise_wh = %d: figure (2 x 4), body over a %d x %d photograph," % (wh, H, W),
             "sample sheet (3 x 6); %d faces over %d DensePose vertices, %d samples.  tools/predict_vis_time.py, commit: %s." % (len(scene.faces), scene.Nd, N, args.commit),
             "Whole images, host work included, host clock to a device synchronise; %d rounds of each route, alternating; median (quartiles)." % args.rounds, ""]
    for k in routes:
        lines.append("  %-16s %9.2f ms  (%.2f .. %.2f)" % (k, q[k][1], q[k][0], q[k][2]))
    lines += ["", "  composed / device, without the encode   %6.2f" % (q["composed"][1] / q["device"][1]),
              "  composed / device, with the encode      %6.2f" % (q["composed + PNG"][1] / q["device + PNG"][1]),
              "  the encode's share of the device route  %6.1f %%  (three PNG files, compress_level 1, on four threads)" % (100.0 * (1 - q["device"][1] / q["device + PNG"][1])), "",
              "libhps calls per image, device route (%d launches): %s" % (launches(calls["device"]), count(calls["device"])),
              "libhps calls per image, composed route (%d launches): %s" % (launches(calls["composed"]), count(calls["composed"])),
              "(hps_render is three launches, the others one; torch's own launches -- the ranking's sort and gather in both routes, the",
              "composed route's matrix products, interpolations, grid samples and device-to-host copies -- are not counted)", "",
              "bytes of the two routes' pictures that differ by more than 1: " + ", ".join(diffs),
              "(the composed route samples the un-crop with F.grid_sample, not with warpAffine's fixed-point positions)"]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
