"""Times of the training renderer (train/train_poseMF_shapeGaussian_net.py:186-196) on one MI355X at the reference's batch: B = 72
images of 256 x 256, an SMPL-sized mesh of 13 774 faces over 7 829 DensePose vertices, 1200 x 800 textures, default kernels.
textured_renderer.TexturedIUVRenderer.render_train_inputs beside the restatement of tests/render_scenario.py written with torch
operations on the device (``torch_route`` below: every face tested at every pixel, 32 faces at a time -- pytorch3d itself cannot be
installed here, and the parent commit has no renderer), in the same process, on the same scene.

    python tests/dev/render_time.py [--out profiles/render_time.txt] [--kernel-stats <rocprofv3 kernel stats csv>]
    python tests/dev/render_time.py --only-render 10            # the device route alone, for rocprofv3 --kernel-trace --stats

Whole calls: HIP events around the call, host work included; 3 warm-up rounds and the median of 10 rounds for the device route, 1 and 3
for the torch route (seconds per round).  hps_render issues its three launches from one library call, so the time per launch comes
from a rocprofv3 --kernel-trace --stats run of ``--only-render`` (a run of its own), given back with --kernel-stats.  Bytes are what
the algorithm needs, from shapes, every tensor counted once and whole (the texture too, of which a render samples a part)."""
import argparse
import csv
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from hierarchicalprobabilistic3dhuman_amd import textured_renderer as tr  # noqa: E402
import render_scenario as S  # noqa: E402

HBM_PEAK = 8.0e12
STEP_MS = 49.6                   # the training step without a renderer
med = lambda v: sorted(v)[len(v) // 2]


def timed(fn, warmup, rounds):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return med(out)


def _normalise(v):
    n = torch.sqrt(v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2])
    return v / torch.clamp(n, min=S.NORM_EPS)[..., None]


def _interp(w, attr):
    return w[..., 0, None] * attr[..., 0, :] + w[..., 1, None] * attr[..., 1, :] + w[..., 2, None] * attr[..., 2, :]


def torch_route(d, W, chunk=32):
    """tests/render_scenario.py's render with torch operations on d's device: d holds the scene's arrays as tensors (faces, verts_map
    int64).  Returns (pix_to_face (B,W,W), zbuf, iuv (B,W,W,3), rgb)."""
    v = d["vertices"][:, d["verts_map"]]
    B, Nd = v.shape[:2]
    dt, dev = v.dtype, v.device
    t, s = d["cam_t"].expand(B, 3), d["scale"].expand(B, 2)
    X, Y, Z = -(v[..., 0] + t[:, None, 0]), -(v[..., 1] + t[:, None, 1]), v[..., 2] + t[:, None, 2]
    xn, yn = s[:, None, 0] * X, s[:, None, 1] * Y
    if d["perspective"]:
        xn, yn = xn / Z, yn / Z
    faces = d["faces"]
    F = faces.shape[0]
    pix = 1 - (2 * torch.arange(W, device=dev) + 1).to(dt) / W
    px, py = pix[None, None, None, :], pix[None, None, :, None]
    zbuf = torch.full((B, W, W), float("inf"), device=dev, dtype=dt)
    face = torch.full((B, W, W), -1, device=dev, dtype=torch.int64)
    inf = torch.tensor(float("inf"), device=dev, dtype=dt)
    for f0 in range(0, F, chunk):
        fc = faces[f0:f0 + chunk]
        x, y, z = (q[:, fc][:, :, :, None, None] for q in (xn, yn, Z))              # (B,C,3,1,1)
        area = (x[:, :, 2] - x[:, :, 0]) * (y[:, :, 1] - y[:, :, 0]) - (y[:, :, 2] - y[:, :, 0]) * (x[:, :, 1] - x[:, :, 0])
        keep = ~(area.abs() <= S.EPS) & ~(z.amax(dim=2) < S.EPS)
        den = area + S.EPS
        w0 = ((px - x[:, :, 1]) * (y[:, :, 2] - y[:, :, 1]) - (py - y[:, :, 1]) * (x[:, :, 2] - x[:, :, 1])) / den
        w1 = ((px - x[:, :, 2]) * (y[:, :, 0] - y[:, :, 2]) - (py - y[:, :, 2]) * (x[:, :, 0] - x[:, :, 2])) / den
        w2 = ((px - x[:, :, 0]) * (y[:, :, 1] - y[:, :, 0]) - (py - y[:, :, 0]) * (x[:, :, 1] - x[:, :, 0])) / den
        pz = w0 * z[:, :, 0] + w1 * z[:, :, 1] + w2 * z[:, :, 2]
        ok = (w0 > 0) & (w1 > 0) & (w2 > 0) & ~(pz < 0) & keep
        pz = torch.where(ok, pz, inf)
        zmin = pz.amin(dim=1)
        idx = torch.arange(f0, f0 + fc.shape[0], device=dev)[None, :, None, None]
        first = torch.where(pz == zmin[:, None], idx, F).amin(dim=1)                 # the lowest face index among equal depths
        better = zmin < zbuf
        zbuf = torch.where(better, zmin, zbuf)
        face = torch.where(better, first, face)
    covered = face >= 0
    corners = faces[face.clamp(min=0)]                                              # (B,W,W,3)
    bi = torch.arange(B, device=dev)[:, None, None, None]
    x, y, z = xn[bi, corners], yn[bi, corners], Z[bi, corners]
    px, py = pix[None, None, :], pix[None, :, None]
    den = (x[..., 2] - x[..., 0]) * (y[..., 1] - y[..., 0]) - (y[..., 2] - y[..., 0]) * (x[..., 1] - x[..., 0]) + S.EPS
    w = torch.stack([((px - x[..., 1]) * (y[..., 2] - y[..., 1]) - (py - y[..., 1]) * (x[..., 2] - x[..., 1])) / den,
                     ((px - x[..., 2]) * (y[..., 0] - y[..., 2]) - (py - y[..., 2]) * (x[..., 0] - x[..., 2])) / den,
                     ((px - x[..., 0]) * (y[..., 1] - y[..., 0]) - (py - y[..., 0]) * (x[..., 1] - x[..., 0])) / den], dim=-1)
    # vertex normals: index_add_ over the corners (its order of addition is the library's, not the table's: a timing yardstick)
    v0, v1, v2 = (v[:, faces[:, k]] for k in range(3))
    cross = torch.cross(v1 - v0, v2 - v0, dim=-1)
    normals = torch.zeros_like(v)
    for k in range(3):
        normals.index_add_(1, faces[:, k], cross)
    normals = _normalise(normals)
    iuv = _interp(w, d["verts_iuv"][corners])
    uv = _interp(w, d["verts_uv"][corners])
    tex = d["texture"]
    Ht, Wt = tex.shape[1:3]
    tx = torch.clamp(uv[..., 0] * (Wt - 1), 0, Wt - 1)
    ty = torch.clamp((1 - uv[..., 1]) * (Ht - 1), 0, Ht - 1)
    xf, yf = torch.floor(tx), torch.floor(ty)
    x0, y0 = xf.long(), yf.long()
    x1, y1 = torch.clamp(x0 + 1, max=Wt - 1), torch.clamp(y0 + 1, max=Ht - 1)
    fx, fy = (tx - xf)[..., None], (ty - yf)[..., None]
    b3 = bi[..., 0]
    lerp = lambda p, q, a: p + a * (q - p)
    texel = lerp(lerp(tex[b3, y0, x0], tex[b3, y0, x1], fx), lerp(tex[b3, y1, x0], tex[b3, y1, x1], fx), fy)
    n = _normalise(_interp(w, normals[bi, corners]))
    P = _interp(w, v[bi, corners])
    light = [d[k].expand(B, 3)[:, None, None, :] for k in ("location", "ambient_color", "diffuse_color", "specular_color")]
    L = _normalise(light[0] - P)
    view = _normalise(-t[:, None, None, :] - P)
    nl = (n * L).sum(-1)
    reflect = -L + 2 * nl[..., None] * n
    sp = torch.clamp((view * reflect).sum(-1), min=0) * (nl > 0).to(dt)
    for _ in range(6):
        sp = sp * sp
    rgb = torch.clamp((light[1] + light[2] * torch.clamp(nl, min=0)[..., None]) * texel + light[3] * sp[..., None], max=1.0)
    zero = torch.zeros((), device=dev, dtype=dt)
    return (face, torch.where(covered, zbuf, -torch.ones((), device=dev, dtype=dt)), torch.where(covered[..., None], iuv, zero),
            torch.where(covered[..., None], rgb, zero))


def scene_tensors(scene, device, dtype=torch.float32):
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dtype)
    d = dict(vertices=f(scene.vertices), verts_map=torch.from_numpy(scene.verts_map).to(device), faces=torch.from_numpy(scene.faces).to(device),
             cam_t=f(scene.cam_t), scale=f(scene.scale), perspective=scene.projection == "perspective", verts_iuv=f(scene.verts_iuv),
             verts_uv=f(scene.verts_uv), texture=f(scene.texture))
    d.update({k: f(v) for k, v in scene.lights.items()})
    return d


def kernel_stats(path):
    """kernel name -> (calls, average ns) from a rocprofv3 --kernel-trace --stats kernel_stats.csv."""
    out = {}
    with open(path) as fh:
        for row in csv.DictReader(fh):
            name = row.get("Name") or row.get("KernelName") or ""
            for key in ("render_project_kernel", "render_setup_kernel", "render_raster_kernel"):
                if key in name:
                    out[key] = (int(row["Calls"]), float(row["AverageNs"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_time.txt"))
    ap.add_argument("--batch", type=int, default=72)
    ap.add_argument("--only-render", type=int, default=0)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--torch-chunk", type=int, default=32)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    B, W = args.batch, 256
    scene = S.make_scene(seed=7, B=B, W=W, rings=83, segments=83, num_faces=13774, duplicates=938.0 / 6891.0, tex_hw=(1200, 800))
    Nd, F, V = scene.Nd, len(scene.faces), scene.V
    d = scene_tensors(scene, "cuda")
    dp = (d["verts_uv"][None].cpu(), d["verts_iuv"][None].cpu(), torch.from_numpy(scene.verts_map), torch.from_numpy(scene.faces)[None])
    renderer = tr.TexturedIUVRenderer("cuda", B, img_wh=W, perspective_focal_length=300.0, render_rgb=True, densepose_uv=dp)
    lights = {k: d[k] for k in ("location", "ambient_color", "diffuse_color", "specular_color")}
    new_route = lambda: renderer.render_train_inputs(vertices=d["vertices"], textures=d["texture"], cam_t=d["cam_t"], lights_rgb_settings=lights)
    if args.only_render:
        for _ in range(args.only_render):
            new_route()
        torch.cuda.synchronize()
        return
    t_new = timed(new_route, 3, 10)
    iuv_in, rgb_in = new_route()
    with torch.no_grad():
        t_torch = timed(lambda: torch_route(d, W, args.torch_chunk), 1, 3)
        face, zbuf, iuv, rgb = torch_route(d, W, args.torch_chunk)
    covered = int((face >= 0).sum())
    same = float(((iuv_in.permute(0, 2, 3, 1)[..., 0] - torch.round(iuv[..., 0])).abs() < 0.5).float().mean())
    rgb_err = float((rgb_in.permute(0, 2, 3, 1) - rgb).abs().max())
    out_bytes = B * W * W * (3 + 3 + 3 + 1) * 4.0
    nbytes = {"render_project_kernel": B * Nd * (12 + 32.0) + Nd * 4,
              "render_setup_kernel": B * Nd * (16 + 16 + 16.0) + (F * 3 + 3 * F + Nd + 1) * 4 + B * F * 8.0,
              "render_raster_kernel": B * F * 8.0 + F * 12 + B * Nd * 48.0 + Nd * 20 + B * 1200 * 800 * 12.0 + out_bytes}
    lines = ["The training renderer on one MI355X (gfx950): B = %d images of %d x %d, %d faces over %d DensePose / %d mesh vertices," % (B, W, W, F, Nd, V),
             "1200 x 800 textures, perspective camera, one shared light; scene of tests/render_scenario.py (seed 7), %d covered pixels" % covered,
             "(%.1f %% of the images).  tests/dev/render_time.py: HIP events, medians.  Outputs: rounded IUV, IUV, RGB, depth." % (100.0 * covered / (B * W * W)), "",
             "whole call, vertices -> (iuv_in, rgb_in), host work included:",
             "  restatement with torch operations on the device (%d faces at a time; 3 rounds)  %10.2f ms" % (args.torch_chunk, t_torch),
             "  TexturedIUVRenderer.render_train_inputs (3 launches; 10 rounds)                 %10.3f ms   = 1 / %.0f of the torch route" % (t_new, t_torch / t_new),
             "  share of the %.1f ms training step (DESIGN.md section 8)                        %10.1f %%" % (STEP_MS, 100.0 * t_new / STEP_MS),
             "  agreement of the two routes: part label equal on %.4f of the pixels, max |rgb difference| %.2e" % (same, rgb_err), ""]
    if args.kernel_stats:
        lines.append("launches (rocprofv3 --kernel-trace --stats of --only-render, average per call; bytes as whole tensors):")
        for name, (calls, ns) in kernel_stats(args.kernel_stats).items():
            nb = nbytes[name]
            lines.append("  %-24s %5d calls %9.4f ms   %9.2f MB   %6.3f TB/s = %.4f of 8 TB/s"
                         % (name, calls, ns * 1e-6, nb / 1e6, nb / (ns * 1e-9) / 1e12, nb / (ns * 1e-9) / HBM_PEAK))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
