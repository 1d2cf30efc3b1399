"""Time of the SSP-3D silhouette counts on one MI355X at an evaluation batch: M = 320 meshes (32 frames x 10 samples) of 13 774 faces over
7 829 DensePose vertices at 256 x 256, orthographic camera and target per frame (group = 10), rotation by pi about x on.

    python tests/dev/silhouette_time.py [--out profiles/silhouette_time.txt]
    python tests/dev/silhouette_time.py --only fused --rounds 20        # one route alone, for rocprofv3 --kernel-trace --stats

Two routes over the same inputs, in the same process, alternating round by round:
  fused     TexturedIUVRenderer.silhouette_counts (hps_silhouette_iou: four launches, no image)
  composed  what the package could do before it: the flip with a torch multiply, TexturedIUVRenderer.forward (render_rgb=False: IUV and
            depth images), round, != 0, the four logical combinations with the repeated targets and their sums.
Whole calls, host work included, HIP events around each; 5 warm-up rounds of both, then 100 timed rounds of each, the median and the
quartiles.  The time per launch comes from a rocprofv3 --kernel-trace --stats run of ``--only`` (a run of its own).  The two routes'
counts are compared before anything is timed.  Bytes are what each route has to move for the images alone,
from shapes: the composed route writes IUV and depth (16 bytes per pixel and mesh) and reads the I plane back; the fused one reads one
target byte per pixel and mesh and writes 16 bytes per 8 x 8 tile."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from hierarchicalprobabilistic3dhuman_amd import textured_renderer as tr  # noqa: E402
import render_scenario as S  # noqa: E402


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "silhouette_time.txt"))
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--samples", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=100)
    ap.add_argument("--only", choices=("fused", "composed"), default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    frames, N, W = args.frames, args.samples, 256
    M = frames * N
    scene = S.make_scene(**dict(S.CASES["w256_smpl_b2"], projection="orthographic"))
    Nd, F = scene.Nd, len(scene.faces)
    cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    vertices = cuda(scene.vertices).repeat((M + 1) // 2, 1, 1)[:M].contiguous()       # the two meshes of the case, alternating
    dp = (torch.from_numpy(scene.verts_uv)[None], torch.from_numpy(scene.verts_iuv)[None], torch.from_numpy(scene.verts_map), torch.from_numpy(scene.faces)[None])
    renderer = tr.TexturedIUVRenderer("cuda", M, img_wh=W, projection_type="orthographic", render_rgb=False, densepose_uv=dp)
    g = torch.Generator().manual_seed(3)
    cam_t = torch.cat([0.05 * torch.randn(frames, 2, generator=g), torch.full((frames, 1), 2.5)], dim=1).cuda()
    scale = torch.empty(frames, 1).uniform_(0.8, 1.0, generator=g).expand(-1, 2).contiguous().cuda()
    rr, cc = np.indices((W, W))
    target = cuda(np.stack([(((rr - 128 - 3 * (k % 5)) / 90.0) ** 2 + ((cc - 128 + 2 * (k % 7)) / 70.0) ** 2 <= 1) for k in range(frames)]).astype(np.uint8))
    flip = torch.tensor([1.0, -1.0, -1.0], device="cuda")

    def fused():
        return renderer.silhouette_counts(vertices, target, cam_t=cam_t, orthographic_scale=scale, group=N, flip=True)

    def composed():
        out = renderer(vertices=vertices * flip, cam_t=cam_t.repeat_interleave(N, dim=0), orthographic_scale=scale.repeat_interleave(N, dim=0))
        pred = out["iuv_images"][..., 0].round() != 0
        tgt = (target != 0).repeat_interleave(N, dim=0)
        return torch.stack([(pred & tgt).sum(dim=(1, 2)), (pred & ~tgt).sum(dim=(1, 2)), (~pred & ~tgt).sum(dim=(1, 2)),
                            (~pred & tgt).sum(dim=(1, 2))], dim=1)

    if args.only:
        with torch.no_grad():
            for _ in range(args.rounds):
                (fused if args.only == "fused" else composed)()
        torch.cuda.synchronize()
        return
    with torch.no_grad():
        a, b = fused().cpu().numpy().astype(np.int64), composed().cpu().numpy()
        same = bool(np.array_equal(a, b))
        for _ in range(5):
            fused()
            composed()
        torch.cuda.synchronize()
        t = {"fused": [], "composed": []}
        for _ in range(args.rounds):
            t["fused"].append(once(fused))
            t["composed"].append(once(composed))
    q = {k: np.percentile(v, [25, 50, 75]) for k, v in t.items()}
    image_bytes = M * W * W * 16.0
    composed_bytes = image_bytes + M * W * W * 4.0
    fused_bytes = M * W * W * 1.0 + M * (W // 8) ** 2 * 16.0
    lines = ["Silhouette counts on one MI355X (gfx950): M = %d meshes (%d frames x %d samples) of %d faces over %d DensePose vertices at" % (M, frames, N, F, Nd),
             "%d x %d, orthographic, group = %d, flip on; the two meshes of tests/render_scenario.py's w256_smpl_b2 repeated; %d set pixels" % (W, W, N, int(a[:, :2].sum())),
             "(%.1f %% of the images).  tests/dev/silhouette_time.py: whole calls, host work included, HIP events, %d rounds of each route," % (100.0 * a[:, :2].sum() / (M * W * W), args.rounds),
             "alternating; median (quartiles).", "",
             "  composed: torch flip, forward(render_rgb=False), round, != 0, logical ops, sums   %9.3f ms  (%.3f .. %.3f)" % (q["composed"][1], q["composed"][0], q["composed"][2]),
             "  fused: silhouette_counts (hps_silhouette_iou, four launches)                      %9.3f ms  (%.3f .. %.3f)" % (q["fused"][1], q["fused"][0], q["fused"][2]),
             "  composed / fused                                                                  %9.2f" % (q["composed"][1] / q["fused"][1]),
             "  counts of the two routes equal: %s" % same, "",
             "image traffic from shapes: composed writes IUV + depth (%.1f MB) and reads the I plane back (%.1f MB) = %.1f MB;" % (image_bytes / 1e6, M * W * W * 4.0 / 1e6, composed_bytes / 1e6),
             "fused reads the target bytes and writes the tile counts = %.1f MB (1 / %.0f); the %.1f MB image buffers are not allocated." % (fused_bytes / 1e6, composed_bytes / fused_bytes, image_bytes / 1e6)]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
