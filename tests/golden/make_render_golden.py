"""Pins the renderer's restatement (tests/render_scenario.py; include/hps.h: hps_render) against pytorch3d itself, wherever
pytorch3d is installed.  ONE command:

    python tests/golden/make_render_golden.py

renders the scenario's scenes through pytorch3d's own API -- Meshes, PerspectiveCameras / OrthographicCameras, RasterizationSettings
with the reference's defaults (run_train.py:86-91), MeshRasterizer, HardPhongShader, TexturesVertex / TexturesUV, PointLights, as
renderers/pytorch3d_textured_renderer.py:155-285 configures them -- and writes tests/golden/render_pytorch3d.npz, which
tests/test_render_pytorch3d_golden.py picks up; without the file that test skips.

pytorch3d has no ROCm build and is not installed where this project is built, so there this script stops at a clear message with
exit status 3, and the restatement's rules stay what they are: written from pytorch3d's rasteriser and shader sources, never run against
them.  Nothing of pytorch3d is vendored or stubbed: what is written is data produced by the installed package.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT_PATH = os.path.join(HERE, "render_pytorch3d.npz")
CASES = ("w16_f13_b1", "w40_f257_b3", "w64_f2400_b3_ortho", "w64_two_b1_vertex", "whole_image", "shared_edge", "coincident")

for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def render_with_pytorch3d(scene, device):
    import torch
    from pytorch3d.renderer import (HardPhongShader, MeshRasterizer, OrthographicCameras, PerspectiveCameras, PointLights,
                                    RasterizationSettings, TexturesUV, TexturesVertex, BlendParams)
    from pytorch3d.structures import Meshes
    B, W = scene.B, scene.W
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float().to(device)
    R = torch.tensor([[-1.0, 0.0, 0.0], [0.0, -1.0, 0.0], [0.0, 0.0, 1.0]], device=device)[None].expand(B, -1, -1)
    T = f(scene.cam_t).expand(B, 3) * torch.tensor([-1.0, -1.0, 1.0], device=device)
    scale = f(scene.scale).expand(B, 2)
    cam = PerspectiveCameras if scene.projection == "perspective" else OrthographicCameras
    cameras = cam(device=device, R=R, T=T, focal_length=scale * (W / 2.0), principal_point=((W / 2.0, W / 2.0),), image_size=((W, W),),
                  in_ndc=False)
    settings = RasterizationSettings(image_size=W, blur_radius=0.0, faces_per_pixel=1, bin_size=None, max_faces_per_bin=None,
                                     perspective_correct=False, cull_backfaces=False, clip_barycentric_coords=None)
    verts = f(scene.vertices)[:, torch.from_numpy(scene.verts_map).to(device)]
    faces = torch.from_numpy(scene.faces).to(device)[None].expand(B, -1, -1)
    iuv_mesh = Meshes(verts=verts, faces=faces, textures=TexturesVertex(verts_features=f(scene.verts_iuv)[None].expand(B, -1, -1)))
    if scene.verts_features is not None:
        tex = TexturesVertex(verts_features=f(scene.verts_features)[:, torch.from_numpy(scene.verts_map).to(device)])
    else:
        tex = TexturesUV(maps=f(scene.texture), faces_uvs=faces, verts_uvs=f(scene.verts_uv)[None].expand(B, -1, -1))
    rgb_mesh = Meshes(verts=verts, faces=faces, textures=tex)
    fragments = MeshRasterizer(cameras=cameras, raster_settings=settings)(iuv_mesh, cameras=cameras)
    blend = BlendParams(background_color=(0.0, 0.0, 0.0))
    flat = PointLights(device=device, ambient_color=[[1, 1, 1]], diffuse_color=[[0, 0, 0]], specular_color=[[0, 0, 0]])
    lights = PointLights(device=device, location=f(scene.lights["location"]), ambient_color=f(scene.lights["ambient_color"]),
                         diffuse_color=f(scene.lights["diffuse_color"]), specular_color=f(scene.lights["specular_color"]))
    iuv = HardPhongShader(device=device, cameras=cameras, lights=flat, blend_params=blend)(fragments, iuv_mesh, lights=flat)[..., :3]
    rgb = HardPhongShader(device=device, cameras=cameras, lights=lights, blend_params=blend)(fragments, rgb_mesh, lights=lights)[..., :3]
    pix = fragments.pix_to_face[..., 0]
    F = scene.faces.shape[0]
    local = torch.where(pix >= 0, pix % F, pix)                                      # packed face index -> the mesh's own
    return dict(pix_to_face=local.cpu().numpy(), zbuf=fragments.zbuf[..., 0].cpu().numpy(), bary=fragments.bary_coords[..., 0, :].cpu().numpy(),
                iuv=iuv.cpu().numpy(), rgb=torch.clamp(rgb, max=1.0).cpu().numpy())


def main():
    try:
        import pytorch3d  # noqa: F401
    except ImportError:
        print("pytorch3d is absent: tests/golden/render_pytorch3d.npz is not written, and tests/test_render_pytorch3d_golden.py skips.\n"
              "Run this script on a machine that has pytorch3d (CPU is enough).")
        return 3
    import torch
    import render_scenario as S
    device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    out = {}
    for name in CASES:
        for k, v in render_with_pytorch3d(S.reference(name)[0], device).items():
            out["%s/%s" % (name, k)] = v
    np.savez_compressed(OUT_PATH, **out)
    print("wrote", OUT_PATH)
    return 0


if __name__ == "__main__":
    sys.exit(main())
