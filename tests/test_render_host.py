"""The training renderer without a GPU: the C ABI's new entry points (exported, prototyped, refusing bad arguments before any
launch), the restatement (tests/render_scenario.py) on closed-form scenes whose arithmetic is exact, the DensePose pre-processing on a
synthetic dict, and the samplers' draws against the reference's formulas.

Closed-form scenes: an orthographic camera of scale 1 and vertices at multiples of 1/4 in NDC on an 8 x 8 image, whose pixel centres
are odd multiples of 1/8 -- every edge function is a dyadic number float32 holds exactly, so a sign is never a rounding decision."""
import ctypes

import numpy as np
import pytest
import torch

import render_scenario as S
from hierarchicalprobabilistic3dhuman_amd import _capi, configs, textured_renderer as tr

NEW_SYMBOLS = ("hps_render", "hps_sizeof_render_args")


def test_render_entry_points_are_exported_and_prototyped():
    """Fails without the feature."""
    lib = ctypes.CDLL(_capi.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), "libhps.so does not export %s" % name
        assert name in _capi.EXPORTED_SYMBOLS
    lib = _capi.load()
    assert lib.hps_version() == 502
    assert lib.hps_sizeof_render_args() == ctypes.sizeof(_capi.RenderArgs)
    # world, NDC and normal as 16-byte records per (image, vertex); a box of two words per face and per chunk of 64 faces
    assert _capi.query_workspace(_capi.WS_RENDER, 72, 7829, 13774) == 72 * (7829 * 48 + 13774 * 8 + 216 * 8)
    assert _capi.query_workspace(_capi.WS_RENDER, 1, 4, 257) == 4 * 48 + 257 * 8 + 5 * 8
    assert lib.hps_query_workspace(7, 64, 0, 0) == -1 and lib.hps_query_workspace(99, 1, 1, 1) == -1


def _args(**over):
    fake = ctypes.c_void_p(64)
    a = _capi.RenderArgs()
    a.struct_bytes = ctypes.sizeof(_capi.RenderArgs)
    a.B, a.H, a.W, a.num_verts, a.num_dp_verts, a.num_faces = 1, 16, 16, 4, 4, 2
    a.projection, a.tex_h, a.tex_w, a.cam_t_stride, a.scale_stride = _capi.RENDER_PERSPECTIVE, 2, 2, 3, 0
    for name in ("vertices", "verts_map", "faces", "vf_offsets", "vf_faces", "verts_iuv", "verts_uv", "cam_t", "scale", "light_location",
                 "ambient", "diffuse", "specular", "texture", "workspace", "iuv", "rgb", "depth"):
        setattr(a, name, fake)
    for k, v in over.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("over,message", [
    (dict(struct_bytes=8), b"struct_bytes"),
    (dict(vertices=None), b"null pointer"),
    (dict(workspace=None), b"null pointer"),
    (dict(H=16, W=24), b"square"),
    (dict(B=0), b"B in"),
    (dict(H=8192, W=8192), b"W in"),
    (dict(num_faces=0), b"num_faces"),
    (dict(projection=2), b"projection"),
    (dict(cam_t_stride=4), b"cam_t_stride"),
    (dict(iuv=None, rgb=None, depth=None), b"no output"),
    (dict(light_location=None), b"lights"),
    (dict(texture=None), b"texture"),
    (dict(tex_w=0), b"texture sides"),
    (dict(workspace=ctypes.c_void_p(72)), b"16-byte"),
])
def test_render_refuses_bad_arguments_before_any_launch(over, message):
    """Every pointer here is a fake: a call that got as far as a launch would not return -1."""
    lib = _capi.load()
    assert lib.hps_render(None, None) == -1 and b"null pointer" in lib.hps_last_error()
    a = _args(**over)
    assert lib.hps_render(ctypes.addressof(a), None) == -1
    assert message in lib.hps_last_error(), lib.hps_last_error()


def test_renderer_refuses_other_settings_and_the_cpu():
    uv = S.flat_scene(8, S.ndc_vertices([(-1, -1, 1), (1, -1, 1), (1, 1, 1)]), [(0, 1, 2)])
    dp = (torch.from_numpy(uv.verts_uv)[None], torch.from_numpy(uv.verts_iuv)[None], torch.from_numpy(uv.verts_map), torch.from_numpy(uv.faces)[None])
    for kw in (dict(blur_radius=0.01), dict(faces_per_pixel=2), dict(perspective_correct=True), dict(cull_backfaces=True),
               dict(clip_barycentric_coords=True), dict(background_color=(1.0, 1.0, 1.0)), dict(cam_R=torch.eye(3)[None])):
        with pytest.raises(NotImplementedError):
            tr.TexturedIUVRenderer("cuda", 1, densepose_uv=dp, **kw)
    with pytest.raises(_capi.HpsError):
        tr.TexturedIUVRenderer("cpu", 1, densepose_uv=dp)
    with pytest.raises(_capi.HpsError):
        tr.TexturedIUVRenderer("cuda", 1)


# ---------------------------------------------------------------------------------------------------------------------------------
# closed-form scenes through the restatement
# ---------------------------------------------------------------------------------------------------------------------------------
def _faces(name, dtype):
    return S.reference(name)[1 if dtype == np.float32 else 2]["pix_to_face"][0]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_pixel_centre_on_a_shared_edge_is_background(dtype):
    f = _faces("shared_edge", dtype)
    r, c = np.indices(f.shape)
    assert (f[r == c] == -1).all() and (f[r > c] == 0).all() and (f[r < c] == 1).all()
    out = S.reference("shared_edge")[2]
    assert (out["zbuf"][0][r == c] == -1).all() and (out["iuv"][0][r == c] == 0).all() and (out["rgb"][0][r == c] == 0).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_coincident_triangles_give_the_lower_face_index(dtype):
    f = _faces("coincident", dtype)
    r, c = np.indices(f.shape)
    assert (f[r > c] == 0).all() and (f[r <= c] == -1).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_faces_behind_the_camera_and_zero_area_faces_are_skipped(dtype):
    for name in ("behind", "zero_area"):
        f = _faces(name, dtype)
        r, c = np.indices(f.shape)
        assert (f[r > c] == 1).all() and (f[r <= c] == -1).all(), name
    assert (S.reference("behind")[2]["zbuf"][0][_faces("behind", np.float64) == 1] == pytest.approx(2.0, abs=1e-7))


def test_closed_form_scenes_are_the_same_in_both_dtypes():
    for name in S.closed_form_scenes():
        _, r32, r64 = S.reference(name)
        assert np.array_equal(r32["pix_to_face"], r64["pix_to_face"]), name
    assert (S.reference("whole_image")[2]["pix_to_face"] == 0).all()


def test_a_vertex_lands_in_the_pixel_perspective_project_torch_gives():
    """cam_utils.perspective_project_torch (utils/cam_utils.py:30-61): u = f (x + tx) / (z + tz) + W / 2; pixel column c holds
    u in [c, c + 1).  A triangle of 0.45 pixels around the projected point covers exactly the centre of that pixel."""
    W, f = 64, 300.0 * 64 / 256
    cam_t = np.array([0.05, -0.2, 2.5])
    for (u, v) in ((10.6, 20.3), (0.5, 63.5), (40.45, 7.55)):
        z = 0.3
        Z = z + cam_t[2]
        centre = np.array([(u - W / 2) * Z / f - cam_t[0], (v - W / 2) * Z / f - cam_t[1], z])
        d = 0.45 * Z / f
        tri = centre + np.array([[-d, -d, 0], [d, -d, 0], [0, d, 0.0]])
        sc = S.flat_scene(W, tri, [(0, 1, 2)], scale=2 * f / W, cam_t=cam_t, projection="perspective")
        for dtype in (np.float32, np.float64):
            rr, cc = np.nonzero(S.render(sc, dtype)["pix_to_face"][0] >= 0)
            assert list(zip(rr.tolist(), cc.tolist())) == [(int(v), int(u))], (u, v, dtype)


def test_the_float32_restatement_stays_within_the_near_tie_cap_on_every_scene():
    for name in list(S.CASES) + ["whole_image"]:
        scene, r32, r64 = S.reference(name)
        dev = S.deviations(scene, r32, r64)
        _, differing, covered, w_min, excess = S.agreement(scene, r32, r64)
        print("%-28s covered %6d differing %3d  deviations %s" % (name, covered, differing, dev))
        assert covered > 0
        assert differing <= S.NEAR_TIE_CAP * covered, name
        if differing:
            assert w_min > -S.FACTOR * dev["bary"] and excess < S.FACTOR * dev["zbuf"], name


def test_scenes_cover_what_they_are_for():
    sc = S.reference("w40_f257_b3")[0]
    faces64 = S.reference("w40_f257_b3")[2]["pix_to_face"]
    assert (faces64[2] == -1).all() and (faces64[1] >= 0).any()                       # wholly off the screen; partly on it
    assert (faces64[1][:, 0] >= 0).any() or (faces64[1][:, -1] >= 0).any() or (faces64[1][0] >= 0).any() or (faces64[1][-1] >= 0).any()
    assert len(np.unique(sc.verts_map)) < len(sc.verts_map)                          # duplicates
    partial = S.reference("w36_f257_b2")[2]["pix_to_face"]                             # the partial tiles of a 36-pixel image are covered
    assert (partial[0][32:, :] >= 0).any() and (partial[1][:, 32:] >= 0).any()
    # a closed sphere: front and back faces overlap in depth, so a renderer without the depth test (the first covering face wins)
    # gives another image
    sc, _, r64 = S.reference("w64_two_b1_vertex")
    _, xn, yn, Z = S.project(sc, np.float64)
    first = S.rasterise(sc, np.float64, xn, yn, np.ones_like(Z))[0]
    assert (first != r64["pix_to_face"])[r64["pix_to_face"] >= 0].mean() > 0.05
    for name in S.CASES:
        sc = S.reference(name)[0]
        assert sc.faces.max() < sc.Nd and sc.verts_map.max() < sc.V


def test_vertex_to_faces_table():
    sc = S.reference("w64_two_b1_vertex")[0]
    off, flat = tr.vertex_faces_csr(sc.faces, sc.Nd)
    off_s, flat_s = S.vertex_faces(sc.faces, sc.Nd)
    assert off.dtype == np.int32 and flat.dtype == np.int32
    assert np.array_equal(off, off_s) and np.array_equal(flat, flat_s)
    for v in (0, 5, sc.Nd - 1):
        mine = flat[off[v]:off[v + 1]]
        assert list(mine) == [f for f in range(len(sc.faces)) for k in range(3) if sc.faces[f, k] == v]
    assert (off[1:] - off[:-1]).max() >= 8                                           # a pole


# ---------------------------------------------------------------------------------------------------------------------------------
# preprocess_densepose_UV, the samplers
# ---------------------------------------------------------------------------------------------------------------------------------
def _densepose_dict():
    """Six vertices, four faces over parts 1, 2 and 8; vertices 1 and 2 lie on the boundary of parts 1 and 2, vertex 5 belongs to no
    face; 1-based indices and column vectors, as the .mat file stores them."""
    return {"All_FaceIndices": np.array([[1], [2], [8], [2]], dtype=np.float64),
            "All_Faces": np.array([[1, 2, 3], [3, 2, 4], [4, 5, 1], [2, 3, 4]], dtype=np.int64),
            "All_vertices": np.array([[7, 3, 3, 1, 9, 2]], dtype=np.uint32),
            "All_U_norm": np.array([[0.1], [0.2], [0.4], [0.6], [0.8], [0.9]], dtype=np.float64),
            "All_V_norm": np.array([[0.9], [0.7], [0.5], [0.3], [0.2], [0.1]], dtype=np.float64)}


def test_preprocess_densepose_uv_on_a_synthetic_dict():
    uv_off, iuv, verts_map, faces = tr.preprocess_densepose_UV(_densepose_dict(), 3)
    assert uv_off.shape == (3, 6, 2) and iuv.shape == (3, 6, 3) and faces.shape == (3, 4, 3) and verts_map.shape == (6,)
    assert verts_map.tolist() == [6, 2, 2, 0, 8, 1] and faces[1].tolist() == [[0, 1, 2], [2, 1, 3], [3, 4, 0], [1, 2, 3]]
    # part -> atlas cell origin: column (p - 1) // 6 of 4, row (p - 1) % 6 of 6
    origin = {1: (0.0, 0.0), 2: (0.0, 1 / 6), 8: (0.25, 1 / 6)}
    u = torch.tensor([0.1, 0.2, 0.4, 0.6, 0.8, 0.9])
    v = torch.tensor([0.9, 0.7, 0.5, 0.3, 0.2, 0.1])
    # offset ONCE, by the first face naming the vertex: 0, 1, 2 by face 0 (part 1) although faces 1 and 3 (part 2) name 1 and 2 again;
    # 3 by face 1 (part 2) although face 2 (part 8) names it again; 4 by face 2 (part 8); 5 never
    first_part = [1, 1, 1, 2, 8, None]
    for i, p in enumerate(first_part):
        if p is None:
            want_u, want_v = u[i], 1 - v[i]
        else:
            want_u = u[i] / 4 + torch.tensor(origin[p][0], dtype=torch.float32)
            want_v = 1 - ((1 - v[i]) / 6 + torch.tensor(np.linspace(0, 1, 6, endpoint=False)[int(round(origin[p][1] * 6))], dtype=torch.float32))
        assert uv_off[0, i, 0] == want_u and uv_off[2, i, 1] == want_v, i
    # the part label is the LAST face's: vertex 0 -> face 2 (8), 1 -> face 3 (2), 2 -> face 3 (2), 3 -> face 3 (2), 4 -> face 2 (8)
    assert iuv[0, :, 0].tolist() == [8.0, 2.0, 2.0, 2.0, 8.0, 0.0]
    assert torch.equal(iuv[1, :, 1], u) and torch.equal(iuv[1, :, 2], 1 - v)


def test_sampler_draws_are_the_reference_formulas_after_the_same_seed():
    """utils/augmentation/lighting_augmentation.py, smpl_augmentation.py:16-21, cam_augmentation.py: the same draws in the same order
    from torch's CPU generator, here with the global generator after torch.manual_seed."""
    cfg = configs.get_cfg_defaults().TRAIN.SYNTH_DATA.AUGMENT
    uniform = lambda r, n: (r[1] - r[0]) * torch.rand(n) + r[0]
    for bs in (1, 4):
        torch.manual_seed(11)
        got = tr.augment_light(bs, "cpu", cfg.RGB)
        after = torch.rand(1)
        torch.manual_seed(11)
        direction = torch.randn(bs, 3)
        direction = direction / torch.norm(direction, dim=-1, keepdim=True)
        want = {"location": direction * uniform(cfg.RGB.LIGHT_LOC_RANGE, bs)[:, None]}
        for key, r in (("ambient_color", cfg.RGB.LIGHT_AMBIENT_RANGE), ("diffuse_color", cfg.RGB.LIGHT_DIFFUSE_RANGE),
                       ("specular_color", cfg.RGB.LIGHT_SPECULAR_RANGE)):
            want[key] = uniform(r, bs)[:, None].expand(-1, 3)
        assert torch.equal(after, torch.rand(1))                                     # the generator is left where the reference leaves it
        for key in want:
            assert got[key].shape == (bs, 3) and torch.equal(got[key], want[key]), key
    assert cfg.RGB.LIGHT_LOC_RANGE == [0.05, 3.0] and cfg.RGB.LIGHT_SPECULAR_RANGE == [0.0, 0.5]
    mean_shape, std = torch.zeros(10), torch.full((10,), cfg.SMPL.SHAPE_STD)
    torch.manual_seed(5)
    shape = tr.normal_sample_shape(6, mean_shape, std)
    torch.manual_seed(5)
    assert torch.equal(shape, mean_shape + torch.randn(6, 10) * std)
    mean_cam_t = torch.tensor(configs.get_cfg_defaults().TRAIN.SYNTH_DATA.MEAN_CAM_T)[None].expand(6, -1)
    torch.manual_seed(6)
    cam_t = tr.augment_cam_t(mean_cam_t, cfg.CAM.XY_STD, cfg.CAM.DELTA_Z_RANGE)
    torch.manual_seed(6)
    want = mean_cam_t.clone()
    want[:, :2] = mean_cam_t[:, :2] + torch.randn(6, 2) * cfg.CAM.XY_STD
    want[:, 2] = mean_cam_t[:, 2] + uniform(cfg.CAM.DELTA_Z_RANGE, 6)
    assert torch.equal(cam_t, want)
