"""The predict visualisations on the device (csrc/visualise.hip through visualise.PredictVisualiser and
predict_poseMF_shapeGaussian_net(vis_renderer=...)) against the restatement of tests/vis_scenario.py.

Colours and views: bit for bit.  Figures and the uncropped picture: a byte may differ from the float64 restatement by 1, and only where
255 v lies within FACTOR x (the float32 twin's largest deviation on that input) of a half-integer; the body / background choice, the
joint discs, empty cells and the photograph's own pixels are exact.  The restatement is fed the planes the kernels were given, so only
the new code is under test.  End to end: the three PNG files per image from all three delivery routes, decoded PNG == device bytes,
the posed panel against a separate forward() of the same view, repeatability, and no picture and the same .pt files without a
renderer."""
import functools
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import vis_scenario as V
from hierarchicalprobabilistic3dhuman_amd import _capi, configs, textured_renderer as tr, visualise

pytestmark = pytest.mark.gpu


def _stub_visualiser(wh, D):
    """A visualiser for the kernel-level tests: no renderer is called, the planes come from the scenario."""
    renderer = NS(projection_type="orthographic", render_rgb=True, img_wh=wh, device=torch.device("cuda", torch.cuda.current_device()))
    return visualise.PredictVisualiser(renderer, NS(DATA=NS(PROXY_REP_SIZE=D)), wh)


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ---------------------------------------------------------------------------------------------------------------------------------
# hps_vis_views
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nv", [1, 63, 64, 65, 257])
def test_colours_equal_matplotlibs_floats_bit_for_bit(dev, nv):
    import matplotlib.pyplot as plt
    edge = V.colour_edge_values()
    starts = list(range(0, len(edge), nv))[:_capi.VIS_MAX_VIEWS]
    var = np.stack([edge[(s + np.arange(nv)) % len(edge)] for s in starts])
    verts = np.zeros((nv, 3), dtype=np.float32)
    vis = _stub_visualiser(16, 8)
    _, colours, _, _ = vis._views([(_cuda(verts), _cuda(v), 0, 0) for v in var], _cuda(np.float32([1, 0, 0])))
    want = plt.cm.jet(plt.Normalize(vmin=0.0, vmax=0.2, clip=True)(var))[..., :3].astype(np.float32)
    assert np.array_equal(_bits(colours.cpu().numpy()), _bits(want))
    assert np.array_equal(_bits(want), _bits(V.jet_colours(var).astype(np.float32)))
    if nv == 257:
        assert len(starts) * nv >= len(edge)                                          # every edge value went through the kernel


@pytest.mark.parametrize("nv", [1, 65, 6890])
def test_views_are_signed_permutations_bit_for_bit(dev, nv):
    rs = np.random.RandomState(nv)
    meshes = rs.standard_normal((2, nv, 3)).astype(np.float32)
    meshes[0, 0] = (0.0, -0.0, 0.0)
    var = rs.uniform(-0.05, 0.3, (2, nv)).astype(np.float32)
    table = [(0, 0, 1, 1), (1, 3, 0, 0), (0, 2, 0, 1), (1, 1, 1, 0), (1, 0, 0, 0), (0, 3, 1, 1), (0, 1, 1, 0)]      # mesh, yaw, jet?, camera
    cam = np.float32([0.83, 0.11, -0.07])
    d_mesh, d_var = _cuda(meshes), _cuda(var)
    vis = _stub_visualiser(16, 8)
    out = vis._views([(d_mesh[m], d_var[m] if jet else None, yaw, camera) for m, yaw, jet, camera in table], _cuda(cam))
    verts, colours, cam_t, scale = (t.cpu().numpy() for t in out)
    for i, (m, yaw, jet, camera) in enumerate(table):
        assert np.array_equal(_bits(verts[i]), _bits(V.view_map(meshes[m], yaw))), i
        want = V.jet_colours(var[m]).astype(np.float32) if jet else np.full((nv, 3), np.float32(0.7))
        assert np.array_equal(_bits(colours[i]), _bits(want)), i
        assert cam_t[i].tolist() == ([cam[1], cam[2], 2.5] if camera else [0.0, np.float32(-0.2), 2.5]), i
        assert scale[i].tolist() == ([cam[0]] * 2 if camera else [np.float32(0.95)] * 2), i
    again = vis._views([(d_mesh[m], d_var[m] if jet else None, yaw, camera) for m, yaw, jet, camera in table], _cuda(cam))
    assert all(np.array_equal(_bits(a.cpu().numpy()), _bits(b)) for a, b in zip(again, (verts, colours, cam_t, scale)))


# ---------------------------------------------------------------------------------------------------------------------------------
# hps_vis_compose
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["2x4", "3x6"])
@pytest.mark.parametrize("D", [8, 20])
@pytest.mark.parametrize("wh", [16, 21, 36])
def test_compose_against_the_float64_restatement(dev, wh, D, layout):
    rows, cols, n, panels = V.LAYOUTS[layout]
    inp = V.compose_inputs(100 * wh + D + rows, wh, D, n)
    proxy = inp.proxy if layout == "2x4" else None
    joints = inp.joints if layout == "2x4" else None
    vis = _stub_visualiser(wh, D)
    bufs = dict(rgb=_cuda(inp.rgb), iuv=_cuda(inp.iuv))
    out = vis._compose("t", rows, cols, panels, bufs, _cuda(inp.crop), _cuda(proxy), _cuda(joints))
    assert out.dtype == torch.uint8 and tuple(out.shape) == (rows * wh, cols * wh, 3)
    got = out.cpu().numpy()
    s64, s32 = (V.compose(rows, cols, wh, panels, inp.rgb, inp.iuv, inp.crop, proxy, joints, dtype=dt) for dt in (np.float64, np.float32))
    worst, near, tol = V.byte_rule(got, s64, s32)
    print("compose wh %d D %d %s: differing bytes %d of %d, tolerance %.3e" % (wh, D, layout, int((got != V.to_byte(s64)).sum()), got.size, tol))
    assert worst <= 1 and near
    # exact: discs and empty cells (values nowhere near a half-integer), and the choice between body and crop
    if layout == "2x4":
        disc = (s64 == (65025.0, 0.0, 0.0)).all(axis=-1)
        assert disc.any() and (got[disc] == (255, 0, 0)).all()
        on_border = disc[wh:, :wh]
        assert on_border[0, :4].any() and on_border[-1, -4:].any()                    # the joints at (0, 0) and (D - 0.01, D - 0.01)
    else:
        assert (got[2 * wh:, 4 * wh:] == 0).all()
    m = 0                                                                           # cell (0, 1) / (0, 0): render 0 over the crop
    cell = got[:wh, wh:2 * wh] if layout == "2x4" else got[:wh, :wh]
    body = np.rint(inp.iuv[m][0]) != 0
    assert not body[inp.iuv[m][0] == np.float32(0.5)].any() and body[inp.iuv[m][0] == np.float32(0.50001)].all()
    own = V.to_byte(V.scaled(inp.rgb[m], np.float32)).transpose(1, 2, 0)            # a render's bytes are the device's own float32 product
    assert np.array_equal(cell[body], own[body])
    # without a crop the panels behind it are black
    out = vis._compose("t", rows, cols, panels, bufs, None, _cuda(proxy), _cuda(joints))
    got = out.cpu().numpy()
    assert (cell.shape == (wh, wh, 3)) and (got[:wh, wh:2 * wh] if layout == "2x4" else got[:wh, :wh])[~body].max() == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# hps_vis_uncrop
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wh", [16, 21])
@pytest.mark.parametrize("H,W", [(37, 50), (50, 37)])
def test_uncrop_against_the_float64_restatement(dev, H, W, wh):
    inp = V.uncrop_inputs(H * wh, H, W, wh)
    vis = _stub_visualiser(wh, 8)
    iuv = np.zeros((1, 3, wh, wh), dtype=np.float32)
    iuv[0, 0] = inp.iplane
    vis._figure_render = dict(rgb=_cuda(inp.rgb[None]), iuv=_cuda(iuv))
    image = _cuda(inp.image)
    for name, (centre, side) in V.uncrop_boxes(H, W).items():
        out = vis.uncropped(image, _cuda(np.float32(centre)), _cuda(np.float32([side])))
        assert out.dtype == torch.uint8 and tuple(out.shape) == (H, W, 3)
        got = out.cpu().numpy()
        (s64, body), (s32, body32) = (V.uncrop(inp.rgb, inp.iplane, inp.image, centre, side, dtype=dt) for dt in (np.float64, np.float32))
        assert np.array_equal(body, body32) and body.any() and not body.all(), name
        assert np.array_equal(got[~body], inp.u8[~body]), name                       # the photograph's own pixels, unchanged
        worst, near, tol = V.byte_rule(got, s64, s32)
        print("uncrop %dx%d wh %d %s: body %d pixels, differing bytes %d, tolerance %.3e" % (H, W, wh, name, int(body.sum()), int((got != V.to_byte(s64)).sum()), tol))
        assert worst <= 1 and near, name
        # the mask is exact: the integer arithmetic is the restatement's
        changed = (got != inp.u8).any(axis=-1)
        assert not changed[~body].any(), name


# ---------------------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------------------
WH = 64


class _ToyHRNet(torch.nn.Module):
    """Stand-in for the injected 2D keypoint detector: (1,3,h,w) -> (1,17,h/4,w/4)."""

    def __init__(self):
        super().__init__()
        torch.manual_seed(123)
        self.conv = torch.nn.Conv2d(3, 17, kernel_size=8, stride=4, padding=2)

    def forward(self, x):
        return self.conv(x)


class _ToyDetector(torch.nn.Module):
    """Stand-in for the injected person detector: one confident 'person' box inside the image."""

    def forward(self, images):
        H, W = images.shape[-2:]
        box = torch.tensor([[0.2 * W, 0.1 * H, 0.85 * W, 0.95 * H]], device=images.device)
        return [{"labels": torch.ones(1, dtype=torch.int64, device=images.device), "scores": torch.ones(1, device=images.device),
                 "boxes": box}]


def _densepose(num_verts, seed=31, num_faces=300):
    """A synthetic DensePose table over the synthetic SMPL's vertices: every vertex once, 5 % twice, ``num_faces`` faces over them."""
    rs = np.random.RandomState(seed)
    verts_map = np.concatenate([np.arange(num_verts), rs.randint(0, num_verts, num_verts // 20)])
    Nd = len(verts_map)
    faces = np.stack([rs.choice(Nd, 3, replace=False) for _ in range(num_faces)]).astype(np.int64)
    iuv = np.stack([1 + np.arange(Nd) % 24, rs.rand(Nd), rs.rand(Nd)], axis=1).astype(np.float32)
    return (torch.from_numpy(rs.rand(1, Nd, 2).astype(np.float32)), torch.from_numpy(iuv)[None], torch.from_numpy(verts_map),
            torch.from_numpy(faces)[None])


@pytest.fixture(scope="module")
def harness(dev, net_gpu, smpl_gpu, tmp_path_factory):
    from hierarchicalprobabilistic3dhuman_amd.canny_edge_detector import CannyEdgeDetector
    from hierarchicalprobabilistic3dhuman_amd import predict_poseMF_shapeGaussian_net as P
    cfg = configs.get_cfg_defaults()
    root = tmp_path_factory.mktemp("predict_vis")
    image_dir = root / "images"
    os.makedirs(image_dir)
    rs = np.random.RandomState(5)
    sizes = {"a": (60, 60), "b": (48, 72), "c": (64, 64)}                            # one is not square
    for name, (h, w) in sizes.items():
        base = rs.rand(h // 4, w // 4, 3)
        np.save(str(image_dir / (name + ".npy")), (np.kron(base, np.ones((4, 4, 1))) * 255).astype(np.uint8))
    hrnet, detector = _ToyHRNet().to(dev), _ToyDetector().to(dev)
    hrnet_cfg = NS(MODEL=NS(IMAGE_SIZE=[288, 384], HEATMAP_SIZE=[72, 96]))
    edge = CannyEdgeDetector(non_max_suppression=cfg.DATA.EDGE_NMS, gaussian_filter_std=cfg.DATA.EDGE_GAUSSIAN_STD,
                             gaussian_filter_size=cfg.DATA.EDGE_GAUSSIAN_SIZE, threshold=cfg.DATA.EDGE_THRESHOLD).to(dev)
    renderer = tr.TexturedIUVRenderer(dev, 1, img_wh=WH, projection_type="orthographic", render_rgb=True, bin_size=32,
                                      densepose_uv=_densepose(smpl_gpu.num_verts))
    written = []
    original = visualise.PngWriter.write

    def recording_write(self, image, path):
        written.append((path, image.cpu().numpy().copy()))
        return original(self, image, path)

    @functools.lru_cache(maxsize=None)
    def run(batch_size, with_renderer, tag=""):
        save_dir = root / ("out_b%d_%d%s" % (batch_size, with_renderer, tag))
        del written[:]
        torch.manual_seed(11)
        visualise.PngWriter.write = recording_write
        try:
            P.predict_poseMF_shapeGaussian_net(net_gpu, cfg, smpl_gpu, hrnet, hrnet_cfg, edge, dev, str(image_dir), str(save_dir),
                                               object_detect_model=detector, visualise_wh=WH, visualise_uncropped=True,
                                               visualise_samples=True, num_samples=12, batch_size=batch_size,
                                               vis_renderer=renderer if with_renderer else None)
        finally:
            visualise.PngWriter.write = original
        return save_dir, dict(written)

    front = P._reference_front_end(cfg, hrnet, hrnet_cfg, edge, detector, 0.75, dev)
    return NS(cfg=cfg, run=run, sizes=sizes, renderer=renderer, image_dir=image_dir, front=front)


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(str(path)))


@pytest.mark.parametrize("batch_size", [1, 2, 3])          # hipGraph replays; graphs and the eager path for the last image; the pipeline
def test_predict_writes_the_three_pictures(harness, batch_size):
    save_dir, device_bytes = harness.run(batch_size, True)
    for name, (h, w) in harness.sizes.items():
        for suffix, shape in (("", (2 * WH, 4 * WH, 3)), ("_uncrop", (h, w, 3)), ("_samples", (3 * WH, 6 * WH, 3))):
            path = save_dir / (name + suffix + ".png")
            assert path.exists(), path
            img = _png(path)
            assert img.shape == shape and img.dtype == np.uint8
            assert np.array_equal(img, device_bytes[str(path)])                      # the decoded PNG is the device's bytes
        assert (save_dir / (name + ".pt")).exists()
        fig = _png(save_dir / (name + ".png"))
        assert fig[:WH, WH:2 * WH].std() > 0 and fig[WH:, :WH].max() == 255           # a body over a crop; red discs on the proxy panel
    assert not [f for f in os.listdir(str(save_dir)) if f.endswith(".part")]


def test_the_posed_panel_is_a_separate_forward_of_the_same_view(harness, dev):
    save_dir, _ = harness.run(3, True)
    vis = visualise.predict_visualiser(harness.renderer, harness.cfg, WH)
    for name in harness.sizes:
        saved = torch.load(str(save_dir / (name + ".pt")))
        ex = harness.front.with_extras(str(harness.image_dir / (name + ".npy")))
        verts = V.view_map(saved["verts_mode"].numpy(), 0)
        colours = V.jet_colours(saved["unc"].numpy()).astype(np.float32)
        cam = saved["cam"].numpy()
        out = harness.renderer(vertices=_cuda(verts[None]), cam_t=_cuda(np.float32([[cam[1], cam[2], 2.5]])),
                               orthographic_scale=_cuda(np.float32([[cam[0], cam[0]]])), lights_rgb_settings=vis.lights,
                               verts_features=_cuda(colours[None]))
        rgb = out["rgb_images"].permute(0, 3, 1, 2).cpu().numpy()
        iuv = out["iuv_images"].permute(0, 3, 1, 2).cpu().numpy()
        crop = ex["cropped_rgb"][0].cpu().numpy()
        panel = ((V.RENDER_OVER_CROP, 0, 0, 0),)
        s64, s32 = (V.compose(1, 1, WH, panel, rgb, iuv, crop, dtype=dt) for dt in (np.float64, np.float32))
        got = _png(save_dir / (name + ".png"))[:WH, WH:2 * WH]
        worst, near, tol = V.byte_rule(got, s64, s32)
        assert worst <= 1 and near, name
        body = np.rint(iuv[0, 0]) != 0
        assert body.any() and not body.all(), name
        # the uncropped picture keeps the photograph outside the body
        photo = np.load(str(harness.image_dir / (name + ".npy")))
        un = _png(save_dir / (name + "_uncrop.png"))
        side = float(ex["bbox_wh"].cpu())
        centre = ex["bbox_centre"].cpu().numpy()
        _, mask = V.uncrop(rgb[0], iuv[0, 0], photo.transpose(2, 0, 1).astype(np.float32) / np.float32(255), centre, side)
        assert np.array_equal(un[~mask], photo[~mask]) and mask.any(), name


def test_two_runs_write_identical_files_and_no_renderer_means_no_picture(harness):
    first, _ = harness.run(3, True)
    second, _ = harness.run(3, True, "_again")
    plain, _ = harness.run(3, False)
    names = sorted(os.listdir(str(first)))
    assert names == sorted(os.listdir(str(second))) and len(names) == 4 * len(harness.sizes)
    for f in names:
        if f.endswith(".png"):
            assert open(str(first / f), "rb").read() == open(str(second / f), "rb").read(), f
    assert sorted(os.listdir(str(plain))) == sorted(n + ".pt" for n in harness.sizes)
    for n in harness.sizes:
        a, b = torch.load(str(first / (n + ".pt"))), torch.load(str(plain / (n + ".pt")))
        assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a), n


def test_a_bare_proxy_tensor_gives_black_crop_panels_and_one_warning(harness, dev, net_gpu, smpl_gpu, tmp_path):
    from hierarchicalprobabilistic3dhuman_amd import predict_poseMF_shapeGaussian_net as P
    bare = lambda path: harness.front(path)
    with pytest.warns(UserWarning, match="uncropped pictures are skipped") as rec:
        P.predict_poseMF_shapeGaussian_net(net_gpu, harness.cfg, smpl_gpu, None, None, None, dev, str(harness.image_dir), str(tmp_path),
                                           visualise_wh=WH, proxy_rep_fn=bare, num_samples=12, batch_size=3, vis_renderer=harness.renderer)
    assert len([w for w in rec if "uncropped" in str(w.message)]) == 1
    for name in harness.sizes:
        fig = _png(tmp_path / (name + ".png"))
        assert fig[:WH, :WH].max() == 0 and fig[WH:, :WH].max() > 0                   # no crop; the proxy panel is there, without discs
        assert not ((fig[WH:, :WH, 0] == 255) & (fig[WH:, :WH, 1] == 0)).any()
        assert not (tmp_path / (name + "_uncrop.png")).exists() and not (tmp_path / (name + "_samples.png")).exists()


def test_a_second_call_allocates_no_device_memory(harness, dev):
    save_dir, _ = harness.run(3, True)
    vis = visualise.predict_visualiser(harness.renderer, harness.cfg, WH)
    saved = torch.load(str(save_dir / "a.pt"))
    ex = harness.front.with_extras(str(harness.image_dir / "a.npy"))
    g = torch.Generator().manual_seed(2)
    V_ = saved["verts_mode"].shape[0]
    result = {k: saved[k].to(dev) for k in ("verts_mode", "verts_tpose", "unc", "cam")}
    result["verts_samples"] = (saved["verts_mode"][None] + 0.01 * torch.randn(12, V_, 3, generator=g)).to(dev)
    result["joints_samples"] = torch.randn(12, 90, 3, generator=g).to(dev)

    def pictures():
        a = vis.figure(result, ex["cropped_rgb"], ex["proxy_rep"], ex["joints2D"]).clone()
        b = vis.uncropped(ex["image"], ex["bbox_centre"], ex["bbox_wh"]).clone()
        c = vis.samples_figure(result, ex["cropped_rgb"], ex["proxy_rep"]).clone()
        return a, b, c
    first = pictures()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    vis.figure(result, ex["cropped_rgb"], ex["proxy_rep"], ex["joints2D"])
    vis.uncropped(ex["image"], ex["bbox_centre"], ex["bbox_wh"])
    vis.samples_figure(result, ex["cropped_rgb"], ex["proxy_rep"])
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before
    assert all(torch.equal(x, y) for x, y in zip(first, pictures()))
    assert tuple(first[0].shape) == (2 * WH, 4 * WH, 3) and tuple(first[2].shape) == (3 * WH, 6 * WH, 3)
