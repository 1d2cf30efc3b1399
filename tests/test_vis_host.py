"""CPU: the restatement the predict visualisation kernels are held to (tests/vis_scenario.py) against what it restates -- matplotlib's
jet and Normalize, Rodrigues rotations, torch's F.interpolate -- and against closed-form warps; the package's colour table against
matplotlib's; the new entry points' argument checks, which run before any launch."""
import ctypes

import numpy as np
import pytest
import torch

import vis_scenario as V
from hierarchicalprobabilistic3dhuman_amd import _capi, visualise


def test_jet_lut_is_matplotlibs_table():
    import matplotlib.cm
    want = matplotlib.cm.jet(np.arange(256))[:, :3]
    lut = visualise.jet_lut()
    assert lut.dtype == np.float32 and lut.shape == (256, 3)
    assert np.array_equal(lut, want.astype(np.float32))
    assert np.array_equal(V.jet_table(), want)


def test_colour_restatement_equals_matplotlib_on_every_bin_edge():
    import matplotlib.pyplot as plt
    var = V.colour_edge_values()
    assert var.dtype == np.float32 and len(var) >= 3 * 257
    want = plt.cm.jet(plt.Normalize(vmin=0.0, vmax=0.2, clip=True)(var))[:, :3]
    got = V.jet_colours(var)
    assert np.array_equal(got, want)
    # the values sit where they should: below every edge the bin before it
    k = np.arange(1, 256)
    e = (0.2 * k / 256).astype(np.float32)
    assert (V.jet_index(np.nextafter(e, np.float32(1))) >= V.jet_index(np.nextafter(e, np.float32(-1)))).all()
    assert V.jet_index(np.float32([0.2, 5.0]))[0] == 255 and V.jet_index(np.float32([-1.0]))[0] == 0


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_view_maps_are_the_reference_rotations(k):
    """predict/...:118-134: pi about x, then k times -pi / 2 about y."""
    R = V.rodrigues((1, 0, 0), np.pi)
    for _ in range(k):
        R = V.rodrigues((0, 1, 0), -np.pi / 2) @ R
    assert np.abs(V.view_matrix(k) - R).max() <= 1e-15
    p = np.random.RandomState(k).standard_normal((50, 3))
    assert np.array_equal(V.view_map(p, k), p @ V.view_matrix(k).T)
    assert np.array_equal(V.view_map(p.astype(np.float32), k), (p.astype(np.float32) @ V.view_matrix(k).T.astype(np.float32)))


@pytest.mark.parametrize("D,wh", [(8, 16), (20, 21), (36, 16)])
def test_resize_restatement_agrees_with_torch_interpolate(D, wh):
    img = np.random.RandomState(D).rand(3, D, D).astype(np.float32)
    want = torch.nn.functional.interpolate(torch.from_numpy(img)[None], size=(wh, wh), mode="bilinear", align_corners=False)[0].numpy()
    for dtype in (np.float64, np.float32):
        assert np.abs(V.resize(img, wh, dtype).astype(np.float64) - want).max() <= 1e-6


def test_warp_restatement_identity_and_integer_translations():
    rs = np.random.RandomState(4)
    wh = 12
    src = rs.rand(3, wh, wh).astype(np.float32)
    M = V.uncrop_matrix((wh / 2.0, wh / 2.0), wh, wh)
    assert np.array_equal(M, np.float32([[1, 0, 0], [0, 1, 0]]))
    assert np.array_equal(V.warp_linear(src, M, wh, wh, np.float32), src) and np.array_equal(V.warp_nearest(src[0], M, wh, wh), src[0])
    for dy, dx in ((3, 0), (0, -2), (5, 4), (-13, 1)):
        M = V.uncrop_matrix((wh / 2.0 + dy, wh / 2.0 + dx), wh, wh)                  # the render's centre lands dy down, dx right
        want = np.zeros((3, 20, 18), dtype=np.float32)
        for y in range(20):
            for x in range(18):
                if 0 <= y - dy < wh and 0 <= x - dx < wh:
                    want[:, y, x] = src[:, y - dy, x - dx]
        assert np.array_equal(V.warp_linear(src, M, 20, 18, np.float32), want)
        assert np.array_equal(V.warp_linear(src, M, 20, 18, np.float64), want.astype(np.float64))
        assert np.array_equal(V.warp_nearest(src[1], M, 20, 18), want[1])


def test_warp_restatement_times_two_with_a_border_crossing():
    """side = 2 wh, centre 5: the matrix is x -> 2 x + 1, its inverse x -> (x - 1) / 2.  In fixed point the linear position of
    column x is 16 x - 16 thirty-seconds: index floor((x - 1) / 2), fraction one half at even x; the nearest index is floor(x / 2).
    Worked by hand for a = (0.25, 0.5, 0.75, 1): linear (0.125, 0.25, 0.375, 0.5, 0.625, 0.75, 0.875, 1, 0.5, 0), the first and the last but
    one averaging with the zero border; nearest (a0, a0, a1, a1, a2, a2, a3, a3, 0, 0)."""
    a = np.float64([0.25, 0.5, 0.75, 1.0])
    lin = np.float64([0.125, 0.25, 0.375, 0.5, 0.625, 0.75, 0.875, 1.0, 0.5, 0.0])
    near = np.float64([0.25, 0.25, 0.5, 0.5, 0.75, 0.75, 1.0, 1.0, 0.0, 0.0])
    b = np.float64([1.0, 0.5, 0.25, 0.125])
    lin_b = np.float64([0.5, 1.0, 0.75, 0.5, 0.375, 0.25, 0.1875, 0.125, 0.0625, 0.0])
    M = V.uncrop_matrix((5.0, 5.0), 8.0, 4)
    assert np.array_equal(M, np.float32([[2, 0, 1], [0, 2, 1]]))
    src = np.outer(b, a)[None]                                                      # rows b, columns a: bilinear is separable
    assert np.array_equal(V.warp_linear(src, M, 10, 10, np.float64)[0], np.outer(lin_b, lin))
    assert np.array_equal(V.warp_linear(src, M, 10, 10, np.float32)[0], np.outer(lin_b, lin).astype(np.float32))
    assert np.array_equal(V.warp_nearest(np.outer(np.ones(4), a), M, 10, 10)[0], near)
    p = V.warp_positions(M, 10, 10)
    assert p["sx"][0].tolist() == [-1, 0, 0, 1, 1, 2, 2, 3, 3, 4] and p["fx"][0].tolist() == [16, 0] * 5


def test_uncrop_restatement_returns_the_photograph_outside_the_body():
    inp = V.uncrop_inputs(1, 37, 50, 16)
    (centre, side) = V.uncrop_boxes(37, 50)["inside"]
    s, body = V.uncrop(inp.rgb, inp.iplane, inp.image, centre, side)
    assert body.any() and not body.all()
    assert np.array_equal(V.to_byte(s)[~body], inp.u8[~body])


def test_compose_restatement_layout_and_rounding():
    rows, cols, n, panels = V.LAYOUTS["3x6"]
    inp = V.compose_inputs(2, 16, 8, n)
    s = V.compose(rows, cols, 16, panels, inp.rgb, inp.iuv, inp.crop)
    assert s.shape == (48, 96, 3) and (s[32:, 64:] == 0).all()                        # cells 16 and 17 are empty
    m = 3                                                                           # cell 3: a plain render
    assert np.array_equal(s[:16, 48:64], 255.0 * inp.rgb[m].transpose(1, 2, 0).astype(np.float64))
    back = np.rint(inp.iuv[2][0]) == 0                                              # cell 2: over the crop; 0.5 rounds to 0, 1.5 to 2
    assert back[inp.iuv[2][0] == np.float32(0.5)].all() and not back[inp.iuv[2][0] == np.float32(0.50001)].any()
    crop = 255.0 * V.resize(inp.crop, 16).transpose(1, 2, 0)
    assert np.array_equal(s[:16, 32:48][back], crop[back])
    assert V.to_byte(np.float64([0.5, 1.5, 2.5, -3.0, 300.0, 65025.0])).tolist() == [0, 2, 2, 0, 255, 255]


def test_new_entry_points_refuse_bad_arguments_before_any_launch():
    lib = _capi.load()
    for name, cls in (("views", _capi.VisViewsArgs), ("compose", _capi.VisComposeArgs), ("uncrop", _capi.VisUncropArgs)):
        assert getattr(lib, "hps_sizeof_vis_%s_args" % name)() == ctypes.sizeof(cls)
        fn = getattr(lib, "hps_vis_" + name)
        assert fn(None, None) == -1
        a = cls()
        a.struct_bytes = ctypes.sizeof(cls) - 4
        assert fn(ctypes.addressof(a), None) == -1 and b"struct_bytes" in lib.hps_last_error()
    fake = ctypes.c_void_p(4096)                                                    # never dereferenced: every call below is refused
    a = _capi.VisViewsArgs()
    a.struct_bytes, a.num_views, a.num_verts = ctypes.sizeof(a), 1, 10
    table = (_capi.VisView * 1)()
    table[0].vertices, table[0].yaw = fake, 4
    a.views, a.lut, a.out_vertices, a.out_colours = table, fake, fake, fake
    assert lib.hps_vis_views(ctypes.addressof(a), None) == -1 and b"yaw" in lib.hps_last_error()
    a.num_views = _capi.VIS_MAX_VIEWS + 1
    assert lib.hps_vis_views(ctypes.addressof(a), None) == -1
    c = _capi.VisComposeArgs()
    c.struct_bytes, c.rows, c.cols, c.wh, c.num_renders, c.out, c.rgb = ctypes.sizeof(c), 2, 4, 16, 2, fake, fake
    panels = (_capi.VisPanel * 2)()
    panels[0].kind, panels[0].render = _capi.VIS_PANEL_RENDER, 2
    c.panels, c.num_panels = panels, 1
    assert lib.hps_vis_compose(ctypes.addressof(c), None) == -1 and b"render index" in lib.hps_last_error()
    panels[0].render, panels[1].kind = 0, _capi.VIS_PANEL_RENDER
    c.num_panels = 2
    assert lib.hps_vis_compose(ctypes.addressof(c), None) == -1 and b"one cell" in lib.hps_last_error()
    c.num_panels, c.out = 1, ctypes.c_void_p(4100)
    assert lib.hps_vis_compose(ctypes.addressof(c), None) == -1 and b"aligned" in lib.hps_last_error()
    c.out, c.rows, c.cols = fake, 6, 6
    assert lib.hps_vis_compose(ctypes.addressof(c), None) == -1
    u = _capi.VisUncropArgs()
    u.struct_bytes, u.H, u.W, u.wh = ctypes.sizeof(u), 10, 0, 16
    u.rgb = u.iplane = u.image = u.bbox_centre = u.bbox_wh = u.out = fake
    assert lib.hps_vis_uncrop(ctypes.addressof(u), None) == -1


def test_visualiser_refuses_a_renderer_that_does_not_fit():
    from types import SimpleNamespace as NS
    cfg = NS(DATA=NS(PROXY_REP_SIZE=256))
    ok = dict(projection_type="orthographic", render_rgb=True, img_wh=64, device=torch.device("cpu"))
    for bad in (dict(projection_type="perspective"), dict(render_rgb=False), dict(img_wh=32)):
        with pytest.raises(_capi.HpsError):
            visualise.PredictVisualiser(NS(**dict(ok, **bad)), cfg, 64)
