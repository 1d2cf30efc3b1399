"""The predict visualisations' restatement and inputs (tests/test_vis_host.py, tests/test_gpu_predict_vis.py).

A numpy restatement of include/hps.h's hps_vis_views, hps_vis_compose and hps_vis_uncrop, operation by operation, in a chosen dtype:
float64 is the yardstick the device is held to, float32 is the twin whose own deviation from float64 sets the tolerance (the
convention and the FACTOR of tests/render_scenario.py).  The colour rule is pinned to matplotlib, the resize to torch's
F.interpolate, the view maps to Rodrigues matrices (tests/test_vis_host.py); the fixed-point warp restates cv2.warpAffine as we read
its sources and has not been run against OpenCV.  Inputs come from seeds, never from files.
"""
from types import SimpleNamespace

import numpy as np

from render_scenario import FACTOR      # noqa: F401  (the tests take it from here)

RENDER, RENDER_OVER_CROP, CROP, PROXY = 0, 1, 2, 3
VAR_MAX = 0.2

_JET = {"red": ((0.00, 0, 0), (0.35, 0, 0), (0.66, 1, 1), (0.89, 1, 1), (1.00, 0.5, 0.5)),
        "green": ((0.000, 0, 0), (0.125, 0, 0), (0.375, 1, 1), (0.640, 1, 1), (0.910, 0, 0), (1.000, 0, 0)),
        "blue": ((0.00, 0.5, 0.5), (0.11, 1, 1), (0.34, 1, 1), (0.65, 0, 0), (1.00, 0, 0))}


# ---------------------------------------------------------------------------------------------------------------------------------
# colours and views
# ---------------------------------------------------------------------------------------------------------------------------------
def jet_table():
    """jet's 256-entry table in float64: each channel interpolated linearly between its published segment points (x, y0, y1) at the
    256 positions 255 linspace(0, 1, 256) of the axis stretched to [0, 255]; the ends take y1 of the first and y0 of the last point."""
    cols = []
    for name in ("red", "green", "blue"):
        seg = np.array(_JET[name], dtype=np.float64)
        x, y0, y1 = seg[:, 0] * 255, seg[:, 1], seg[:, 2]
        at = 255 * np.linspace(0, 1, 256)
        hi = np.searchsorted(x, at)[1:-1]
        t = (at[1:-1] - x[hi - 1]) / (x[hi] - x[hi - 1])
        cols.append(np.clip(np.concatenate([[y1[0]], t * (y0[hi] - y1[hi - 1]) + y1[hi - 1], [y0[-1]]]), 0.0, 1.0))
    return np.stack(cols, axis=1)


def jet_index(var):
    """float32 variances -> table index: float64 arithmetic -- clip to [0, 0.2], / 0.2, * 256, truncate, 256 -> 255."""
    t = np.clip(np.asarray(var, dtype=np.float32).astype(np.float64), 0.0, VAR_MAX) / VAR_MAX * 256.0
    i = t.astype(np.int64)
    i[i == 256] = 255
    return i


def jet_colours(var):
    """plt.cm.jet(plt.Normalize(0, 0.2, clip=True)(var))[:, :3] restated, float64."""
    return jet_table()[jet_index(var)]


def colour_edge_values():
    """Every bin edge 0.2 k / 256 and its two float32 neighbours, 0, 0.2, negatives and values above 0.2; float32."""
    e = (0.2 * np.arange(257) / 256).astype(np.float32)
    return np.concatenate([e, np.nextafter(e, np.float32(-1)), np.nextafter(e, np.float32(1)),
                           np.float32([0.0, 0.2, -1.0, -1e-9, -0.0, 0.3, 5.0, 1e30, 0.19999999])]).astype(np.float32)


def view_matrix(k):
    """(x, y, z) -> (x, -y, -z), then k times (x, y, z) -> (-z, y, x), as a matrix of 0 and +-1 acting on column vectors."""
    M = np.diag([1.0, -1.0, -1.0])
    step = np.array([[0.0, 0.0, -1.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0]])
    for _ in range(k):
        M = step @ M
    return M


def view_map(verts, k):
    """The view's vertices, exactly: a signed permutation of the columns (dtype kept)."""
    v = np.asarray(verts)
    x, y, z = v[..., 0], -v[..., 1], -v[..., 2]
    for _ in range(k):
        x, z = -z, x
    return np.stack([x, y, z], axis=-1)


def rodrigues(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


# ---------------------------------------------------------------------------------------------------------------------------------
# resize, bytes, compose
# ---------------------------------------------------------------------------------------------------------------------------------
def resize_taps(D, wh, dtype):
    """(i0, i1, l0, l1) per output index: position max((i + 0.5) D / wh - 0.5, 0), the upper neighbour clamped to D - 1."""
    dt = np.dtype(dtype).type
    scale = dt(D) / dt(wh)
    s = np.maximum((np.arange(wh).astype(dtype) + dt(0.5)) * scale - dt(0.5), dt(0))
    i0 = np.minimum(s.astype(np.int64), D - 1)
    i1 = np.minimum(i0 + 1, D - 1)
    l1 = s - i0.astype(dtype)
    return i0, i1, dt(1) - l1, l1


def resize(img, wh, dtype=np.float64):
    """(C, D, D) -> (C, wh, wh): F.interpolate(mode='bilinear', align_corners=False) / cv2.resize(INTER_LINEAR)."""
    img = np.asarray(img, dtype=dtype)
    i0, i1, l0, l1 = resize_taps(img.shape[-1], wh, dtype)
    r0, r1 = img[:, i0], img[:, i1]                                                    # rows
    top = l0[None, None, :] * r0[:, :, i0] + l1[None, None, :] * r0[:, :, i1]
    bot = l0[None, None, :] * r1[:, :, i0] + l1[None, None, :] * r1[:, :, i1]
    return l0[None, :, None] * top + l1[None, :, None] * bot


def scaled(v, dtype):
    """255 v in ``dtype``, as float64: what is rounded to a byte."""
    return (np.dtype(dtype).type(255) * np.asarray(v, dtype=dtype)).astype(np.float64)


def to_byte(s):
    return np.clip(np.rint(s), 0, 255).astype(np.uint8)


def compose(rows, cols, wh, panels, rgb=None, iuv=None, crop=None, proxy=None, joints=None, dtype=np.float64):
    """hps_vis_compose: the (rows wh, cols wh, 3) array of 255 v BEFORE rounding (float64; to_byte() makes the figure).  ``rgb``,
    ``iuv`` (M,3,wh,wh) float32 planes as the device renderer gave them; a disc pixel is (255 * 255, 0, 0), an empty cell 0."""
    fig = np.zeros((rows * wh, cols * wh, 3))
    crop_s = None
    if crop is not None:
        crop_s = scaled(resize(crop, wh, dtype), dtype).transpose(1, 2, 0)
    for kind, row, col, m in panels:
        cell = fig[row * wh:(row + 1) * wh, col * wh:(col + 1) * wh]
        if kind == CROP:
            cell[:] = 0 if crop_s is None else crop_s
        elif kind in (RENDER, RENDER_OVER_CROP):
            cell[:] = scaled(np.asarray(rgb[m], dtype=np.float32), dtype).transpose(1, 2, 0)
            if kind == RENDER_OVER_CROP:
                background = np.rint(np.asarray(iuv[m][0], dtype=np.float32)) == 0
                cell[background] = 0 if crop_s is None else crop_s[background]
        elif kind == PROXY:
            p = np.asarray(proxy, dtype=dtype)
            total = np.zeros(p.shape[1:], dtype=dtype)
            for ch in range(p.shape[0]):
                total = total + p[ch]
            cell[:] = scaled(resize(total[None], wh, dtype), dtype)[0][:, :, None]
            if joints is not None:
                D = p.shape[-1]
                rr, cc = np.indices((wh, wh))
                for x, y in np.asarray(joints, dtype=np.float32).astype(np.float64):
                    jx, jy = x * wh / D, y * wh / D
                    if not (abs(jx) < 1e6 and abs(jy) < 1e6):
                        continue
                    disc = (cc - int(jx)) ** 2 + (rr - int(jy)) ** 2 <= 9
                    cell[disc] = (255.0 * 255.0, 0.0, 0.0)
        else:
            raise ValueError(kind)
    return fig


def byte_rule(got, s64, s32):
    """The +-1 rule: (largest byte difference from the float64 restatement, whether every differing byte lies where 255 v is within
    FACTOR x (the float32 twin's largest deviation on this input) of a half-integer, that tolerance)."""
    tol = FACTOR * float(np.abs(s32 - s64).max())
    diff = np.abs(got.astype(np.int64) - to_byte(s64).astype(np.int64))
    near = np.abs(s64 - np.floor(s64) - 0.5) <= tol
    return int(diff.max()), bool(near[diff > 0].all()), tol


# ---------------------------------------------------------------------------------------------------------------------------------
# warp and uncrop
# ---------------------------------------------------------------------------------------------------------------------------------
def uncrop_matrix(centre, side, wh):
    """utils/image_utils.py:197-201 in float32: (2,3) taking the render to the photograph; centre = (vertical, horizontal)."""
    f = np.float32
    owh, side = f(wh), f(side)
    oc = owh * f(0.5)
    M = np.zeros((2, 3), dtype=np.float32)
    M[0, 0] = side / owh
    M[1, 1] = side / owh
    M[0, 2] = f(centre[1]) - (side / owh) * oc
    M[1, 2] = f(centre[0]) - (side / owh) * oc
    return M


def warp_positions(M, H, W):
    """cv2.warpAffine's fixed-point source positions for a (H, W) destination (no WARP_INVERSE_MAP: M is inverted in float64):
    dict of nearest (ny, nx) and linear (sy, sx, fy, fx), fractions in thirty-seconds; (H, W) int64 arrays."""
    m = np.asarray(M, dtype=np.float32).astype(np.float64).reshape(-1).copy()
    D = m[0] * m[4] - m[1] * m[3]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = m[4] * D, m[0] * D
    m[0], m[1], m[3], m[4] = A11, m[1] * -D, m[3] * -D, A22
    b1 = -m[0] * m[2] - m[1] * m[5]
    b2 = -m[3] * m[2] - m[4] * m[5]
    cvr = lambda v: np.rint(np.clip(v, -2147483648.0, 2147483647.0)).astype(np.int64)
    x, y = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)
    ax, ay = cvr(m[0] * x * 1024.0)[None, :], cvr(m[3] * x * 1024.0)[None, :]
    rx, ry = cvr((m[1] * y + b1) * 1024.0)[:, None], cvr((m[4] * y + b2) * 1024.0)[:, None]
    wrap = lambda v: ((v + 2 ** 31) % 2 ** 32) - 2 ** 31                              # 32-bit int arithmetic
    nx, ny = wrap(rx + 512 + ax) >> 10, wrap(ry + 512 + ay) >> 10
    lx, ly = wrap(rx + 16 + ax) >> 5, wrap(ry + 16 + ay) >> 5
    return dict(ny=ny + 0 * nx, nx=nx + 0 * ny, sy=np.clip(ly >> 5, -32768, 32767) + 0 * lx, sx=np.clip(lx >> 5, -32768, 32767) + 0 * ly,
                fy=(ly & 31) + 0 * lx, fx=(lx & 31) + 0 * ly)


def _tap(src, y, x):
    h, w = src.shape[-2:]
    inside = (y >= 0) & (y < h) & (x >= 0) & (x < w)
    return np.where(inside, src[..., np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)], 0)


def warp_nearest(src, M, H, W):
    """(h, w) -> (H, W), INTER_NEAREST, constant border 0."""
    p = warp_positions(M, H, W)
    return _tap(np.asarray(src), p["ny"], p["nx"])


def warp_linear(src, M, H, W, dtype=np.float64):
    """(C, h, w) -> (C, H, W), INTER_LINEAR, constant border 0: v00 w00 + v01 w01 + v10 w10 + v11 w11 with the weights
    (1 - fy)(1 - fx), ... formed in float32 (OpenCV's table) and the sum in ``dtype``."""
    p = warp_positions(M, H, W)
    f = np.float32
    fx, fy = p["fx"].astype(f) * f(0.03125), p["fy"].astype(f) * f(0.03125)
    w = [((f(1) - fy) * (f(1) - fx)), ((f(1) - fy) * fx), (fy * (f(1) - fx)), (fy * fx)]
    w = [a.astype(dtype) for a in w]
    src = np.asarray(src, dtype=dtype)
    sy, sx = p["sy"], p["sx"]
    return _tap(src, sy, sx) * w[0] + _tap(src, sy, sx + 1) * w[1] + _tap(src, sy + 1, sx) * w[2] + _tap(src, sy + 1, sx + 1) * w[3]


def uncrop(rgb, iplane, image, centre, side, dtype=np.float64):
    """hps_vis_uncrop: (255 v before rounding (H, W, 3) float64, body mask (H, W)).  ``rgb`` (3,wh,wh), ``iplane`` (wh,wh), ``image``
    (3,H,W) float32."""
    wh = rgb.shape[-1]
    H, W = image.shape[1:]
    M = uncrop_matrix(centre, side, wh)
    body = warp_nearest(np.asarray(iplane, dtype=np.float32), M, H, W) != 0
    colour = scaled(warp_linear(np.asarray(rgb, dtype=np.float32), M, H, W, dtype), dtype).transpose(1, 2, 0)
    back = scaled(np.asarray(image, dtype=np.float32), np.float32).transpose(1, 2, 0)     # the device recovers it in float32: exact
    return np.where(body[:, :, None], colour, back), body


# ---------------------------------------------------------------------------------------------------------------------------------
# seeded inputs
# ---------------------------------------------------------------------------------------------------------------------------------
LAYOUTS = {
    # the eight-panel figure (:241-274) with render indices 0..5
    "2x4": (2, 4, 6, ((CROP, 0, 0, 0), (PROXY, 1, 0, 0), (RENDER_OVER_CROP, 0, 1, 0), (RENDER, 1, 1, 1), (RENDER, 0, 2, 2),
                      (RENDER, 1, 2, 3), (RENDER, 0, 3, 4), (RENDER, 1, 3, 5))),
    # the sample sheet (:324-330) with eight meshes: cells 16 and 17 stay empty
    "3x6": (3, 6, 16, tuple((RENDER_OVER_CROP if k % 2 == 0 else RENDER, k // 6, k % 6, k) for k in range(16))),
}


def compose_inputs(seed, wh, D, num_renders, channels=18, num_joints=17):
    """Random planes with the part-plane values that decide body against background: 0, 0.5 (background under round-to-even),
    0.50001, 1.5, 24 and -1; joints inside, on the border and outside the crop."""
    rs = np.random.RandomState(seed)
    rgb = rs.rand(num_renders, 3, wh, wh).astype(np.float32)
    iuv = rs.rand(num_renders, 3, wh, wh).astype(np.float32)
    iuv[:, 0] = rs.choice(np.float32([0.0, 0.5, 0.50001, 1.5, 24.0, -1.0, 0.49999, 2.5]), size=(num_renders, wh, wh))
    crop = rs.rand(3, D, D).astype(np.float32)
    proxy = (rs.rand(channels, D, D) * (rs.rand(channels, D, D) < 0.3)).astype(np.float32) * np.float32(0.2)
    joints = rs.uniform(0, D, (num_joints, 2)).astype(np.float32)
    joints[:6] = np.float32([[0, 0], [D - 0.01, D - 0.01], [-1.5, D / 2], [D / 2, D + 2.0], [-40, -40], [D / 2, -0.5]])
    return SimpleNamespace(rgb=rgb, iuv=iuv, crop=crop, proxy=proxy, joints=joints)


# boxes (centre (vertical, horizontal), side) on a (H, W) photograph: inside, half outside, larger than the image, smaller than wh
def uncrop_boxes(H, W):
    return {"inside": ((H / 2.0 + 0.3, W / 2.0 - 1.7), 0.6 * min(H, W)), "half_outside": ((H * 0.9, 2.25), 0.8 * min(H, W)),
            "larger": ((H / 2.0, W / 2.0), 1.7 * max(H, W)), "small": ((H / 3.0, W / 1.5), 7.3)}


def uncrop_inputs(seed, H, W, wh):
    """A uint8 photograph as the float image the front end holds, and render planes whose colours differ from it."""
    rs = np.random.RandomState(seed)
    u8 = rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
    image = (u8.transpose(2, 0, 1).astype(np.float32) / np.float32(255.0))
    rgb = rs.rand(3, wh, wh).astype(np.float32)
    rr, cc = np.indices((wh, wh))
    blob = ((rr - wh / 2.0) ** 2 + (cc - wh / 2.2) ** 2) <= (0.3 * wh) ** 2
    iplane = np.where(blob, rs.choice(np.float32([1.0, 2.3, 24.0, 0.4]), size=(wh, wh)), np.float32(0)).astype(np.float32)
    return SimpleNamespace(u8=u8, image=image, rgb=rgb, iplane=iplane)
