"""The training renderer's restatement and scenes (tests/test_render_host.py, tests/test_gpu_render.py, tests/dev/render_time.py,
tests/golden/make_render_golden.py).

``render`` restates include/hps.h's hps_render -- pytorch3d's hard rasteriser (blur_radius 0, one face per pixel, no perspective
correction, no culling, no clipping) and HardPhongShader as the reference configures them (renderers/pytorch3d_textured_renderer.py
:223-290, run_train.py:86-91) -- in numpy, operation by operation, in a chosen dtype: float64 is the yardstick the device is held to,
float32 is the run whose own deviation from float64 sets the tolerances.  pytorch3d cannot be imported here; the rules were written
from its rasteriser and shader sources and have not been checked against it (tests/golden/make_render_golden.py is that check, for a
machine that has it).

Scenes come from a seed, never from a file: closed bumpy UV-spheres (front and back faces overlap in depth, the poles have a high
vertex degree), optionally two that interpenetrate, a ``verts_map`` with duplicates, random ``verts_iuv`` / ``verts_uv`` / textures /
vertex colours, cameras near MEAN_CAM_T with f = 300 W / 256.
"""
import functools
from types import SimpleNamespace

import numpy as np

EPS = 1e-8
NORM_EPS = 1e-6
MEAN_CAM_T = (0.0, -0.2, 2.5)
FACTOR = 16.0                    # tolerance = FACTOR * (float32 restatement's largest deviation from float64 on the scene)
NEAR_TIE_CAP = 0.01              # differing face indices: at most this share of a scene's covered pixels, near-ties only


# ---------------------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------------------
def vertex_faces(faces, num_verts):
    """Vertex-to-faces table in compressed sparse rows: (offsets (Nd+1,), flat face list); a vertex's faces in increasing face index
    (a face naming the vertex twice is listed twice)."""
    corner = np.asarray(faces, dtype=np.int64).reshape(-1)
    order = np.argsort(corner, kind="stable")
    offsets = np.zeros(num_verts + 1, dtype=np.int64)
    np.cumsum(np.bincount(corner, minlength=num_verts), out=offsets[1:])
    return offsets, (order // 3)


def _normalise(v, dt):
    n = np.sqrt(v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2])
    return v / np.maximum(n, dt(NORM_EPS))[..., None]


def _per_image(a, B, dtype):
    a = np.asarray(a, dtype=dtype)
    return np.broadcast_to(a.reshape(-1, a.shape[-1]), (B, a.shape[-1]))


def project(scene, dtype):
    """(world (B,Nd,3), ndc x, ndc y, z (B,Nd)) of the DensePose vertices."""
    v = np.asarray(scene.vertices, dtype=dtype)[:, scene.verts_map]
    B = v.shape[0]
    t, s = _per_image(scene.cam_t, B, dtype), _per_image(scene.scale, B, dtype)
    X, Y, Z = -(v[..., 0] + t[:, None, 0]), -(v[..., 1] + t[:, None, 1]), v[..., 2] + t[:, None, 2]
    xn, yn = s[:, None, 0] * X, s[:, None, 1] * Y
    if scene.projection == "perspective":
        xn, yn = xn / Z, yn / Z
    return v, xn, yn, Z


def vertex_normals(world, faces, dt):
    """Sum over each vertex's faces, in the table's order, of cross(v1 - v0, v2 - v0); then / max(|n|, 1e-6)."""
    B, Nd = world.shape[:2]
    v0, v1, v2 = (world[:, faces[:, k]] for k in range(3))
    a, b = v1 - v0, v2 - v0
    cross = np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                      a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)
    offsets, flat = vertex_faces(faces, Nd)
    degree = offsets[1:] - offsets[:-1]
    n = np.zeros_like(world)
    for k in range(int(degree.max()) if Nd else 0):
        sel = np.nonzero(degree > k)[0]
        n[:, sel] = n[:, sel] + cross[:, flat[offsets[sel] + k]]
    return _normalise(n, dt)


def rasterise(scene, dtype, xn, yn, Z):
    """pix_to_face (B,W,W) int64, zbuf (B,W,W), bary (B,W,W,3): faces walked in index order, replaced on a strictly smaller depth."""
    dt = np.dtype(dtype).type
    faces, W = scene.faces, scene.W
    B, F = xn.shape[0], faces.shape[0]
    pix = dt(1) - (2 * np.arange(W) + 1).astype(dtype) / dt(W)
    pix_to_face = np.full((B, W, W), -1, dtype=np.int64)
    zbuf = np.full((B, W, W), np.inf, dtype=dtype)
    bary = np.full((B, W, W, 3), -1, dtype=dtype)
    eps = dt(EPS)
    for b in range(B):
        x, y, z = (q[b][faces] for q in (xn, yn, Z))                                  # (F,3)
        area = (x[:, 2] - x[:, 0]) * (y[:, 1] - y[:, 0]) - (y[:, 2] - y[:, 0]) * (x[:, 1] - x[:, 0])
        keep = ~(np.abs(area) <= eps) & ~(z.max(axis=1) < eps)
        # pixels a face can cover, generously (float64, one pixel of margin): which pixels are LOOKED at, never coverage
        with np.errstate(invalid="ignore", over="ignore"):
            def span(q):
                q = np.nan_to_num(q.astype(np.float64), nan=0.0, posinf=1e9, neginf=-1e9)
                lo = np.floor((W * (1 - q.max(axis=1)) - 1) / 2) - 1
                hi = np.ceil((W * (1 - q.min(axis=1)) - 1) / 2) + 1
                bad = ~np.isfinite(x).all(axis=1) | ~np.isfinite(y).all(axis=1)
                lo, hi = np.where(bad, 0, lo), np.where(bad, W - 1, hi)
                return np.clip(lo, 0, W).astype(np.int64), np.clip(hi, -1, W - 1).astype(np.int64)
            c_lo, c_hi = span(x)
            r_lo, r_hi = span(y)
        keep &= (c_lo <= c_hi) & (r_lo <= r_hi)
        for f in np.nonzero(keep)[0]:
            rs, cs = slice(r_lo[f], r_hi[f] + 1), slice(c_lo[f], c_hi[f] + 1)
            px, py = pix[cs][None, :], pix[rs][:, None]
            (x0, x1, x2), (y0, y1, y2), (z0, z1, z2) = x[f], y[f], z[f]
            den = area[f] + eps
            with np.errstate(all="ignore"):
                w0 = ((px - x1) * (y2 - y1) - (py - y1) * (x2 - x1)) / den
                w1 = ((px - x2) * (y0 - y2) - (py - y2) * (x0 - x2)) / den
                w2 = ((px - x0) * (y1 - y0) - (py - y0) * (x1 - x0)) / den
                pz = w0 * z0 + w1 * z1 + w2 * z2
                win = (w0 > 0) & (w1 > 0) & (w2 > 0) & ~(pz < 0) & (pz < zbuf[b, rs, cs])
            if win.any():
                zbuf[b, rs, cs][win] = pz[win]
                pix_to_face[b, rs, cs][win] = f
                bw = bary[b, rs, cs]
                bw[win] = np.stack([w0, w1, w2], axis=-1)[win]
    zbuf[pix_to_face < 0] = -1
    return pix_to_face, zbuf, bary


def _interp(w, attr):
    """sum of w attr over the three corners, left to right: w (N,3), attr (N,3,C)."""
    return w[:, 0, None] * attr[:, 0] + w[:, 1, None] * attr[:, 1] + w[:, 2, None] * attr[:, 2]


def shade(scene, dtype, world, pix_to_face, bary):
    """iuv, rgb (B,W,W,3)."""
    dt = np.dtype(dtype).type
    B, W = pix_to_face.shape[0], scene.W
    faces = scene.faces
    iuv = np.zeros((B, W, W, 3), dtype=dtype)
    rgb = np.zeros((B, W, W, 3), dtype=dtype)
    normals = vertex_normals(world, faces, dt)
    verts_iuv = np.asarray(scene.verts_iuv, dtype=dtype)
    lights = [_per_image(scene.lights[k], B, dtype) for k in ("location", "ambient_color", "diffuse_color", "specular_color")]
    cam_t = _per_image(scene.cam_t, B, dtype)
    for b in range(B):
        rr, cc = np.nonzero(pix_to_face[b] >= 0)
        if rr.size == 0:
            continue
        corners = faces[pix_to_face[b, rr, cc]]                                     # (N,3)
        w = bary[b, rr, cc]
        iuv[b, rr, cc] = _interp(w, verts_iuv[corners])
        if scene.verts_features is not None:
            texel = _interp(w, np.asarray(scene.verts_features, dtype=dtype)[b][scene.verts_map][corners])
        else:
            tex = np.asarray(scene.texture, dtype=dtype)[b]
            Ht, Wt = tex.shape[:2]
            uv = _interp(w, np.asarray(scene.verts_uv, dtype=dtype)[corners])
            x = np.minimum(np.maximum(uv[:, 0] * dt(Wt - 1), dt(0)), dt(Wt - 1))
            y = np.minimum(np.maximum((dt(1) - uv[:, 1]) * dt(Ht - 1), dt(0)), dt(Ht - 1))
            xf, yf = np.floor(x), np.floor(y)
            x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
            x1, y1 = np.minimum(x0 + 1, Wt - 1), np.minimum(y0 + 1, Ht - 1)
            fx, fy = (x - xf)[:, None], (y - yf)[:, None]
            lerp = lambda p, q, t: p + t * (q - p)
            texel = lerp(lerp(tex[y0, x0], tex[y0, x1], fx), lerp(tex[y1, x0], tex[y1, x1], fx), fy)
        n = _normalise(_interp(w, normals[b][corners]), dt)
        P = _interp(w, world[b][corners])
        L = _normalise(lights[0][b][None, :] - P, dt)
        view = _normalise(-cam_t[b][None, :] - P, dt)
        nl = n[:, 0] * L[:, 0] + n[:, 1] * L[:, 1] + n[:, 2] * L[:, 2]
        reflect = -L + dt(2) * nl[:, None] * n
        s = np.maximum(view[:, 0] * reflect[:, 0] + view[:, 1] * reflect[:, 1] + view[:, 2] * reflect[:, 2], dt(0)) * (nl > 0).astype(dtype)
        for _ in range(6):                                                          # shininess 64
            s = s * s
        diffuse = lights[2][b][None, :] * np.maximum(nl, dt(0))[:, None]
        rgb[b, rr, cc] = np.minimum(dt(1), (lights[1][b][None, :] + diffuse) * texel + lights[3][b][None, :] * s[:, None])
    return iuv, rgb


def render(scene, dtype=np.float64):
    """dict of pix_to_face (B,W,W) int64, zbuf (B,W,W), bary, iuv, rgb (B,W,W,3) in ``dtype``."""
    world, xn, yn, Z = project(scene, dtype)
    pix_to_face, zbuf, bary = rasterise(scene, dtype, xn, yn, Z)
    iuv, rgb = shade(scene, dtype, world, pix_to_face, bary)
    return dict(pix_to_face=pix_to_face, zbuf=zbuf, bary=bary, iuv=iuv, rgb=rgb)


def face_at(scene, face, dtype=np.float64):
    """(w (B,W,W,3), pz (B,W,W)) of face index ``face`` (B,W,W) evaluated at every pixel -- the near-tie rule's evaluation of the
    device's face in float64.  Pixels with face < 0 give nan."""
    dt = np.dtype(dtype).type
    _, xn, yn, Z = project(scene, dtype)
    B, W = face.shape[0], scene.W
    pix = dt(1) - (2 * np.arange(W) + 1).astype(dtype) / dt(W)
    px, py = pix[None, None, :], pix[None, :, None]
    corners = scene.faces[np.maximum(face, 0)]                                      # (B,W,W,3)
    bi = np.arange(B)[:, None, None]
    x0, x1, x2 = (xn[bi, corners[..., k]] for k in range(3))
    y0, y1, y2 = (yn[bi, corners[..., k]] for k in range(3))
    z0, z1, z2 = (Z[bi, corners[..., k]] for k in range(3))
    den = (x2 - x0) * (y1 - y0) - (y2 - y0) * (x1 - x0) + dt(EPS)
    with np.errstate(all="ignore"):
        w0 = ((px - x1) * (y2 - y1) - (py - y1) * (x2 - x1)) / den
        w1 = ((px - x2) * (y0 - y2) - (py - y2) * (x0 - x2)) / den
        w2 = ((px - x0) * (y1 - y0) - (py - y0) * (x1 - x0)) / den
    w = np.stack([w0, w1, w2], axis=-1)
    pz = w0 * z0 + w1 * z1 + w2 * z2
    w[face < 0] = np.nan
    pz = np.where(face < 0, np.nan, pz)
    return w, pz


# ---------------------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------------------
def uv_sphere(rings, segments, rng, radius=0.5, centre=(0.0, 0.0, 0.0), bump=0.15):
    """A closed UV-sphere of ``rings`` latitude rings and ``segments`` longitudes with a smooth bump and a little noise on the radius:
    (vertices (2 + rings segments, 3) float32, faces (2 segments rings, 3) int64), wound outwards.  The two poles have degree
    ``segments``."""
    theta = np.pi * (np.arange(rings) + 1) / (rings + 1)
    phi = 2 * np.pi * np.arange(segments) / segments
    th, ph = np.meshgrid(theta, phi, indexing="ij")
    r = radius * (1 + bump * np.sin(3 * th + 0.3) * np.cos(2 * ph + 0.7) + 0.02 * rng.standard_normal(th.shape))
    ring = np.stack([r * np.sin(th) * np.cos(ph), r * np.cos(th), r * np.sin(th) * np.sin(ph)], axis=-1).reshape(-1, 3)
    verts = np.concatenate([[[0, radius, 0]], ring, [[0, -radius, 0]]]) + np.asarray(centre)
    idx = lambda i, j: 1 + i * segments + (j % segments)
    south = 1 + rings * segments
    faces = []
    for j in range(segments):
        faces.append((0, idx(0, j + 1), idx(0, j)))
    for i in range(rings - 1):
        for j in range(segments):
            faces.append((idx(i, j), idx(i, j + 1), idx(i + 1, j)))
            faces.append((idx(i, j + 1), idx(i + 1, j + 1), idx(i + 1, j)))
    for j in range(segments):
        faces.append((south, idx(rings - 1, j), idx(rings - 1, j + 1)))
    return verts.astype(np.float32), np.asarray(faces, dtype=np.int64)


def make_scene(seed, B, W, rings, segments, num_faces=None, two=False, projection="perspective", route="uv", tex_hw=(24, 16),
               lights_per_image=False, scale_per_image=False, shift=None, duplicates=0.15):
    """A seeded scene.  ``num_faces``: keep the first num_faces faces (an open mesh).  ``two``: a second, smaller sphere that
    interpenetrates the first.  ``shift`` (B,2): added to cam_t's x and y -- meshes partly or wholly off the screen.  ``route``: 'uv'
    (texture through verts_uv) or 'vertex' (verts_features).  All float arrays float32."""
    rng = np.random.RandomState(seed)
    verts, faces = uv_sphere(rings, segments, rng)
    if two:
        v2, f2 = uv_sphere(max(2, rings // 2), max(3, segments // 2), rng, radius=0.35, centre=(0.3, 0.1, -0.25))
        faces = np.concatenate([faces, f2 + len(verts)])
        verts = np.concatenate([verts, v2])
    if num_faces is not None:
        assert num_faces <= len(faces)
        faces = faces[:num_faces]
    V = len(verts)
    # per-image pose: a small rotation about y and x, a little scaling
    vertices = np.zeros((B, V, 3), dtype=np.float32)
    for b in range(B):
        ay, ax = rng.uniform(-0.6, 0.6, 2)
        Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
        Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
        vertices[b] = (verts @ (Ry @ Rx).T * rng.uniform(0.9, 1.1)).astype(np.float32)
    # DensePose-style vertex duplication: every SMPL vertex at least once, some twice or more, in shuffled order
    ndup = int(round(duplicates * V))
    verts_map = np.concatenate([np.arange(V), rng.randint(0, V, ndup)])
    rng.shuffle(verts_map)
    Nd = len(verts_map)
    copies = [[] for _ in range(V)]
    for i, v in enumerate(verts_map):
        copies[v].append(i)
    faces_dp = np.array([[copies[v][rng.randint(len(copies[v]))] for v in face] for face in faces], dtype=np.int64)
    verts_iuv = np.concatenate([rng.randint(1, 25, (Nd, 1)).astype(np.float32), rng.rand(Nd, 2).astype(np.float32)], axis=1)
    verts_uv = rng.uniform(-0.05, 1.05, (Nd, 2)).astype(np.float32)                  # a few outside the map: the border clamp
    cam_t = (np.asarray(MEAN_CAM_T) + np.concatenate([rng.normal(0, 0.05, (B, 2)), rng.uniform(-0.5, 0.5, (B, 1))], axis=1))
    if shift is not None:
        cam_t[:, :2] += np.asarray(shift)
    if projection == "perspective":
        scale = np.full((1, 2), 2 * (300.0 * W / 256.0) / W)
    else:
        scale = rng.uniform(0.7, 1.1, (B, 2)) if scale_per_image else np.full((1, 2), 0.9)
    nl = B if lights_per_image else 1
    direction = rng.standard_normal((nl, 3))
    lights = dict(location=(direction / np.linalg.norm(direction, axis=1, keepdims=True) * rng.uniform(0.5, 3.0, (nl, 1))).astype(np.float32),
                  ambient_color=np.repeat(rng.uniform(0.2, 0.8, (nl, 1)), 3, axis=1).astype(np.float32),
                  diffuse_color=np.repeat(rng.uniform(0.2, 0.8, (nl, 1)), 3, axis=1).astype(np.float32),
                  specular_color=np.repeat(rng.uniform(0.2, 0.8, (nl, 1)), 3, axis=1).astype(np.float32))
    texture = rng.rand(B, tex_hw[0], tex_hw[1], 3).astype(np.float32) if route == "uv" else None
    verts_features = rng.rand(B, V, 3).astype(np.float32) if route == "vertex" else None
    return SimpleNamespace(B=B, W=W, V=V, Nd=Nd, vertices=vertices, verts_map=verts_map, faces=faces_dp, verts_iuv=verts_iuv,
                           verts_uv=verts_uv, texture=texture, verts_features=verts_features, cam_t=cam_t.astype(np.float32),
                           projection=projection, scale=scale.astype(np.float32), lights=lights)


def flat_scene(W, vertices, faces, scale=1.0, cam_t=(0.0, 0.0, 0.0), projection="orthographic", verts_iuv=None):
    """A closed-form scene: ``vertices`` (V,3) given so that the NDC position is (-x, -y) under the orthographic camera with scale 1
    and no translation; identity verts_map, constant white texture, ambient light only."""
    vertices = np.asarray(vertices, dtype=np.float32)[None]
    V = vertices.shape[1]
    if verts_iuv is None:
        verts_iuv = np.stack([np.arange(V) % 24 + 1, (np.arange(V) % 4) / 4.0, (np.arange(V) % 8) / 8.0], axis=1)
    lights = dict(location=np.array([[0, 0, -2]], np.float32), ambient_color=np.full((1, 3), 0.5, np.float32),
                  diffuse_color=np.zeros((1, 3), np.float32), specular_color=np.zeros((1, 3), np.float32))
    return SimpleNamespace(B=1, W=W, V=V, Nd=V, vertices=vertices, verts_map=np.arange(V), faces=np.asarray(faces, dtype=np.int64).reshape(-1, 3),
                           verts_iuv=np.asarray(verts_iuv, dtype=np.float32), verts_uv=np.full((V, 2), 0.5, np.float32),
                           texture=np.ones((1, 2, 2, 3), np.float32), verts_features=None,
                           cam_t=np.asarray(cam_t, dtype=np.float32)[None], projection=projection,
                           scale=np.full((1, 2), scale, np.float32), lights=lights)


def ndc_vertices(points):
    """World vertices whose orthographic NDC position (scale 1, no translation) is ``points`` (x_ndc, y_ndc, z)."""
    p = np.asarray(points, dtype=np.float64)
    return np.stack([-p[:, 0], -p[:, 1], p[:, 2]], axis=1)


# Closed-form scenes on an 8 x 8 image: pixel centres at odd multiples of 1/8, vertices at multiples of 1/4 -- every edge function,
# quotient's numerator and depth below is exact in float32, so float32, float64 and the device agree to the bit on coverage.
def closed_form_scenes():
    S = {}
    # two triangles sharing the diagonal x = y of the square [-1, 1]^2 (pixel centres with row == col lie ON it)
    S["shared_edge"] = flat_scene(8, ndc_vertices([(-1, -1, 1), (1, -1, 1), (1, 1, 1), (-1, 1, 1)]), [(0, 1, 2), (0, 2, 3)])
    # the same triangle twice, at the same depth: the lower index wins everywhere
    S["coincident"] = flat_scene(8, ndc_vertices([(-1, -1, 1), (1, -1, 1), (1, 1, 1), (-1, -1, 1), (1, -1, 1), (1, 1, 1)]),
                                 [(3, 4, 5), (0, 1, 2)])
    # a face with every z < 0 in front of (nearer than) a visible one: skipped
    S["behind"] = flat_scene(8, ndc_vertices([(-1, -1, -1), (1, -1, -1), (1, 1, -1), (-1, -1, 2), (1, -1, 2), (1, 1, 2)]),
                             [(0, 1, 2), (3, 4, 5)])
    # a zero-area face (three collinear vertices) beside a proper one
    S["zero_area"] = flat_scene(8, ndc_vertices([(-1, -1, 1), (0, 0, 1), (1, 1, 1), (-1, -1, 2), (1, -1, 2), (1, 1, 2)]),
                                [(0, 1, 2), (3, 4, 5)])
    # one triangle over the whole image
    S["whole_image_exact"] = flat_scene(8, ndc_vertices([(-4, -2, 1), (4, -2, 1.5), (0, 6, 2)]), [(0, 1, 2)])
    return S


# name -> make_scene arguments.  Image sides 16, 40 (no multiple of a 16-pixel tile), 64; 13, 257 and 2400 faces (remainders of a
# 256-face chunk: 13, 1 and 96; of a 64-face chunk: 13, 1 and 32); both projections, both texel routes, lights shared and per image, meshes partly / wholly off the screen.
CASES = {
    "w16_f13_b1": dict(seed=1, B=1, W=16, rings=3, segments=4, num_faces=13),
    "w40_f257_b3": dict(seed=2, B=3, W=40, rings=11, segments=12, num_faces=257, lights_per_image=True,
                        shift=[(0.0, 0.0), (0.8, 0.3), (6.0, 0.0)]),                 # image 1 partly, image 2 wholly off the screen
    "w64_f2400_b3_ortho": dict(seed=3, B=3, W=64, rings=30, segments=40, projection="orthographic", scale_per_image=True,
                               shift=[(0.0, 0.2), (0.9, 0.2), (0.0, 0.2)]),
    "w64_two_b1_vertex": dict(seed=4, B=1, W=64, rings=14, segments=16, two=True, route="vertex"),
    "w40_f257_b1_bigtex": dict(seed=5, B=1, W=40, rings=11, segments=12, num_faces=257, tex_hw=(1200, 800)),
    "w64_f2400_b3_vertex_ortho": dict(seed=6, B=3, W=64, rings=30, segments=40, projection="orthographic", route="vertex",
                                      lights_per_image=True, shift=[(0.0, 0.2)] * 3),
    # 36 pixels: no multiple of the rasteriser's 8-pixel tile either; the mesh reaches the partial tiles at the right and bottom edges
    "w36_f257_b2": dict(seed=10, B=2, W=36, rings=11, segments=12, num_faces=257, shift=[(0.0, 0.75), (0.7, 0.5)]),
    # 2400 faces on 16 x 16 pixels: every tile's record list overflows again and again
    "w16_f2400_b1": dict(seed=9, B=1, W=16, rings=30, segments=40),
    "w256_smpl_b2": dict(seed=7, B=2, W=256, rings=83, segments=83, num_faces=13774, duplicates=938.0 / 6891.0, tex_hw=(24, 16)),
}


def whole_image_scene():
    """One large triangle over a 40-pixel image (every tile walks it), perspective camera."""
    sc = make_scene(8, 1, 40, 3, 4, num_faces=1)
    sc.vertices[0, sc.verts_map[sc.faces[0]]] = np.array([[-6, -4, 0.2], [6, -4, -0.1], [0, 8, 0.4]], dtype=np.float32)
    return sc


@functools.lru_cache(maxsize=None)
def reference(name):
    """(scene, float32 restatement, float64 restatement) of a case, computed once and shared: callers must not modify them."""
    if name in CASES:
        scene = make_scene(**CASES[name])
    elif name == "whole_image":
        scene = whole_image_scene()
    else:
        scene = closed_form_scenes()[name]
    return scene, render(scene, np.float32), render(scene, np.float64)


def agreement(scene, got, r64):
    """Pixels where ``got``'s face differs from the float64 one: (agree mask (B,W,W), count of differing, count of covered,
    w_min (over the differing pixels, of got's face in float64), pz excess over the float64 winner)."""
    agree = got["pix_to_face"] == r64["pix_to_face"]
    covered = int((r64["pix_to_face"] >= 0).sum())
    diff = ~agree
    if not diff.any():
        return agree, 0, covered, np.inf, -np.inf
    # a pixel the yardstick leaves empty has no winner to beat: its depth counts as +inf; a pixel ``got`` leaves empty where the
    # yardstick has a face has no face to evaluate and fails both tests (-inf, +inf)
    face = np.where(diff, got["pix_to_face"], -1)
    w, pz = face_at(scene, face)
    z_win = np.where(r64["pix_to_face"] >= 0, r64["zbuf"], np.inf)
    w_min = np.where(face < 0, -np.inf, w.min(axis=-1))[diff]
    excess = np.where(face < 0, np.inf, pz - z_win)[diff]
    return agree, int(diff.sum()), covered, float(np.min(w_min)), float(np.max(excess))


def deviations(scene, r32, r64):
    """The float32 restatement's largest deviation from float64, per quantity, over the pixels where their faces agree."""
    agree = (r32["pix_to_face"] == r64["pix_to_face"]) & (r64["pix_to_face"] >= 0)
    dev = {}
    for k in ("zbuf", "bary", "iuv", "rgb"):
        d = np.abs(r32[k].astype(np.float64) - r64[k])
        dev[k] = float(d[agree].max()) if agree.any() else 0.0
    return dev
