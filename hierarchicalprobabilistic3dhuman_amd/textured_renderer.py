"""The training step's renderer on the device (renderers/pytorch3d_textured_renderer.py; train/train_poseMF_shapeGaussian_net.py
:186-196) and the three small samplers the step calls beside it (utils/augmentation/lighting_augmentation.py, smpl_augmentation.py
:16-21, cam_augmentation.py).

``TexturedIUVRenderer`` keeps the reference's constructor and ``forward`` and runs csrc/render.hip (include/hps.h: hps_render): a hard
nearest-face rasteriser with Phong shading, three launches, forward only -- what the reference's defaults ask of pytorch3d
(run_train.py:86-91: blur_radius 0, one face per pixel, no perspective correction, no culling, no clipping, HardPhongShader under
no_grad).  Any other setting raises NotImplementedError; there is no pytorch3d behind this module and no CPU path.

The images are stored planar, (B,3,H,W), and returned as (B,H,W,3) views of that storage, so the training loop's
``.permute(0, 3, 1, 2).contiguous()`` copies nothing.  Output buffers are owned per batch size and overwritten by the next call.

``silhouette_counts`` is the evaluation's use of the same rasteriser (evaluate/evaluate_poseMF_shapeGaussian_net.py:143-155, 192-203;
include/hps.h: hps_silhouette_iou): the silhouette of every mesh compared with a target and counted, without an image in between.
"""
import numpy as np
import torch

from . import _capi

_DEFAULT_CAM_R = ((-1.0, 0.0, 0.0), (0.0, -1.0, 0.0), (0.0, 0.0, 1.0))


def preprocess_densepose_UV(uv_path_or_dict, batch_size):
    """:22-70.  ``uv_path_or_dict``: the processed DensePose ``.mat`` file, or its fields already loaded (All_FaceIndices (F,1),
    All_Faces (F,3) and All_vertices (1,Nd), both 1-based, All_U_norm, All_V_norm (Nd,1)).  Returns (verts_uv_offset (bs,Nd,2),
    verts_iuv (bs,Nd,3), verts_map (Nd,) int64, faces_densepose (bs,F,3) int64), the batch dimension expanded.

    The texture atlas is a grid of 4 columns by 6 rows of part maps, parts counted down the rows first.  A vertex's UV is moved into
    the cell of the part of the FIRST face that names it, once (vertices are shared at part boundaries); its part label in
    verts_iuv is the part of the LAST face that names it."""
    if isinstance(uv_path_or_dict, dict):
        dp = uv_path_or_dict
    else:
        from scipy.io import loadmat
        dp = loadmat(uv_path_or_dict)
    faces_parts = torch.as_tensor(np.asarray(dp["All_FaceIndices"], dtype=np.float32)).reshape(-1)
    faces = torch.from_numpy((np.asarray(dp["All_Faces"]) - 1).astype(np.int64))
    verts_map = torch.from_numpy(np.asarray(dp["All_vertices"])[0].astype(np.int64)) - 1
    u = torch.as_tensor(np.asarray(dp["All_U_norm"], dtype=np.float32)).reshape(-1, 1)
    v = torch.as_tensor(np.asarray(dp["All_V_norm"], dtype=np.float32)).reshape(-1, 1)
    Nd, F = u.shape[0], faces.shape[0]
    cols, rows = 4, 6
    corner = faces.reshape(-1)
    face_of_corner = torch.arange(F).repeat_interleave(3)
    first = torch.full((Nd,), 3 * F, dtype=torch.int64).scatter_reduce(0, corner, torch.arange(3 * F), reduce="amin")
    last = torch.full((Nd,), -1, dtype=torch.int64).scatter_reduce(0, corner, torch.arange(3 * F), reduce="amax")
    used = last >= 0
    part_first = faces_parts[face_of_corner[first[used]]].long()
    # part p (1-based) sits in column (p - 1) // rows, row (p - 1) % rows of the atlas; the cell's origin as np.linspace gives it
    off_u = torch.as_tensor(np.linspace(0, 1, cols, endpoint=False), dtype=torch.float32)[(part_first - 1) // rows]
    off_v = torch.as_tensor(np.linspace(0, 1, rows, endpoint=False), dtype=torch.float32)[(part_first - 1) % rows]
    u_off, v_off = u.clone(), v.clone()
    u_off[used, 0] = u[used, 0] / cols + off_u
    v_off[used, 0] = (1 - v[used, 0]) / rows + off_v             # each part map is stored upside down
    vertex_parts = torch.zeros(Nd)
    vertex_parts[used] = faces_parts[face_of_corner[last[used]]]
    v, v_off = 1 - v, 1 - v_off
    verts_uv_offset = torch.cat([u_off, v_off], dim=1)[None].expand(batch_size, -1, -1)
    verts_iuv = torch.cat([vertex_parts[:, None], u, v], dim=1)[None].expand(batch_size, -1, -1)
    return verts_uv_offset, verts_iuv, verts_map, faces[None].expand(batch_size, -1, -1)


def vertex_faces_csr(faces, num_verts):
    """Vertex-to-faces table in compressed sparse rows (include/hps.h: vf_offsets, vf_faces), int32: a vertex's faces in increasing
    face index.  The order is the order the device adds the face normals in."""
    corner = np.asarray(faces, dtype=np.int64).reshape(-1)
    offsets = np.zeros(num_verts + 1, dtype=np.int64)
    np.cumsum(np.bincount(corner, minlength=num_verts), out=offsets[1:])
    return offsets.astype(np.int32), (np.argsort(corner, kind="stable") // 3).astype(np.int32)


class TexturedIUVRenderer(torch.nn.Module):
    """:73-290 over hps_render.  ``densepose_uv``: the processed DensePose file's path, its loaded dict, or the four results of
    preprocess_densepose_UV (the reference reads configs.paths.DP_UV_PROCESSED_FILE, an asset this package does not ship)."""

    def __init__(self, device, batch_size, img_wh=256, cam_t=None, cam_R=None, projection_type="perspective",
                 perspective_focal_length=300, orthographic_scale=0.9, blur_radius=0.0, faces_per_pixel=1, bin_size=None,
                 max_faces_per_bin=None, perspective_correct=False, cull_backfaces=False, clip_barycentric_coords=None,
                 render_rgb=False, light_t=((0.0, 0.0, -2.0),), light_ambient_color=((0.5, 0.5, 0.5),),
                 light_diffuse_color=((0.3, 0.3, 0.3),), light_specular_color=((0.2, 0.2, 0.2),),
                 background_color=(0.0, 0.0, 0.0), densepose_uv=None):
        super().__init__()
        for what, bad in (("blur_radius != 0", blur_radius != 0), ("faces_per_pixel != 1", faces_per_pixel != 1),
                          ("perspective_correct=True", bool(perspective_correct)), ("cull_backfaces=True", bool(cull_backfaces)),
                          ("clip_barycentric_coords=True", bool(clip_barycentric_coords)),
                          ("a background colour other than black", tuple(float(c) for c in background_color) != (0.0, 0.0, 0.0))):
            if bad:
                raise NotImplementedError("TexturedIUVRenderer: %s is not implemented (the device renderer is the hard, one-face-"
                                          "per-pixel rasteriser the training step uses)" % what)
        if cam_R is not None and not torch.equal(torch.as_tensor(cam_R).float().cpu().reshape(-1, 3, 3),
                                                 torch.tensor(_DEFAULT_CAM_R).expand(torch.as_tensor(cam_R).reshape(-1, 3, 3).shape[0], 3, 3)):
            raise NotImplementedError("TexturedIUVRenderer: only the default camera rotation diag(-1, -1, 1) is implemented")
        if projection_type not in ("perspective", "orthographic"):
            raise ValueError("Invalid projection type: %s" % projection_type)
        if densepose_uv is None:
            raise _capi.HpsError("TexturedIUVRenderer needs densepose_uv: the processed DensePose UV file (UV_Processed.mat), its "
                                 "loaded dict, or preprocess_densepose_UV's results")
        device = torch.device(device)
        if device.type != "cuda":
            raise _capi.HpsError("TexturedIUVRenderer runs on a HIP device only; this package has no CPU path")
        self.device, self.batch_size, self.img_wh = device, int(batch_size), int(img_wh)
        self.projection_type, self.render_rgb = projection_type, bool(render_rgb)
        # bin_size / max_faces_per_bin only steer pytorch3d's coarse pass and do not change its output
        uv = densepose_uv if isinstance(densepose_uv, (tuple, list)) else preprocess_densepose_UV(densepose_uv, batch_size)
        verts_uv_offset, verts_iuv, verts_map, faces = uv
        self.verts_uv_offset, self.verts_iuv = verts_uv_offset.to(device), verts_iuv.to(device)
        self.verts_map, self.faces_densepose = verts_map.to(device), faces.to(device)
        faces0, map0 = faces[0].cpu().numpy(), verts_map.cpu().numpy()
        self._Nd, self._F, self._map_max = int(map0.shape[0]), int(faces0.shape[0]), int(map0.max())
        if self._F < 1 or faces0.min() < 0 or faces0.max() >= self._Nd or map0.min() < 0:
            raise _capi.HpsError("faces_densepose must index the %d DensePose vertices, verts_map must not be negative" % self._Nd)
        offsets, flat = vertex_faces_csr(faces0, self._Nd)
        i32 = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.int32).to(device)
        f32 = lambda a: torch.as_tensor(a, dtype=torch.float32).contiguous().to(device)
        self._faces, self._map, self._vf_offsets, self._vf_faces = i32(faces0), i32(map0), i32(offsets), i32(flat)
        self._iuv, self._uv = f32(verts_iuv[0]), f32(verts_uv_offset[0])
        self._cam_t = f32([[0.0, 0.2, 2.5]]) if cam_t is None else self._per_image(cam_t, 3, "cam_t")
        s = 2.0 * float(perspective_focal_length) / self.img_wh if projection_type == "perspective" else float(orthographic_scale)
        self._scale = f32([[s, s]])
        self._lights = [f32(np.asarray(c, dtype=np.float32).reshape(-1, 3)) for c in
                        (light_t, light_ambient_color, light_diffuse_color, light_specular_color)]
        self._bufs = {}
        self._silhouette_bufs = {}

    def to(self, device):
        if torch.device(device) != self.device:
            raise _capi.HpsError("TexturedIUVRenderer was built for %s" % self.device)
        return self

    def _per_image(self, t, width, what):
        """(rows, width) float32 contiguous on the device, rows 1 (shared) or the batch size."""
        _capi.require_device(t, what)
        t = _capi.f32c(t.reshape(-1, width) if t.dim() != 2 else t)
        if t.dim() != 2 or t.shape[1] != width:
            raise _capi.HpsError("%s must be (B,%d) or (1,%d)" % (what, width, width))
        return t

    def _outputs(self, B, fragments, train):
        bufs = self._bufs.get(B)
        if bufs is None:
            W, dev = self.img_wh, self.device
            ws = torch.empty(_capi.query_workspace(_capi.WS_RENDER, B, self._Nd, self._F) // 4, device=dev, dtype=torch.float32)
            bufs = dict(ws=ws, iuv=torch.empty(B, 3, W, W, device=dev), depth=torch.empty(B, W, W, device=dev),
                        rgb=torch.empty(B, 3, W, W, device=dev) if self.render_rgb else None, pix_to_face=None, bary=None,
                        iuv_train=None)
            self._bufs[B] = bufs
        W, dev = self.img_wh, self.device
        if fragments and bufs["bary"] is None:
            bufs["pix_to_face"] = torch.empty(B, W, W, device=dev, dtype=torch.int32)
            bufs["bary"] = torch.empty(B, 3, W, W, device=dev)
        if train and bufs["iuv_train"] is None:
            bufs["iuv_train"] = torch.empty(B, 3, W, W, device=dev)
        return bufs

    def _render(self, vertices, textures, cam_t, orthographic_scale, lights_rgb_settings, verts_features, fragments, train):
        _capi.require_device(vertices, "vertices")
        vertices = _capi.f32c(vertices)
        if vertices.dim() != 3 or vertices.shape[2] != 3:
            raise _capi.HpsError("vertices must be (B,N,3)")
        B, V = vertices.shape[0], vertices.shape[1]
        if self._map_max >= V:
            raise _capi.HpsError("verts_map names vertex %d, the meshes have %d" % (self._map_max, V))
        bufs = self._outputs(B, fragments, train)
        a = _capi.RenderArgs()
        a.struct_bytes = _capi._c.sizeof(_capi.RenderArgs)
        a.B, a.H, a.W, a.num_verts, a.num_dp_verts, a.num_faces = B, self.img_wh, self.img_wh, V, self._Nd, self._F
        a.projection = _capi.RENDER_PERSPECTIVE if self.projection_type == "perspective" else _capi.RENDER_ORTHOGRAPHIC
        P, I = _capi.ptr, _capi.iptr
        keep = [vertices]                                  # what the argument block points to stays alive until the launches are issued

        def per_image(t, width, what):
            t = self._per_image(t, width, what)
            if t.shape[0] not in (1, B):
                raise _capi.HpsError("%s has %d rows, the batch %d" % (what, t.shape[0], B))
            keep.append(t)
            return P(t), (0 if t.shape[0] == 1 else width)

        a.cam_t, a.cam_t_stride = per_image(self._cam_t if cam_t is None else cam_t, 3, "cam_t")
        scale = self._scale
        if orthographic_scale is not None and self.projection_type == "orthographic":
            scale = orthographic_scale
        a.scale, a.scale_stride = per_image(scale, 2, "orthographic_scale")
        a.vertices, a.verts_map, a.faces, a.vf_offsets, a.vf_faces = P(vertices), I(self._map), I(self._faces), I(self._vf_offsets), I(self._vf_faces)
        a.verts_iuv, a.verts_uv = P(self._iuv), P(self._uv)
        if self.render_rgb:
            lights = self._lights
            if lights_rgb_settings is not None:
                lights = [lights_rgb_settings[k] for k in ("location", "ambient_color", "diffuse_color", "specular_color")]
            for k, name in enumerate(("light_location", "ambient", "diffuse", "specular")):
                p, stride = per_image(lights[k], 3, name)
                setattr(a, name, p)
                a.light_stride[k] = stride
            if verts_features is not None:
                _capi.require_device(verts_features, "verts_features")
                verts_features = _capi.f32c(verts_features)
                if tuple(verts_features.shape) != (B, V, 3):
                    raise _capi.HpsError("verts_features must be (B,%d,3)" % V)
                keep.append(verts_features)
                a.verts_features = P(verts_features)
            else:
                if textures is None:
                    raise _capi.HpsError("render_rgb needs textures (B,Ht,Wt,3) or verts_features (B,N,3)")
                _capi.require_device(textures, "textures")
                textures = _capi.f32c(textures)
                if textures.dim() != 4 or textures.shape[0] != B or textures.shape[3] != 3:
                    raise _capi.HpsError("textures must be (B,Ht,Wt,3)")
                keep.append(textures)
                a.texture, a.tex_h, a.tex_w = P(textures), textures.shape[1], textures.shape[2]
            a.rgb = P(bufs["rgb"])
        a.workspace = P(bufs["ws"])
        a.iuv, a.depth = P(bufs["iuv"]), P(bufs["depth"])
        if fragments:
            a.pix_to_face, a.bary = I(bufs["pix_to_face"]), P(bufs["bary"])
        if train:
            a.iuv_train = P(bufs["iuv_train"])
        _capi.call("hps_render", _capi._c.addressof(a), _capi.stream())
        return bufs

    def forward(self, vertices, textures=None, cam_t=None, orthographic_scale=None, lights_rgb_settings=None, verts_features=None,
                return_fragments=False):
        """:223-290 -> {'iuv_images' (B,H,W,3), 'rgb_images' (B,H,W,3) with render_rgb, 'depth_images' (B,H,W)}; with
        ``return_fragments`` also 'pix_to_face' (B,H,W) int32, the face's index in faces_densepose[0] (-1: none), and
        'bary_coords' (B,H,W,3)."""
        bufs = self._render(vertices, textures, cam_t, orthographic_scale, lights_rgb_settings, verts_features, return_fragments, False)
        out = {"iuv_images": bufs["iuv"].permute(0, 2, 3, 1), "depth_images": bufs["depth"]}
        if self.render_rgb:
            out["rgb_images"] = bufs["rgb"].permute(0, 2, 3, 1)
        if return_fragments:
            out["pix_to_face"], out["bary_coords"] = bufs["pix_to_face"], bufs["bary"].permute(0, 2, 3, 1)
        return out

    def render_train_inputs(self, vertices, textures=None, cam_t=None, orthographic_scale=None, lights_rgb_settings=None,
                            verts_features=None):
        """train/train_poseMF_shapeGaussian_net.py:189-196 -> (iuv_in, rgb_in), both (B,3,H,W): the IUV image with U and V times
        255 and all three planes rounded half to even, and the RGB image -- what SyntheticTrainFrontEnd.__call__ takes."""
        if not self.render_rgb:
            raise _capi.HpsError("render_train_inputs needs a renderer built with render_rgb=True")
        bufs = self._render(vertices, textures, cam_t, orthographic_scale, lights_rgb_settings, verts_features, False, True)
        return bufs["iuv_train"], bufs["rgb"]

    def _silhouette(self, vertices, target_silhouettes, cam_t, orthographic_scale, group, flip, want_counts, want_masks):
        """hps_silhouette_iou into the buffers owned per (M, group): (counts or None, masks or None)."""
        _capi.require_device(vertices, "vertices")
        vertices = _capi.f32c(vertices)
        if vertices.dim() != 3 or vertices.shape[2] != 3:
            raise _capi.HpsError("vertices must be (M,N,3)")
        M, V, W, group = vertices.shape[0], vertices.shape[1], self.img_wh, int(group)
        if self._map_max >= V:
            raise _capi.HpsError("verts_map names vertex %d, the meshes have %d" % (self._map_max, V))
        if group < 1 or M % group != 0:
            raise _capi.HpsError("group (%d) must divide the number of meshes (%d)" % (group, M))
        bufs = self._silhouette_bufs.get((M, group))
        if bufs is None:
            nbytes = _capi.query_workspace(_capi.WS_SILHOUETTE, M, self._Nd, _capi.silhouette_d2(self._F, W))
            bufs = dict(ws=torch.empty(nbytes // 4, device=self.device, dtype=torch.float32),
                        counts=torch.empty(M, 4, device=self.device, dtype=torch.int32), masks=None)
            self._silhouette_bufs[(M, group)] = bufs
        if want_masks and bufs["masks"] is None:
            bufs["masks"] = torch.empty(M, W, W, device=self.device, dtype=torch.uint8)
        a = _capi.SilhouetteArgs()
        a.struct_bytes = _capi._c.sizeof(_capi.SilhouetteArgs)
        a.M, a.W, a.group, a.num_verts, a.num_dp_verts, a.num_faces = M, W, group, V, self._Nd, self._F
        a.projection = _capi.RENDER_PERSPECTIVE if self.projection_type == "perspective" else _capi.RENDER_ORTHOGRAPHIC
        a.flip_x_pi = 1 if flip else 0
        P = _capi.ptr
        keep = [vertices]                                  # what the argument block points to stays alive until the launches are issued

        def per_group(t, width, what):
            t = self._per_image(t, width, what)
            if t.shape[0] not in (1, M // group):
                raise _capi.HpsError("%s has %d rows, there are %d groups of meshes" % (what, t.shape[0], M // group))
            keep.append(t)
            return P(t), (0 if t.shape[0] == 1 else width)

        a.cam_t, a.cam_t_stride = per_group(self._cam_t if cam_t is None else cam_t, 3, "cam_t")
        scale = self._scale
        if orthographic_scale is not None and self.projection_type == "orthographic":
            scale = orthographic_scale
        a.scale, a.scale_stride = per_group(scale, 2, "orthographic_scale")
        a.vertices, a.verts_map, a.faces, a.verts_iuv = P(vertices), _capi.iptr(self._map), _capi.iptr(self._faces), P(self._iuv)
        if target_silhouettes is not None:
            _capi.require_device(target_silhouettes, "target_silhouettes")
            t = target_silhouettes
            if t.dtype not in (torch.bool, torch.uint8):
                raise _capi.HpsError("target_silhouettes must be bool or uint8, got %s" % t.dtype)
            if tuple(t.shape) != (M // group, W, W):
                raise _capi.HpsError("target_silhouettes must be (%d,%d,%d)" % (M // group, W, W))
            t = t.contiguous()
            t = t.view(torch.uint8) if t.dtype == torch.bool else t                 # True is stored as the byte 1
            keep.append(t)
            a.target = P(t, torch.uint8, "target_silhouettes")
        a.workspace = P(bufs["ws"])
        if want_counts:
            a.counts = _capi.iptr(bufs["counts"])
        if want_masks:
            a.mask_out = P(bufs["masks"], torch.uint8)
        _capi.call("hps_silhouette_iou", _capi._c.addressof(a), _capi.stream())
        return (bufs["counts"] if want_counts else None), (bufs["masks"] if want_masks else None)

    def silhouette_counts(self, vertices, target_silhouettes=None, cam_t=None, orthographic_scale=None, group=1, flip=False,
                          return_silhouettes=False):
        """The silhouette metrics' pixel counts (evaluate/evaluate_poseMF_shapeGaussian_net.py:143-155, 192-203 with
        metrics/eval_metrics_tracker.py:294-304) in one call of hps_silhouette_iou, whatever ``render_rgb`` the renderer was built
        with: ``vertices`` (M,N,3) in groups of ``group`` consecutive meshes (a frame's samples); group g is seen by row g of
        ``cam_t`` / ``orthographic_scale`` (or their one shared row) and scored against ``target_silhouettes[g]`` ((M/group,W,W) bool
        or uint8, nonzero = foreground; None: every pixel counts as background).  ``flip``: the meshes are rotated by pi about x
        first, as the reference does before it renders.  A pixel is set where round(iuv_images[..., 0]) != 0 in forward()'s image,
        bit for bit.  Returns counts (M,4) int32 = [tp, fp, tn, fn] on the device -- with ``return_silhouettes`` (counts, masks
        (M,W,W) uint8 of 0 / 1).  The buffers are owned per (M, group) and overwritten by the next call."""
        counts, masks = self._silhouette(vertices, target_silhouettes, cam_t, orthographic_scale, group, flip, True,
                                         bool(return_silhouettes))
        return (counts, masks) if return_silhouettes else counts


# ---------------------------------------------------------------------------------------------------------------------------------
# the samplers beside the renderer.  Draws come from torch's CPU generator (``generator`` None: the global one), in the reference's
# order, and are moved to the device -- the rule of train_augmentation.draw_augment_plan.
# ---------------------------------------------------------------------------------------------------------------------------------
def _uniform(generator, low_high, *shape):
    low, high = low_high
    return (high - low) * torch.rand(*shape, generator=generator) + low


def augment_light(batch_size, device, rgb_augment_config, generator=None):
    """lighting_augmentation.py:52-67: a light position uniform in direction (a normalised Gaussian vector) and in distance over
    LIGHT_LOC_RANGE, and white ambient / diffuse / specular intensities uniform over their ranges, each (batch_size, 3)."""
    c = rgb_augment_config
    direction = torch.randn(batch_size, 3, generator=generator)
    direction = direction / torch.norm(direction, dim=-1, keepdim=True)
    location = direction * _uniform(generator, c.LIGHT_LOC_RANGE, batch_size)[:, None]
    colours = [_uniform(generator, r, batch_size)[:, None].expand(-1, 3).contiguous()
               for r in (c.LIGHT_AMBIENT_RANGE, c.LIGHT_DIFFUSE_RANGE, c.LIGHT_SPECULAR_RANGE)]
    return {"location": location.to(device), "ambient_color": colours[0].to(device), "diffuse_color": colours[1].to(device),
            "specular_color": colours[2].to(device)}


def normal_sample_shape(batch_size, mean_shape, std_vector, generator=None):
    """smpl_augmentation.py:16-21: mean_shape + N(0, 1) * std_vector, (batch_size, num_betas) on mean_shape's device."""
    noise = torch.randn(batch_size, mean_shape.shape[0], generator=generator).to(mean_shape.device)
    return mean_shape + noise * std_vector


def augment_cam_t(mean_cam_t, xy_std=0.05, delta_z_range=(-0.5, 0.5), generator=None):
    """cam_augmentation.py: x and y moved by N(0, xy_std), z by a uniform draw over delta_z_range; (B,3) like mean_cam_t."""
    batch_size = mean_cam_t.shape[0]
    delta_xy = torch.randn(batch_size, 2, generator=generator) * xy_std
    delta_z = _uniform(generator, delta_z_range, batch_size)
    return mean_cam_t + torch.cat([delta_xy, delta_z[:, None]], dim=1).to(mean_cam_t.device)
