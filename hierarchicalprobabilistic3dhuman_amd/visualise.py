"""The predict visualisations (predict/predict_poseMF_shapeGaussian_net.py:149-333) from the device renderer: the eight-panel figure,
the body projected back onto the original photograph, and the sheet of the eight most 2D-consistent samples.

``PredictVisualiser`` holds the reference's fixed light and camera (:47-52) and builds every picture from three kernels of
csrc/visualise.hip around ONE hps_render call over all of the picture's views (include/hps.h: hps_vis_views, hps_vis_compose,
hps_vis_uncrop).  The kernels write finished uint8 RGB images, so only bytes cross to the host; ``PngWriter`` copies them into
page-locked buffers without blocking and encodes them with PIL on a small thread pool.  ``DevicePngWriter`` is the opt-in beside it:
the PNG file itself is made on the device (hps_png_encode) and only the compressed bytes cross; ``DeviceJpegWriter`` does the same with
baseline JPEG files (hps_jpeg_encode), byte for byte what PIL would save.

Differences from the reference, all deliberate:
  * the joint numbers and confidences it prints into the proxy-representation panel with cv2.putText (:256-263) are NOT drawn: the
    Hershey font lives in OpenCV, which this package does not depend on.  The red joint discs are;
  * the two T-pose views and the sample sheet take a constant per-vertex colour where the reference uses a constant UV texture (all
    views of a picture share one render call; the routes differ by rounding in the interpolation of a constant only);
  * pictures are written as PNG unless the caller asks for JPEG (the reference reuses the input's file name, which makes a lossy JPEG
    of a ``.jpg`` input and a PNG of a ``.png`` one; here the format is the caller's choice and the name is <stem>.png / <stem>.jpg);
  * the warp onto the photograph restates cv2.warpAffine's fixed-point arithmetic and has not been run against OpenCV itself.
There is no matplotlib behind this module: ``jet_lut`` builds the colour map's table from jet's published segments.
"""
import concurrent.futures
import ctypes
import os

import numpy as np
import torch

from . import _capi

_JET_SEGMENTS = {          # matplotlib's _jet_data: (x, y0, y1) per channel, piecewise linear
    "red": ((0.00, 0, 0), (0.35, 0, 0), (0.66, 1, 1), (0.89, 1, 1), (1.00, 0.5, 0.5)),
    "green": ((0.000, 0, 0), (0.125, 0, 0), (0.375, 1, 1), (0.640, 1, 1), (0.910, 0, 0), (1.000, 0, 0)),
    "blue": ((0.00, 0.5, 0.5), (0.11, 1, 1), (0.34, 1, 1), (0.65, 0, 0), (1.00, 0, 0)),
}
PLAIN_COLOUR = 0.7         # :46: the plain texture
NUM_VIS_SAMPLES = 8        # :168


def jet_lut(N=256):
    """matplotlib.cm.jet's look-up table, (N,3) float32: LinearSegmentedColormap's table (gamma 1) evaluated with the same float64
    operations -- the table matplotlib.cm.jet(np.arange(256))[:, :3] returns, rounded to float32."""
    cols = []
    for name in ("red", "green", "blue"):
        data = np.array(_JET_SEGMENTS[name], dtype=np.float64)
        x, y0, y1 = data[:, 0] * (N - 1), data[:, 1], data[:, 2]
        xind = (N - 1) * np.linspace(0, 1, N) ** 1.0
        ind = np.searchsorted(x, xind)[1:-1]
        distance = (xind[1:-1] - x[ind - 1]) / (x[ind] - x[ind - 1])
        lut = np.concatenate([[y1[0]], distance * (y0[ind] - y1[ind - 1]) + y1[ind - 1], [y0[-1]]])
        cols.append(np.clip(lut, 0.0, 1.0))
    return np.stack(cols, axis=1).astype(np.float32)


class PredictVisualiser:
    """:39-52, :149-333 over ``renderer``, a textured_renderer.TexturedIUVRenderer built with projection_type='orthographic',
    render_rgb=True and img_wh=visualise_wh (the DensePose asset is not shipped, so the caller brings the renderer).

    Every picture is one hps_vis_views, one hps_render over all of its views and one hps_vis_compose (``uncropped`` is one
    hps_vis_uncrop on the posed render the preceding ``figure`` left in the renderer's buffers); nothing goes to the host in between.
    The returned uint8 images are owned buffers, overwritten by the next call of the same method."""

    def __init__(self, renderer, pose_shape_cfg, visualise_wh):
        if getattr(renderer, "projection_type", None) != "orthographic":
            raise _capi.HpsError("PredictVisualiser needs an orthographic renderer (projection_type='orthographic')")
        if not getattr(renderer, "render_rgb", False):
            raise _capi.HpsError("PredictVisualiser needs a renderer built with render_rgb=True")
        if int(renderer.img_wh) != int(visualise_wh):
            raise _capi.HpsError("the renderer draws %d x %d images, visualise_wh is %d" % (renderer.img_wh, renderer.img_wh, visualise_wh))
        self.renderer, self.wh = renderer, int(visualise_wh)
        self.D = int(pose_shape_cfg.DATA.PROXY_REP_SIZE)
        dev = self.device = renderer.device
        f32 = lambda a: torch.tensor(a, dtype=torch.float32, device=dev)
        self.lights = {"location": f32([[0.0, -0.8, -2.0]]), "ambient_color": f32([[0.5] * 3]), "diffuse_color": f32([[0.3] * 3]),
                       "specular_color": f32([[0.0] * 3])}                                                    # :47-50
        self.fixed_cam_t, self.fixed_scale, self.cam_z = (0.0, -0.2, 2.5), 0.95, 2.5                          # :51-52, :153
        self.lut = torch.from_numpy(jet_lut()).to(dev)
        self._view_bufs = {}
        self._out = {}
        self._figure_render = None

    # -- the three kernels ---------------------------------------------------------------------------------------------------
    def _views(self, views, cam):
        """views: list of (vertices (V,3), var (V,) or None, yaw, camera) -> (vertices, colours (n,V,3), cam_t (n,3), scale (n,2))."""
        n, V = len(views), int(views[0][0].shape[0])
        bufs = self._view_bufs.get((n, V))
        if bufs is None:
            e = lambda *s: torch.empty(*s, dtype=torch.float32, device=self.device)
            bufs = self._view_bufs[(n, V)] = (e(n, V, 3), e(n, V, 3), e(n, 3), e(n, 2))
        table = (_capi.VisView * n)()
        keep = []
        for i, (verts, var, yaw, camera) in enumerate(views):
            verts = _capi.f32c(verts)
            if tuple(verts.shape) != (V, 3):
                raise _capi.HpsError("every view's mesh must be (%d,3)" % V)
            keep.append(verts)
            table[i].vertices = _capi.ptr(verts, what="vertices")
            if var is not None:
                var = _capi.f32c(var)
                if tuple(var.shape) != (V,):
                    raise _capi.HpsError("the per-vertex variance must be (%d,)" % V)
                keep.append(var)
                table[i].var = _capi.ptr(var, what="variance")
            table[i].yaw, table[i].camera = int(yaw), int(camera)
        cam = _capi.f32c(cam).reshape(-1)
        if cam.numel() != 3:
            raise _capi.HpsError("cam must hold [s, tx, ty]")
        a = _capi.VisViewsArgs()
        a.struct_bytes = ctypes.sizeof(_capi.VisViewsArgs)
        a.num_views, a.num_verts, a.constant = n, V, PLAIN_COLOUR
        a.fixed_cam_t[0], a.fixed_cam_t[1], a.fixed_cam_t[2] = self.fixed_cam_t
        a.fixed_scale, a.cam_z = self.fixed_scale, self.cam_z
        a.views, a.lut, a.cam = table, _capi.ptr(self.lut), _capi.ptr(cam, what="cam")
        a.out_vertices, a.out_colours, a.out_cam_t, a.out_scale = (_capi.ptr(b) for b in bufs)
        _capi.call("hps_vis_views", ctypes.addressof(a), _capi.stream())
        return bufs

    def _render(self, views, cam):
        verts, colours, cam_t, scale = self._views(views, cam)
        return self.renderer._render(verts, None, cam_t, scale, self.lights, colours, False, False)

    def _output(self, key, shape):
        out = self._out.get(key)
        if out is None or tuple(out.shape) != tuple(shape):
            out = self._out[key] = torch.empty(shape, dtype=torch.uint8, device=self.device)
        return out

    def _compose(self, key, rows, cols, panels, bufs, cropped_rgb, proxy_rep, joints2D):
        wh, D = self.wh, self.D
        keep = []

        def plane_stack(t, what, channels=None):
            if t is None:
                return None
            _capi.require_device(t, what)
            t = _capi.f32c(t)
            t = t[0] if t.dim() == 4 else t
            if t.dim() != 3 or t.shape[1] != D or t.shape[2] != D or (channels is not None and t.shape[0] != channels):
                raise _capi.HpsError("%s must be (%s,%d,%d)" % (what, channels if channels is not None else "C", D, D))
            keep.append(t)
            return t

        crop, proxy = plane_stack(cropped_rgb, "cropped_rgb", 3), plane_stack(proxy_rep, "proxy_rep")
        joints = None
        if joints2D is not None:
            _capi.require_device(joints2D, "joints2D")
            joints = _capi.f32c(joints2D).reshape(-1, 2)
            keep.append(joints)
        table = (_capi.VisPanel * len(panels))()
        for i, (kind, row, col, render) in enumerate(panels):
            table[i].kind, table[i].row, table[i].col, table[i].render = kind, row, col, render
        out = self._output(key, (rows * wh, cols * wh, 3))
        a = _capi.VisComposeArgs()
        a.struct_bytes = ctypes.sizeof(_capi.VisComposeArgs)
        a.rows, a.cols, a.wh, a.num_panels, a.num_renders = rows, cols, wh, len(panels), bufs["rgb"].shape[0]
        a.D, a.proxy_channels, a.num_joints = D, (proxy.shape[0] if proxy is not None else 0), (joints.shape[0] if joints is not None else 0)
        a.panels, a.rgb, a.iuv = table, _capi.ptr(bufs["rgb"]), _capi.ptr(bufs["iuv"])
        a.crop, a.proxy, a.joints = _capi.ptr(crop), _capi.ptr(proxy), _capi.ptr(joints)
        a.out = _capi.ptr(out, torch.uint8)
        _capi.call("hps_vis_compose", ctypes.addressof(a), _capi.stream())
        return out

    # -- the three pictures --------------------------------------------------------------------------------------------------
    FIGURE_VIEWS = ((0, 0, 1), (0, 1, 0), (0, 2, 0), (0, 3, 0), (1, 0, 0), (1, 1, 0))      # (0 posed / 1 T-pose, yaw step, camera)
    FIGURE_PANELS = ((_capi.VIS_PANEL_CROP, 0, 0, 0), (_capi.VIS_PANEL_PROXY, 1, 0, 0),       # :241-274: crop | posed | rot180 | T-pose
                     (_capi.VIS_PANEL_RENDER_OVER_CROP, 0, 1, 0), (_capi.VIS_PANEL_RENDER, 1, 1, 1),    # proxy | rot90 | rot270 | T-pose rot90
                     (_capi.VIS_PANEL_RENDER, 0, 2, 2), (_capi.VIS_PANEL_RENDER, 1, 2, 3),
                     (_capi.VIS_PANEL_RENDER, 0, 3, 4), (_capi.VIS_PANEL_RENDER, 1, 3, 5))

    @torch.no_grad()
    def figure(self, result, cropped_rgb, proxy_rep, joints2D):
        """:187-276 -> (2 wh, 4 wh, 3) uint8 on the device.  ``result``: one image's entries of infer()'s dict (verts_mode, verts_tpose
        (V,3), unc (V,), cam (3,)); ``cropped_rgb`` (3,D,D) or (1,3,D,D), None: the crop panels are black; ``proxy_rep`` (C,D,D) or
        (1,C,D,D); ``joints2D`` (K,2) in crop pixels or None: no discs."""
        views = [((result["verts_mode"], result["unc"]) if which == 0 else (result["verts_tpose"], None)) + (yaw, camera)
                 for which, yaw, camera in self.FIGURE_VIEWS]
        bufs = self._render(views, result["cam"])
        self._figure_render = bufs
        return self._compose("figure", 2, 4, self.FIGURE_PANELS, bufs, cropped_rgb, proxy_rep, joints2D)

    @torch.no_grad()
    def uncropped(self, image, bbox_centre, bbox_wh):
        """:278-300 -> (H, W, 3) uint8 on the device: the posed render of the preceding ``figure`` call over the photograph.  ``image``
        (3,H,W) float in [0,1] (what the front end holds), ``bbox_centre`` (2,) = (vertical, horizontal) and ``bbox_wh`` = max(h, w)
        BBOX_SCALE_FACTOR, device tensors."""
        bufs = self._figure_render
        if bufs is None:
            raise _capi.HpsError("uncropped() uses the posed render of a preceding figure() call")
        for t, what in ((image, "image"), (bbox_centre, "bbox_centre"), (bbox_wh, "bbox_wh")):
            _capi.require_device(t, what)
        image = _capi.f32c(image)
        if image.dim() != 3 or image.shape[0] != 3:
            raise _capi.HpsError("image must be (3,H,W)")
        centre, side = _capi.f32c(bbox_centre).reshape(-1), _capi.f32c(bbox_wh).reshape(-1)
        if centre.numel() != 2 or side.numel() != 1:
            raise _capi.HpsError("bbox_centre must hold 2 values, bbox_wh 1")
        H, W = int(image.shape[1]), int(image.shape[2])
        out = self._output("uncrop", (H, W, 3))
        a = _capi.VisUncropArgs()
        a.struct_bytes = ctypes.sizeof(_capi.VisUncropArgs)
        a.H, a.W, a.wh = H, W, self.wh
        a.rgb, a.iplane = _capi.ptr(bufs["rgb"][0]), _capi.ptr(bufs["iuv"][0, 0])
        a.image, a.bbox_centre, a.bbox_wh, a.out = _capi.ptr(image), _capi.ptr(centre), _capi.ptr(side), _capi.ptr(out, torch.uint8)
        _capi.call("hps_vis_uncrop", ctypes.addressof(a), _capi.stream())
        return out

    @torch.no_grad()
    def samples_figure(self, result, cropped_rgb, proxy_rep):
        """:167-185, :302-333 -> (3 wh, 6 wh, 3) uint8 on the device: the mode and the eight samples whose projected joints agree best
        with the input heat-maps (joints2D_error_sorted_verts_sampling), each from the front over the crop and from the side; cell
        2 i is sample i's front view, cell 2 i + 1 its side view, cells counted along the rows.  ``result`` also holds
        verts_samples (N,V,3) and joints_samples (N,J,3); with fewer than eight samples the remaining cells stay black."""
        from .sampling_utils import joints2D_error_sorted_verts_sampling
        proxy = proxy_rep if proxy_rep.dim() == 4 else proxy_rep[None]
        best = joints2D_error_sorted_verts_sampling(result["verts_samples"], result["joints_samples"], proxy[:, 1:],
                                                    result["cam"].reshape(1, 3), top=NUM_VIS_SAMPLES)
        meshes = [result["verts_mode"]] + list(best.unbind(0))
        views, panels = [], []
        for i, mesh in enumerate(meshes):
            views += [(mesh, None, 0, 1), (mesh, None, 1, 0)]
            panels += [(_capi.VIS_PANEL_RENDER_OVER_CROP, (2 * i) // 6, (2 * i) % 6, 2 * i),
                       (_capi.VIS_PANEL_RENDER, (2 * i + 1) // 6, (2 * i + 1) % 6, 2 * i + 1)]
        bufs = self._render(views, result["cam"])
        return self._compose("samples", 3, 6, panels, bufs, cropped_rgb, None, None)


def predict_visualiser(renderer, pose_shape_cfg, visualise_wh):
    """The PredictVisualiser of ``renderer``, kept with it between predict calls (its device buffers are allocated once)."""
    vis = renderer.__dict__.get("_predict_visualiser")
    if vis is None or vis.wh != int(visualise_wh) or vis.D != int(pose_shape_cfg.DATA.PROXY_REP_SIZE):
        vis = renderer.__dict__["_predict_visualiser"] = PredictVisualiser(renderer, pose_shape_cfg, visualise_wh)
    return vis


class PngWriter:
    """Device uint8 images -> PNG files without stalling the caller: ``write`` copies the bytes into a page-locked buffer with a
    non-blocking copy on the current stream and hands buffer and event to a pool of at most ``workers`` (<= 4, never sized from the
    CPU count) threads, which wait for the copy and encode with PIL.  ``drain`` waits for every file and re-raises the first error.
    At most 2 x workers pictures are in flight; page-locked buffers are reused by size."""

    def __init__(self, workers=4):
        self.workers = max(1, min(4, int(workers)))
        self._pool = concurrent.futures.ThreadPoolExecutor(max_workers=self.workers)
        self._free = {}
        self._pending = []

    def _buffer(self, nbytes):
        free = self._free.setdefault(nbytes, [])
        return free.pop() if free else torch.empty(nbytes, dtype=torch.uint8).pin_memory()

    def write(self, image, path):
        from PIL import Image      # noqa: F401  (fail here, on the caller's thread, if PIL is missing)
        while len(self._pending) >= 2 * self.workers:
            self._pending.pop(0).result()
        shape, nbytes = tuple(image.shape), image.numel()
        host = self._buffer(nbytes)
        host.copy_(image.reshape(-1), non_blocking=True)
        copied = torch.cuda.Event()
        copied.record()
        self._pending.append(self._pool.submit(self._encode, host, copied, shape, path))

    def _encode(self, host, copied, shape, path):
        from PIL import Image
        try:
            copied.synchronize()
            tmp = path + ".part"
            Image.fromarray(host.numpy().reshape(shape)).save(tmp, format="PNG", compress_level=1)
            os.replace(tmp, path)
        finally:
            self._free.setdefault(host.numel(), []).append(host)

    def drain(self):
        pending, self._pending = self._pending, []
        error = None
        for f in pending:
            try:
                f.result()
            except Exception as e:      # every file is waited for before the first error goes up
                error = error or e
        if error is not None:
            raise error

    def close(self):
        self.drain()
        self._pool.shutdown(wait=True)




class _FileSlot:
    """What one picture of a device writer holds while it is in flight: the file's device buffer (``bound`` bytes), the library's
    workspace, the device length, and page-locked mirrors of file and length.  Reused by picture shape."""

    def __init__(self, key, device, bound, workspace_bytes):
        self.key, self.bound = key, bound
        self.out = torch.empty(self.bound, dtype=torch.uint8, device=device)
        self.workspace = torch.empty(max(16, workspace_bytes), dtype=torch.uint8, device=device)
        self.length = torch.zeros(1, dtype=torch.int64, device=device)
        self.host = torch.empty(self.bound, dtype=torch.uint8).pin_memory()
        self.host_length = torch.zeros(1, dtype=torch.int64).pin_memory()


def png_bound(H, W, C):
    """include/hps.h: hps_png_bound -- a capacity no file of an (H, W, C) picture exceeds."""
    n = _capi.load(dev=_capi._use_dev).hps_png_bound(int(H), int(W), int(C))
    if n < 0:
        raise _capi.HpsError("hps_png_bound(%d, %d, %d): %s" % (H, W, C, _capi.load(dev=_capi._use_dev).hps_last_error().decode()))
    return int(n)


def png_segment_rows(H, W, C):
    """include/hps.h: hps_png_segment_rows -- the rows of one independently compressed segment."""
    n = _capi.load(dev=_capi._use_dev).hps_png_segment_rows(int(H), int(W), int(C))
    if n < 0:
        raise _capi.HpsError("hps_png_segment_rows(%d, %d, %d): %s" % (H, W, C, _capi.load(dev=_capi._use_dev).hps_last_error().decode()))
    return int(n)


class _DeviceFileWriter:
    """What the device writers share: PngWriter's interface with the encoder on the device.  ``write`` / ``write_many`` launch the
    library's kernels on the current stream into reused device buffers and never block the caller; a worker thread waits for the
    file's length, copies exactly that many bytes through a reused page-locked buffer on a copy stream of its own, writes
    ``path + ".part"`` and renames it.  No host thread compresses anything.  At most 2 x workers pictures are in flight; ``drain``
    waits for every file and re-raises the first error.  Pictures are (H, W), (H, W, 1) or (H, W, 3) uint8 device tensors.
    A subclass names the library call (ENTRY, ARGS, MAX_IMAGES) and gives a picture's bound, workspace and arguments."""

    ENTRY = ARGS = MAX_IMAGES = None

    def __init__(self, workers=4):
        self.workers = max(1, min(4, int(workers)))
        self._pool = concurrent.futures.ThreadPoolExecutor(max_workers=self.workers)
        self._free = {}
        self._pending = []
        self._copy_streams = {}

    def _bound(self, H, W, C):
        raise NotImplementedError

    def _workspace_bytes(self, H, W, C):
        raise NotImplementedError

    def _describe(self, im):
        """The entry's own fields of one picture's arguments (strategy; quality and sampling)."""
        raise NotImplementedError

    def _slot(self, key, device):
        free = self._free.setdefault((key, device), [])
        return free.pop() if free else _FileSlot(key, device, self._bound(*key), self._workspace_bytes(*key))

    def write(self, image, path):
        self.write_many([image], [path])

    def write_many(self, images, paths):
        if len(images) != len(paths) or not 1 <= len(images) <= self.MAX_IMAGES:
            raise _capi.HpsError("write_many takes 1 .. %d pictures and as many paths" % self.MAX_IMAGES)
        while len(self._pending) + len(images) > 2 * self.workers and self._pending:
            self._pending.pop(0).result()
        a = self.ARGS()
        a.struct_bytes, a.num_images = ctypes.sizeof(self.ARGS), len(images)
        slots, keep = [], []
        try:
            for i, image in enumerate(images):
                _capi.require_device(image, "image")
                if image.dtype != torch.uint8 or image.dim() not in (2, 3) or (image.dim() == 3 and image.shape[2] not in (1, 3)):
                    raise _capi.HpsError("a picture is (H, W), (H, W, 1) or (H, W, 3) uint8")
                image = image.contiguous()
                if image.data_ptr() % 16:
                    image = image.clone()
                keep.append(image)
                key = (int(image.shape[0]), int(image.shape[1]), int(image.shape[2]) if image.dim() == 3 else 1)
                slot = self._slot(key, image.device)
                slots.append(slot)
                im = a.image[i]
                im.pixels, (im.H, im.W, im.C) = _capi.ptr(image, torch.uint8, "image"), key
                self._describe(im)
                im.out, im.capacity = _capi.ptr(slot.out, torch.uint8), slot.bound
                im.length, im.workspace = _capi.ptr(slot.length, torch.int64), _capi.ptr(slot.workspace, torch.uint8)
            _capi.call(self.ENTRY, ctypes.addressof(a), _capi.stream())
        except Exception:
            for slot in slots:
                self._free[(slot.key, slot.out.device)].append(slot)
            raise
        for slot in slots:
            slot.host_length.copy_(slot.length, non_blocking=True)
        encoded = torch.cuda.Event()
        encoded.record()
        for slot, path in zip(slots, paths):
            self._pending.append(self._pool.submit(self._deliver, slot, encoded, path))

    def _deliver(self, slot, encoded, path):
        try:
            encoded.synchronize()
            n = int(slot.host_length[0])
            if not 0 < n <= slot.bound:
                raise _capi.HpsError("%s reported a file of %d bytes, the bound is %d" % (self.ENTRY, n, slot.bound))
            device = slot.out.device
            with torch.cuda.device(device):
                stream = self._copy_streams.get(device)
                if stream is None:
                    stream = self._copy_streams.setdefault(device, torch.cuda.Stream(device=device))
                with torch.cuda.stream(stream):
                    slot.host[:n].copy_(slot.out[:n], non_blocking=True)
                    copied = torch.cuda.Event()
                    copied.record()
                copied.synchronize()
            tmp = path + ".part"
            with open(tmp, "wb") as f:
                f.write(memoryview(slot.host.numpy())[:n])
            os.replace(tmp, path)
        finally:
            self._free[(slot.key, slot.out.device)].append(slot)

    def drain(self):
        pending, self._pending = self._pending, []
        error = None
        for f in pending:
            try:
                f.result()
            except Exception as e:      # every file is waited for before the first error goes up
                error = error or e
        if error is not None:
            raise error

    def close(self):
        self.drain()
        self._pool.shutdown(wait=True)


class DevicePngWriter(_DeviceFileWriter):
    """PngWriter's interface with the encoder on the device (include/hps.h: hps_png_encode; _DeviceFileWriter holds the route): two
    kernels per call, only the compressed bytes cross.  ``write_many`` puts up to _capi.PNG_MAX_IMAGES pictures -- one predicted
    image's three -- into one library call.  ``strategy``: "fixed" (the default: deflate's fixed Huffman code, filters Sub and Up) or
    "dynamic" (one dynamic Huffman code per segment, all five filters: smaller files for more device time) -- hps_png_image.strategy
    0 and 1."""

    STRATEGIES = {"fixed": 0, "dynamic": 1}
    ENTRY, ARGS, MAX_IMAGES = "hps_png_encode", _capi.PngEncodeArgs, _capi.PNG_MAX_IMAGES

    def __init__(self, workers=4, strategy="fixed"):
        if strategy not in self.STRATEGIES:
            raise ValueError("strategy is 'fixed' or 'dynamic', not %r" % (strategy,))
        self.strategy = strategy
        super().__init__(workers)

    def _bound(self, H, W, C):
        return png_bound(H, W, C)

    def _workspace_bytes(self, H, W, C):
        return _capi.query_workspace(_capi.WS_PNG, H, W, C)

    def _describe(self, im):
        im.strategy = self.STRATEGIES[self.strategy]


class DeviceJpegWriter(_DeviceFileWriter):
    """PngWriter's interface writing baseline JPEG files made on the device (include/hps.h: hps_jpeg_encode; _DeviceFileWriter holds
    the route): four kernels per call, only the compressed bytes cross.  The files equal PIL's ``save(format="JPEG", quality=quality,
    subsampling=...)`` byte for byte.  ``subsampling``: "444", "422" or "420" (ignored for greyscale pictures); quality 95 and "420"
    are what cv2.imwrite leaves libjpeg at, but nothing here has been run against OpenCV itself."""

    SUBSAMPLINGS = {"444": 0, "422": 1, "420": 2}
    ENTRY, ARGS, MAX_IMAGES = "hps_jpeg_encode", _capi.JpegEncodeArgs, _capi.JPEG_ENC_MAX_IMAGES

    def __init__(self, workers=4, quality=95, subsampling="420"):
        if subsampling not in self.SUBSAMPLINGS:
            raise ValueError("subsampling is '444', '422' or '420', not %r" % (subsampling,))
        if not 1 <= int(quality) <= 100:
            raise ValueError("quality is 1 .. 100, not %r" % (quality,))
        self.quality, self.subsampling = int(quality), subsampling
        super().__init__(workers)

    def _bound(self, H, W, C):
        from .jpeg import encode_bound
        return encode_bound(H, W, C, self.SUBSAMPLINGS[self.subsampling])

    def _workspace_bytes(self, H, W, C):
        return _capi.query_workspace(_capi.WS_JPEG_ENC, H, W, _capi.jpeg_enc_d2(C, self.SUBSAMPLINGS[self.subsampling]))

    def _describe(self, im):
        im.quality, im.sampling = self.quality, self.SUBSAMPLINGS[self.subsampling]
