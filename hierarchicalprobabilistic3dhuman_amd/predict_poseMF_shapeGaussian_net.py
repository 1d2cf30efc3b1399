"""Per-image inference harness: the batched core of the reference's
predict/predict_poseMF_shapeGaussian_net.py:103-165 (``infer``) and a ``predict_poseMF_shapeGaussian_net``
with the reference's signature (:19-32) that feeds it.

Everything between the proxy representation and the sampled meshes runs on the device through
libhps.so.  The front end before it (:61-100) runs on the device for a whole group of images when the key-point detector is the
device HRNet (predict_frontend.DevicePredictFrontEnd: box, crops and key points are the kernels of csrc/predict_frontend.hip, one
HRNet forward per group); with any other injected ``hrnet_model`` it is assembled per image from
``hrnet_model`` / ``object_detect_model`` (the person detector itself is out of scope), the torch crop
glue of image_utils / predict_hrnet and the Canny / heat-map kernels of SURVEY 8(f)1; ``proxy_rep_fn`` may replace it.  Results go to ``result_fn`` or to .pt files;
with ``vis_renderer=`` the reference's three pictures per image (:149-333: the eight-panel figure, the body over the original
photograph, the sample sheet) are written beside them as PNG files -- or, with ``picture_format="jpeg"``, as baseline JPEG files made on the device (row (f)25) --
by visualise.PredictVisualiser (section 9 for what stays out: the text labels of the proxy panel, the
reference's reuse of the input's own file name).
"""
import os
import weakref

import torch

from . import _capi
from .rigid_transform_utils import rot6d_to_rotmat, batch_rodrigues
from .sampling_utils import pose_matrix_fisher_sampling_torch, vertex_uncertainty, check_sampling
from .label_conversions import make_proxy_representation
from .resnet import FilledStemFrames


FUSE_JOINTS_AND_UNCERTAINTY = True     # False: hps_smpl_joints and hps_vertex_uncertainty as two launches (the cross-check of the tests; same bits)


@torch.no_grad()
def infer(pose_shape_model, smpl_model, proxy_rep_input, num_samples=50, use_mean_shape=True,
          sample_on_cpu=False, seed=None, image_offset=0, input_feats=None, _before_meshes=None, _after_smpl=None,
          _run_net=None, _after_unc=None, _seed_dev=None):
    """predict/predict_poseMF_shapeGaussian_net.py:103-165 for a batch of B proxy representations.

    proxy_rep_input: (B,18,256,256) on the device.  Returns a dict of device tensors; every entry equals
    what looping the reference's batch-1 code over the images yields:
      pose_F/U/V (B,23,3,3), pose_S (B,23,3), pose_rotmats_mode (B,23,3,3), shape_loc/shape_scale (B,10),
      glob (B,6), cam (B,3), glob_rotmats (B,3,3), verts_mode (B,6890,3), joints_mode (B,90,3),
      verts_tpose (B,6890,3), R_samples (B,N,23,3,3), verts_samples (B,N,6890,3),
      joints_samples (B,N,90,3), unc (B,6890).
    """
    run_net = _run_net if _run_net is not None else pose_shape_model
    pose_F, pose_U, pose_S, pose_V, mode, shape_dist, glob, cam = run_net(proxy_rep_input, input_feats=input_feats)
    B, nj = pose_F.shape[:2]
    N = num_samples
    dev = pose_F.device
    if glob.shape[-1] == 3:                                                       # :107-110
        glob_rotmats = batch_rodrigues(glob)
    else:
        glob_rotmats = rot6d_to_rotmat(glob)
    # One flattened SMPL call over M = B (N + 2) meshes: [mode | T-pose | samples].  The reference makes three calls per image
    # (:112-115, :136, sampling_utils.py:182-185); SMPL is per-mesh so the results are the same, and the zero axis-angle pose
    # of :136 is exactly the identity rotation under smplx's Rodrigues.  The sampler writes its rotations straight into the
    # sample rows of the pose buffer and one kernel (hps_infer_assemble) fills everything else: no torch cat / expand glue.
    M = B * (N + 2)
    f32 = dict(device=dev, dtype=torch.float32)
    body = torch.empty(M, nj, 3, 3, **f32)
    R = pose_matrix_fisher_sampling_torch(pose_U, pose_S, pose_V, N, b=1.5, oversampling_ratio=8, sample_on_cpu=sample_on_cpu,
                                          seed=seed, image_offset=image_offset, out=body[2 * B:].view(B, N, nj, 3, 3),
                                          seed_dev=_seed_dev)
    loc = _capi.f32c(shape_dist.loc)
    nb = loc.shape[1]
    betas_s = None
    if not use_mean_shape:                                                        # sampling_utils.py:178-181
        if sample_on_cpu:
            host = torch.distributions.Normal(loc.cpu(), shape_dist.scale.cpu(), validate_args=False)
            betas_s = host.sample([N]).transpose(0, 1).contiguous().to(dev)
        else:
            betas_s = shape_dist.sample([N]).transpose(0, 1).contiguous()
    glob_all = torch.empty(M, 1, 3, 3, **f32)
    betas_all = torch.empty(M, nb, **f32)
    P = _capi.ptr
    _capi.call("hps_infer_assemble", P(_capi.f32c(mode)), P(_capi.f32c(glob_rotmats)), P(loc), P(betas_s) if betas_s is not None else None,
               P(body), P(glob_all), P(betas_all), B, N, nj, nb, _capi.stream())
    # InferencePipeline: the chip-filling mesh kernel waits at _before_meshes and signals at _after_smpl; sampling, the input
    # assembly, pose prep (before) and the joint regression / uncertainty (after) are small or HBM-bound and may run beside the
    # neighbouring batches' encoders
    # (the uncertainties are allocated HERE, on the caller's stream: a hook may move the launches between _before_meshes and
    # _after_unc to another stream, and every result must come from the caller's pool -- see SMPL.forward, "ordered")
    unc = torch.empty(B, smpl_model.num_verts, **f32)
    shared = None
    if use_mean_shape and hasattr(smpl_model, "layout_tables"):
        # every mesh of image b has the betas loc[b]: the shape blend is formed once per image (hps_smpl_mesh_fused_shared_shape)
        rows = lambda: list(range(B)) + list(range(B)) + [b for b in range(B) for _ in range(N)]          # [mode | T-pose | samples]
        shared = (loc,) + smpl_model.layout_tables((B, N), rows)
    # the joint regression of the call's meshes and the uncertainty pass read what the mesh kernel has just written and do not depend
    # on each other: one launch (hps_joints_and_uncertainty) when the sample count takes the register-resident pass
    deferred = {}
    out = smpl_model(body_pose=body, global_orient=glob_all, betas=betas_all, pose2rot=False,
                     _before_mesh=_before_meshes, _after_mesh=_after_smpl, _shared_shapes=shared,
                     _defer_joints=deferred.update if (FUSE_JOINTS_AND_UNCERTAINTY and 8 <= N <= 128) else None)
    V = out.vertices.shape[1]
    verts_s = out.vertices[2 * B:].view(B, N, V, 3)
    joints_s = out.joints[2 * B:].view(B, N, -1, 3)
    if deferred:
        d = deferred
        _capi.call("hps_joints_and_uncertainty", P(d["picked"]), P(d["j_posed"]), _capi.iptr(d["csr_ptr"]), _capi.iptr(d["csr_slot"]),
                   P(d["csr_val"]), d["n_rows"], d["J"], P(d["transl"]) if d["transl"] is not None else None, P(d["joints"]), d["M"],
                   d["n_picked"], P(verts_s), P(unc), B, N, V, _capi.stream())
    else:
        vertex_uncertainty(verts_s, out=unc)                                      # sampling_utils.py:189-190
    if _after_unc is not None:
        _after_unc()
    return dict(pose_F=pose_F, pose_U=pose_U, pose_S=pose_S, pose_V=pose_V, pose_rotmats_mode=mode,
                shape_loc=loc, shape_scale=shape_dist.scale, glob=glob, cam=cam,
                glob_rotmats=glob_rotmats, verts_mode=out.vertices[:B], joints_mode=out.joints[:B],
                verts_tpose=out.vertices[B:2 * B], R_samples=R, verts_samples=verts_s, joints_samples=joints_s,
                unc=unc)


def proxy_representation(rgb, joints2D, joints2D_visib, edge_detect_model, pose_shape_cfg, out=None, encoder=None):
    """predict/predict_poseMF_shapeGaussian_net.py:88-100: RGB crop (B,3,D,D), 2D joints (B,17,2) in crop pixels and
    their visibility (B,17) -> the (B,18,D,D) network input.  ``edge_detect_model`` is a CannyEdgeDetector: its edge map goes
    straight into channel 0 (hps_canny_edge_map: the five other outputs of the detector's dict are not materialised), the
    heat-map kernel fills channels 1..17.  Any other callable with the reference's interface works through its output dict.

    ``encoder``: the ResNet that will consume the result ON THE CURRENT STREAM (InferencePipeline.submit(make_input=...) calls this
    function on the encoder's stream).  When its Winograd stem takes this shape, the proxy representation is written straight into
    the stem's phase frames (hps_proxy_rep_phase_frames: the same values hps_proxy_rep + hps_stem_phase_split would leave there,
    without the (B,18,D,D) tensor) and the returned FilledStemFrames is what ``encoder(...)`` accepts in its place."""
    D = pose_shape_cfg.DATA.PROXY_REP_SIZE
    if encoder is not None and hasattr(edge_detect_model, "edge_map_into"):
        B, K = joints2D.shape[:2]
        filled = encoder.stem_frames(B, K + 1, D, D, rgb.device) if K == 17 else None
        if filled is not None:
            edge = torch.empty(B, 1, D, D, device=rgb.device, dtype=torch.float32)
            edge_detect_model.edge_map_into(rgb, edge, nms=bool(pose_shape_cfg.DATA.EDGE_NMS))
            j = _capi.f32c(joints2D)
            vis = None if joints2D_visib is None else _capi.f32c(joints2D_visib.to(rgb.device).float()).reshape(B, K)
            std = float(pose_shape_cfg.DATA.HEATMAP_GAUSSIAN_STD)
            # the edge map is computed now (it may run beside the previous batch's mesh kernel); the frames themselves are written
            # by encoder.forward(filled) right in front of the stem convolution, on the stream that call runs on
            filled.fill = lambda: _capi.call("hps_proxy_rep_phase_frames", _capi.ptr(edge), _capi.ptr(j), _capi.ptr(vis) if vis is not None else None,
                                             _capi.ptr(filled.frames), B, K, D, D, std, _capi.stream())
            return filled
    if hasattr(edge_detect_model, "edge_map_into"):
        B, K = joints2D.shape[:2]
        if out is None:
            out = torch.empty(B, K + 1, D, D, device=rgb.device, dtype=torch.float32)
        edge_detect_model.edge_map_into(rgb, out, nms=bool(pose_shape_cfg.DATA.EDGE_NMS))       # the CONFIG picks the entry (:93)
        return make_proxy_representation(None, joints2D, joints2D_visib, D, pose_shape_cfg.DATA.HEATMAP_GAUSSIAN_STD, out=out)
    edges = edge_detect_model(rgb)
    edge = edges["thresholded_thin_edges"] if pose_shape_cfg.DATA.EDGE_NMS else edges["thresholded_grad_magnitude"]
    return make_proxy_representation(edge, joints2D, joints2D_visib, D, pose_shape_cfg.DATA.HEATMAP_GAUSSIAN_STD)


class InferencePipeline:
    """Software pipeline over successive batches on three HIP streams.

    The head of batch i is a dependency chain of eleven small launches (eight kinematic levels, each an MLP + a serial 3x3 SVD:
    0.5 ms of latency on a handful of CUs); the encoder of batch i+1 does not depend on it.  ``submit`` enqueues the encoder on a
    side stream, ``finish`` runs the head on a high-priority stream as soon as its encoder's event fires, then sampling -> SMPL ->
    uncertainty on the caller's stream:

        pipe = InferencePipeline(net, smpl, num_samples=100)
        t = pipe.submit(x0)
        for x_next in batches[1:]:
            t_next = pipe.submit(x_next)
            result = pipe.finish(t, after=t_next)     # same dict as infer()
            t = t_next
        result = pipe.finish(t)

    ``after=`` makes the mesh kernel (blend GEMM + LBS) of this batch start only when the next batch's encoder has drained, and the
    encoder after that waits for it: the two fill the chip on their own and would only time-share it.  Everything else -- the head,
    sampling, pose prep, the joint regression and the HBM-bound uncertainty pass -- is small or memory-bound and runs beside the
    neighbouring encoders (what that overlap costs, and why the head's workgroups are kept small).
    Results are identical to ``infer`` (same kernels, same order per batch)."""

    def __init__(self, pose_shape_model, smpl_model, num_samples=50, use_mean_shape=True, sample_on_cpu=False):
        self.net, self.smpl = pose_shape_model, smpl_model
        self.num_samples, self.use_mean_shape, self.sample_on_cpu = num_samples, use_mean_shape, sample_on_cpu
        # The head is a chain of small dependent kernels on a stream of its own: it depends on its batch's encoder only, not on what is
        # queued on the caller's stream.  (Rounds 3-5 made this a HIGH-priority stream so that its workgroups would take the next free
        # slots beside kernels that fill every CU.  With the side kernels in stream order behind the mesh kernel it no longer changes
        # the rate at any batch size -- 22.48-22.56 k against 22.53-22.58 k images/s at B = 64, equal at B = 8 / 16 and N = 50 / 100 /
        # 1000, profiles/r06_ab.txt -- and a high-priority queue in the process has a side effect on every OTHER queue: a stream-side
        # wait that polls beside a chain of small kernels doubled that chain's time, tests/dev/graph_time.py.  Normal priority.)
        self.head_stream = torch.cuda.Stream()
        self.enc_stream = None        # created by the first submit (its kind depends on the batch size)
        self._seen = (None, None)     # the encoder's and the head's device states at the last submit
        self.mesh_stream = None
        self._smpl_done = None
        self._enc_tail = None         # the event recorded last on the encoder's stream, while nothing has been queued behind it
        self._exclusive = True
        self.enc_events = None
        self.trace = None             # bench.py --trace-steps: list of per-batch dicts of timing events (head / mesh phases)
        self.early_relayout = False   # A/B (bench.py --early-relayout): round 3 +0.9 % images/s with the mesh kernel 12 % slower; round 4's kernels: 21.2 -> 19.6 k
        # exclusive_mesh: the mesh kernel and the neighbouring encoders take turns (right when each fills the chip on its own:
        # B = 64: 17.9 k images/s either way, the encoder stretched from 2.9 to 3.5 ms when they share).  False: no ordering
        # between them -- a small batch's encoder cannot fill the chip (its persistent Winograd workgroups are few: 64-256 items
        # per layer at B = 16) and the mesh kernel's workgroups take the idle CUs: B = 16, N = 1000 4 680 -> 4 925 images/s
        # (profiles/r03_ablations.txt).  None = decide from the batch size (overlap below 32 images).
        self.exclusive_mesh = None
        # encoder_cus > 0: when not exclusive, encoder and mesh phases run on DISJOINT CU subsets (encoder_cus of the 32 CUs of
        # every XCD for the encoder, hps_stream_create_cu_partition).  Which side wins depends on which chain is longer.  Measured
        # at B = 16, N = 1000 (16 032 meshes: mesh kernel 1.5 ms against an encoder of 0.97 ms alone) with the round-3 encoder:
        # shared CUs 5 570-5 580 images/s, 8 CUs per XCD 5 750-5 790, 10 -> 5 200-5 240, 4 or 6 -> 3 200-3 270 (the persistent
        # Winograd workgroups of 16 images need 64 CUs); with the slower round-2 encoder sharing won (4 925 against 4 860).  At
        # B = 16, N = 100 the mesh kernel is a tenth of that and a partition would only slow the encoder down.  None = decide from
        # the work: 8 CUs per XCD when the batch is small enough to overlap at all AND carries at least 12 000 meshes, else 0 -- 12 when
        # the SMPL object's mesh_arith is "bf16x3" at that moment (the faster mesh kernel shifts the balance: B = 16, N = 1000,
        # images/s by encoder CUs 0 / 8 / 12 / 16 / 20: fp32 5 770 / 6 090 / 5 480 / 4 730 / 3 770, bf16x3 6 880 / 5 980 / 6 950 / 6 270 / 5 280).
        self.encoder_cus = None
        # head_cus > 0 (exclusive schedule only; an experiment, default off): the head's chain of small dependent kernels runs on
        # head_cus CUs of every XCD that the mesh kernel's stream does not use (the caller's stream becomes the partition of the other
        # 32 - head_cus; the encoder keeps the whole chip).  The idea: the head of batch i + 1 is ready when the mesh kernel of batch i
        # starts, but beside that kernel's four workgroups per CU it only gets a slot when one retires, so most of its 11 launches slip
        # into the next encoder's stem and Winograd layers.  Measured (profiles/r05_experiments.txt item 7): with 1-4 CUs per XCD the
        # encoder's time in the loop does not change and the mesh kernel loses its CUs in proportion -- 20.6-20.8 k against 21.0-21.1 k
        # images/s.  None = 0.
        self.head_cus = None
        # inline_mesh (exclusive schedule): the chip-filling mesh kernel of batch i is enqueued ON THE ENCODER'S STREAM, behind encoder
        # i + 1 and in front of encoder i + 2, instead of on the caller's stream with an event on either side.  The two take turns
        # anyway; as neighbours in one queue they need no hand-over between hardware queues on the critical path (+0.7-1 % images/s,
        # interleaved A/B, identical results).  Pose prep (before) and joints / uncertainty (after) stay on the caller's stream and
        # meet the mesh kernel through two events; the kernel's operands are NOT registered with the encoder's stream -- the caller's
        # stream waits for the kernel instead (SMPL.forward, "ordered"): record_stream would have the allocator put one event record
        # per freed operand into the encoder's queue.
        self.inline_mesh = True
        # inline_side (with inline_mesh): the joint regression and the uncertainty pass of batch i FOLLOW its mesh kernel on the encoder's
        # stream, in front of encoder i + 2, instead of racing that encoder's first kernel from the caller's stream.  Left on the
        # caller's stream the two become ready at the moment the mesh kernel ends -- exactly when the next encoder's first kernel is
        # dispatched; a persistent first kernel (the NCHW-fed stem: every CU's LDS and registers for 0.6 ms) then decided the step by
        # whether it or the side kernels won that race (round 5: -3 to -7 % when it won).  In stream order there is no race: the
        # HBM-bound pass runs alone (0.09 ms against 0.14 ms beside an encoder; it reads vertices the mesh kernel has just written),
        # and a step is the sum of its kernels' work either way.
        self.inline_side = True
        # (measured and dropped: making the next encoder wait for the uncertainty pass as well -- B = 16, N = 1000: 3.15 -> 3.24 ms
        # per step; B = 64, N = 100: 3.53 -> 3.51)

    def caller_stream(self, batch):
        """The stream a caller should make current around its submit / finish loop for batches of ``batch`` images: the mesh
        partition's stream when the pipeline runs encoder and mesh kernels side by side on CU subsets, otherwise the stream
        that is current now.  (finish() also works from any other stream -- it then hops to the partition's stream and back,
        which makes every result tensor cross streams: correct, but the caching allocator cannot recycle such blocks promptly.)"""
        if self.enc_stream is None:
            self._setup_streams(batch)
        return self.mesh_stream if self.mesh_stream is not None else torch.cuda.current_stream()

    def _setup_streams(self, batch):
        self._exclusive = self.exclusive_mesh if self.exclusive_mesh is not None else batch >= 32
        k = self.encoder_cus
        if k is None:
            k = 0
            if not self._exclusive and batch * (self.num_samples + 2) >= 12000:
                k = 12 if getattr(self.smpl, "mesh_arith", "f32") == "bf16x3" else 8
        self.enc_stream = None
        if not self._exclusive and k:
            # CUs per XCD from the device (MI355X: 256 / 8 = 32); a device or partition mode the mask scheme does not fit (a CU
            # count that is not a multiple of 8, fewer CUs per XCD than asked for, a runtime without CU masks) falls back to
            # shared CUs instead of failing the first submit
            k = int(k)
            per_xcd = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count // 8
            try:
                if not 0 < k < per_xcd:
                    raise _capi.HpsError("encoder_cus = %d does not fit %d CUs per XCD" % (k, per_xcd))
                enc = _capi.cu_partition_stream(0, k)
                self.mesh_stream = _capi.cu_partition_stream(k, per_xcd - k)
                self.enc_stream, self._mesh_cus = enc, per_xcd - k
            except _capi.HpsError as e:
                import warnings
                warnings.warn("InferencePipeline: no CU partition on this device (%s); encoder and mesh kernels share the CUs" % e)
                self.mesh_stream = None
        h = self.head_cus
        if h is None:
            h = 0
        if self._exclusive and h:
            per_xcd = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count // 8
            try:
                if not 0 < int(h) < per_xcd:
                    raise _capi.HpsError("head_cus = %d does not fit %d CUs per XCD" % (h, per_xcd))
                self.mesh_stream = _capi.cu_partition_stream(0, per_xcd - int(h))
                self.head_stream = _capi.cu_partition_stream(per_xcd - int(h), int(h))
                self._mesh_cus = per_xcd - int(h)
            except _capi.HpsError as e:
                import warnings
                warnings.warn("InferencePipeline: no CU partition on this device (%s); the head shares the CUs" % e)
                self.mesh_stream = None
        if self.enc_stream is None:
            self.enc_stream = torch.cuda.Stream()

    @torch.no_grad()
    def submit(self, proxy_rep_input=None, input_ready=None, make_input=None):
        """Enqueue the encoder of one batch on the side stream.

        ``make_input``: instead of a finished tensor, a callable that BUILDS the proxy representation -- it is called on the
        encoder's stream (after ``input_ready``, in front of the wait for the previous batch's mesh kernel, so the HBM-bound
        front-end kernels -- proxy_representation(): Canny edge map + heat-maps -- may run beside that MFMA-bound kernel) and
        returns the (B,18,D,D) tensor.  This is the reference's order (predict/...:88-104: front end, then the net) without a
        stream hop in between.

        ``input_ready`` says when ``proxy_rep_input`` is complete:
          * an event -- the encoder waits for exactly that event (the precise form: record it right behind the kernels / the
            non-blocking copy that produce the input, on whatever stream they run);
          * ``None`` (default) -- safe for any producer on the caller's stream: an event recorded on the caller's stream NOW,
            i.e. the encoder waits for everything queued there so far -- including a previous batch's uncertainty pass, which it
            would otherwise run beside (measured: 3.15 -> 3.24 ms per step at B = 64);
          * ``False`` -- no ordering: the caller guarantees the input is already complete (resident data, or its own
            synchronisation)."""
        if make_input is None:
            _capi.require_device(proxy_rep_input, "proxy_rep_input")
        main = torch.cuda.current_stream()
        if self.enc_stream is None:
            if proxy_rep_input is None:
                raise _capi.HpsError("InferencePipeline: call caller_stream(batch) before the first submit(make_input=...)")
            self._setup_streams(proxy_rep_input.shape[0])
        # ONE-TIME ordering of the side streams behind whatever the caller has queued so far: parameters still being
        # written by a device-to-device load_state_dict, BN folding of a preceding warm-up infer(), ... -- whatever `input_ready` says
        # about the INPUT, the encoder's lazy prepare() and first convolutions (and the head) must not read weights that are still in
        # flight.  Again whenever the encoder's or the head's device state has been replaced (load_state_dict / invalidate() / .to() /
        # a switch): the next forward re-prepares on the side streams.  Costs nothing in steady state.
        seen, self._seen = self._seen, (self.net.image_encoder.device_state(), self.net.device_state())
        if seen[0] is not self._seen[0] or seen[1] is not self._seen[1]:
            self.enc_stream.wait_stream(main)
            self.head_stream.wait_stream(main)
            if self.mesh_stream is not None and self.mesh_stream != main:
                self.mesh_stream.wait_stream(main)
        if input_ready is None:
            ready = torch.cuda.Event()
            ready.record(main)
            self.enc_stream.wait_event(ready)
        elif input_ready is not False:
            self.enc_stream.wait_event(input_ready)
        if make_input is not None:
            with torch.cuda.stream(self.enc_stream):
                proxy_rep_input = make_input()
            if not isinstance(proxy_rep_input, FilledStemFrames):
                _capi.require_device(proxy_rep_input, "proxy_rep_input")
        gate = None
        if self._smpl_done is None or not self._exclusive:
            pass
        elif self.early_relayout:
            # the input relayout (HBM-bound) is enqueued at once and may run beside the previous batch's fused mesh kernel
            # (MFMA-bound); the convolutions wait for that batch's SMPL kernels
            prev_done = self._smpl_done
            gate = lambda: self.enc_stream.wait_event(prev_done)
        else:
            self.enc_stream.wait_event(self._smpl_done)
        with torch.cuda.stream(self.enc_stream):
            ev = None
            tail, self._enc_tail = self._enc_tail, None
            if self.enc_events is not None:      # bench.py: HIP events around the encoder, on its own stream
                # (an event record is a marker packet of ~8 us in the queue: the mark behind the previous batch's last kernel on this
                # stream, when it was recorded with timing and nothing has been queued since, is this encoder's start mark, and the
                # end mark is the event the head waits for)
                start = tail if (tail is not None and make_input is None and input_ready is False and gate is None) else None
                ev = (start if start is not None else torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                if start is None:
                    ev[0].record(self.enc_stream)
            feats = self.net.image_encoder(proxy_rep_input, _gate=gate)
            if ev is not None:
                ev[1].record(self.enc_stream)
                self.enc_events.append(ev)
                done = ev[1]
            else:
                done = torch.cuda.Event()
                done.record(self.enc_stream)
        proxy_rep_input.record_stream(self.enc_stream)
        return feats, done

    @torch.no_grad()
    def finish(self, ticket, seed=None, image_offset=0, after=None):
        if self.mesh_stream is None or torch.cuda.current_stream() == self.mesh_stream:
            return self._finish(ticket, seed, image_offset, after)
        # partitioned: everything after the encoder runs on the mesh partition's stream, ordered after what the caller has
        # queued; the caller's stream then waits for the results
        caller = torch.cuda.current_stream()
        self.mesh_stream.wait_stream(caller)
        with torch.cuda.stream(self.mesh_stream):
            res = self._finish(ticket, seed, image_offset, after)
        caller.wait_stream(self.mesh_stream)
        for v in res.values():
            if torch.is_tensor(v):
                v.record_stream(caller)
        return res

    def _finish(self, ticket, seed, image_offset, after):
        feats, done = ticket
        main = torch.cuda.current_stream()
        main.wait_event(done)
        feats.record_stream(main)
        inline = self._exclusive and self.inline_mesh and self.mesh_stream is None and self.enc_stream is not None

        def hook():
            if inline:
                # everything the mesh kernel reads was produced on `main` (sampling, assembly, pose prep): one event, normally long
                # signalled when encoder i + 1 drains; from here to smpl_done() the current stream is the encoder's
                ready = torch.cuda.Event()
                ready.record(main)
                self.enc_stream.wait_event(ready)
                torch.cuda.set_stream(self.enc_stream)
                if tr is not None:
                    tr["mesh0"].record(self.enc_stream)
                return "ordered"                         # smpl_done() makes `main` wait for the mesh kernel (see SMPL.forward)
            elif after is not None and self._exclusive:
                main.wait_event(after[1])
            if tr is not None:
                tr["mesh0"].record(torch.cuda.current_stream())
        hs = self.head_stream

        tr = None
        if self.trace is not None:
            tr = {k: torch.cuda.Event(enable_timing=True) for k in ("head0", "head1", "mesh0", "mesh1")}
            self.trace.append(tr)

        def run_net(_, input_feats=None):
            # head on the high-priority stream: depends on the encoder only, not on what is still queued on `main`
            hs.wait_event(done)
            input_feats.record_stream(hs)
            with torch.cuda.stream(hs):
                if tr is not None:
                    tr["head0"].record(hs)
                outs = self.net(None, input_feats=input_feats)
                if tr is not None:
                    tr["head1"].record(hs)
            main.wait_stream(hs)
            for t in outs:
                for u in ((t.loc, t.scale) if isinstance(t, torch.distributions.Normal) else (t,)):
                    u.record_stream(main)
            return outs

        side = inline and self.inline_side

        def smpl_done(mesh_end=None):
            if side:                                     # joints + uncertainty follow in stream order; side_done() hands back
                if tr is not None:
                    tr["mesh1"].record(self.enc_stream)
                return
            if inline:
                done_ev = mesh_end                       # SMPL.forward's own event behind the kernel, when it recorded one
                if done_ev is None:
                    done_ev = torch.cuda.Event()
                    done_ev.record(self.enc_stream)
                if tr is not None:
                    tr["mesh1"].record(self.enc_stream)
                torch.cuda.set_stream(main)
                main.wait_event(done_ev)                 # joints / uncertainty read the vertices
                self._smpl_done = None                   # the next encoder follows the mesh kernel in stream order
                return
            self._smpl_done = torch.cuda.Event()
            self._smpl_done.record(main)
            if tr is not None:
                tr["mesh1"].record(main)

        def side_done():
            if not side:
                return
            # one event behind the uncertainty pass: the caller's stream waits for it (every result of the batch is complete), and
            # with the bench's timing on it doubles as the next encoder's start mark (nothing is queued between the two)
            timing = self.enc_events is not None
            done_ev = torch.cuda.Event(enable_timing=timing)
            done_ev.record(self.enc_stream)
            self._enc_tail = done_ev if timing else None
            torch.cuda.set_stream(main)
            main.wait_event(done_ev)
            self._smpl_done = None                       # the next encoder follows in stream order

        try:
            return infer(self.net, self.smpl, None, num_samples=self.num_samples, use_mean_shape=self.use_mean_shape,
                         sample_on_cpu=self.sample_on_cpu, seed=seed, image_offset=image_offset, input_feats=feats,
                         _before_meshes=hook, _after_smpl=smpl_done, _run_net=run_net, _after_unc=side_done)
        finally:
            # an error between the hooks (a failed launch in SMPL.forward) must not leave the caller on the encoder's stream -- nor
            # let it reuse operands a kernel already queued there still reads: on the error path the caller's stream waits for the
            # encoder's (no cost in steady state)
            if torch.cuda.current_stream() != main:
                torch.cuda.set_stream(main)
                main.wait_stream(self.enc_stream)


class GraphedInfer:
    """``infer`` for ONE fixed (batch, num_samples) captured in hipGraphs: a call costs the host one graph launch instead of the ~50
    kernel launches of the eager path (batch 1: 0.34 ms of host time for 0.53 ms of device time -- at the reference's own operating
    point, one image per call (predict/predict_poseMF_shapeGaussian_net.py:58-59), the host was what bounded a loop of calls).

        g = GraphedInfer(net, smpl, batch=1, num_samples=50)
        out = g(x, seed=7)                  # same dict as infer(net, smpl, x, num_samples=50, seed=7): same kernels, same order, same bits

    ``slots`` graphs with their own static buffers and streams alternate: call k + 1 may be issued (and, the chip being mostly idle at
    batch 1, may run) while call k is still in flight.  The returned tensors are the slot's STATIC output buffers: they are valid
    until the same slot is used again, ``slots`` calls later -- consume or clone them before that (the predict loop hands them to
    ``result_fn`` / saves them at once).  The Philox key is read from device memory at run time (hps_mf_sample seed_dev), so replays
    draw new samples; ``seed`` / ``image_offset`` mean what they mean for infer().  Philox sampling only (the reference's
    seed-reproducible host-noise route draws on the host per call and cannot be captured)."""

    def __init__(self, pose_shape_model, smpl_model, batch, num_samples=50, use_mean_shape=True, slots=2, input_shape=(18, 256, 256)):
        if not use_mean_shape:
            # (sampled shapes draw from torch's device generator inside infer(): a captured draw would need the generator's graph-safe
            # offset bookkeeping, which nothing here has exercised -- the predict path, the one this class serves, uses the mean shape)
            raise ValueError("GraphedInfer captures the use_mean_shape=True form of infer() only")
        self.net, self.smpl = pose_shape_model, smpl_model
        self.batch, self.num_samples, self.use_mean_shape = int(batch), int(num_samples), True
        self.input_shape = tuple(input_shape)
        self._slots = [None] * max(1, int(slots))
        self._k = 0

    def _state(self):
        """What a captured launch sequence depends on beyond its own buffers; held by the slot, it keeps that memory alive."""
        return (self.net.image_encoder.device_state(), self.net.device_state(), self.smpl.device_state(), FUSE_JOINTS_AND_UNCERTAINTY)

    def _capture(self, dev):
        stream = torch.cuda.Stream()
        x = torch.zeros((self.batch,) + self.input_shape, device=dev, dtype=torch.float32)
        key_dev = torch.zeros(2, dtype=torch.int64, device=dev)
        key_host = torch.zeros(2, dtype=torch.int64).pin_memory()
        run = lambda: infer(self.net, self.smpl, x, num_samples=self.num_samples, use_mean_shape=self.use_mean_shape, _seed_dev=key_dev)
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            for _ in range(2):                   # eager warm-up on the capture stream: weight preparation, frame buffers, LDS grants
                run()
        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            out = run()
        from . import sampling_utils
        accepted = sampling_utils.last_accepted[0]
        return dict(stream=stream, x=x, key_dev=key_dev, key_host=key_host, graph=graph, out=out, accepted=accepted,
                    copied=None, done=None, state=self._state())

    @torch.no_grad()
    def __call__(self, proxy_rep_input, seed=None, image_offset=0, wait=True):
        """``proxy_rep_input``: (batch, 18, D, D) device or page-locked host tensor, or a list of ``batch`` (1, 18, D, D) items (copied
        row by row into the slot's static input: no concatenation).  ``wait=False``: the caller's stream is NOT made to wait for the
        replay -- returns (out, done_event) and the caller waits for the event before it reads ``out`` (the predict loop issues call
        k + 1 first, so that two replays overlap)."""
        from .sampling_utils import _philox_seed, philox_key
        items = proxy_rep_input if isinstance(proxy_rep_input, (list, tuple)) else None
        shape = ((len(items),) + tuple(items[0].shape[1:])) if items is not None else tuple(proxy_rep_input.shape)
        if shape != (self.batch,) + self.input_shape:
            raise _capi.HpsError("GraphedInfer was captured for inputs of shape %s, got %s" % ((self.batch,) + self.input_shape, shape))
        i = self._k % len(self._slots)
        self._k += 1
        s = self._slots[i]
        if s is not None and any(a is not b for a, b in zip(s["state"], self._state())):
            torch.cuda.synchronize()             # every graph is stale: none may still run when its memory goes back to the allocator
            self._slots = [None] * len(self._slots)
            s = None
        if s is None:
            s = self._slots[i] = self._capture(torch.device("cuda", torch.cuda.current_device()))
        if s["copied"] is not None:
            s["copied"].synchronize()            # the key copy that last used the page-locked pair (``slots`` calls ago) has run
        s["key_host"][0] = philox_key(_philox_seed(seed), signed=True)
        s["key_host"][1] = int(image_offset) * self.net.num_joints
        caller = torch.cuda.current_stream()
        st = s["stream"]
        st.wait_stream(caller)                   # the input's producer (and whoever still reads the slot's previous outputs)
        with torch.cuda.stream(st):
            for dst, src in (zip(s["x"].split(1), items) if items is not None else [(s["x"], proxy_rep_input)]):
                dst.copy_(src, non_blocking=True)
                if src.is_cuda:
                    src.record_stream(st)        # the caller may drop its input before the copy has run
            s["key_dev"].copy_(s["key_host"], non_blocking=True)
            s["copied"] = torch.cuda.Event()
            s["copied"].record(st)
            s["graph"].replay()
            done = torch.cuda.Event()
            done.record(st)
        if not wait:
            return s["out"], done
        # the HOST waits (the call's contract is "one image, results ready on return").  Making the caller's STREAM wait for the event
        # instead -- a barrier packet that polls for the whole replay -- was measured to slow the replay's own kernels down by up to 2x
        # once a high-priority queue exists in the process (tests/dev/graph_time.py --pipeline --bisect: 1.08 -> 1.94 ms)
        done.synchronize()
        return s["out"]

    def check_sampling(self):
        """Raise if a (image, joint) call of any slot's LAST replay never reached N accepted proposals (synchronises)."""
        bad = 0
        for s in self._slots:
            if s is not None:
                s["stream"].synchronize()
                bad += int((s["accepted"] < self.num_samples).sum().item())
        if bad:
            raise _capi.HpsError("matrix-Fisher sampling failed for %d (image, joint) calls (are pose_S / pose_U / pose_V finite?)" % bad)


_PREDICT_PIPELINES = weakref.WeakKeyDictionary()      # model -> (key, InferencePipeline, StagedUpload) of predict_poseMF_shapeGaussian_net


class StagedUpload:
    """Host -> device staging for a loop of batches: page-locked host tensors are copied with non_blocking=True on a copy
    stream of their own into ``slots`` alternating sets of device buffers (allocated once), so the copy of batch k+1 runs under
    the kernels of batch k.  ``upload(host_tensors)`` returns (device_tensors, ready_event); hand the event to
    InferencePipeline.submit(input_ready=...) and give the batch's encoder event back through ``release`` -- a slot is
    overwritten only after the consumer recorded on it has run.  Pageable host tensors work too (the runtime then stages them
    itself, synchronously)."""

    def __init__(self, slots=2, copy_streams=2):
        self.stream = torch.cuda.Stream()
        # upload_rows deals its per-item copies over several streams (several DMA queues: the set-up gap of one copy, ~20 us per
        # 4.7 MB item, runs under another's transfer)
        self.more_streams = [torch.cuda.Stream() for _ in range(max(0, copy_streams - 1))]
        self._bufs = [None] * slots
        self._consumed = [None] * slots
        self._k = 0

    def upload(self, host_tensors):
        slot = self._k % len(self._bufs)
        self._k += 1
        if self._bufs[slot] is None or any(b.shape != h.shape or b.dtype != h.dtype for b, h in zip(self._bufs[slot], host_tensors)):
            with torch.cuda.stream(self.stream):
                self._bufs[slot] = [torch.empty(h.shape, dtype=h.dtype, device="cuda") for h in host_tensors]
        if self._consumed[slot] is not None:
            self.stream.wait_event(self._consumed[slot])
        with torch.cuda.stream(self.stream):
            for b, h in zip(self._bufs[slot], host_tensors):
                b.copy_(h, non_blocking=True)
            ready = torch.cuda.Event()
            ready.record(self.stream)
        self._last = slot
        return list(self._bufs[slot]), ready

    def upload_rows(self, host_items):
        """Like upload() for ONE batched tensor given as its items: ``host_items`` = list of (1, ...) host tensors (what a
        per-image loader returns); item i is copied straight into row i of the slot's (len, ...) device buffer -- no host-side
        concatenation (a 4.7 MB proxy representation per image is a memcpy worth avoiding).  Returns (batch, ready_event)."""
        slot = self._k % len(self._bufs)
        self._k += 1
        shape = (len(host_items),) + tuple(host_items[0].shape[1:])
        buf = self._bufs[slot]
        if buf is None or buf[0].shape != shape:
            with torch.cuda.stream(self.stream):
                buf = self._bufs[slot] = [torch.empty(shape, dtype=torch.float32, device="cuda")]
        streams = [self.stream] + self.more_streams
        if self._consumed[slot] is not None:
            for st in streams:
                st.wait_event(self._consumed[slot])
        for st in self.more_streams:
            st.wait_stream(self.stream)                  # the buffer's allocation (first use) is ordered on the first stream
        for j, st in enumerate(streams):
            with torch.cuda.stream(st):
                for i in range(j, len(host_items), len(streams)):
                    buf[0][i:i + 1].copy_(host_items[i], non_blocking=True)
        for st in self.more_streams:
            self.stream.wait_stream(st)
        ready = torch.cuda.Event()
        ready.record(self.stream)
        self._last = slot
        return buf[0], ready

    def release(self, consumed_event, slot=None):
        """``consumed_event``: recorded after the last kernel that reads the most recent upload's device buffers."""
        self._consumed[self._last if slot is None else slot] = consumed_event


def predict_poseMF_shapeGaussian_net(pose_shape_model, pose_shape_cfg, smpl_model, hrnet_model, hrnet_cfg,
                                     edge_detect_model, device, image_dir, save_dir, object_detect_model=None,
                                     joints2Dvisib_threshold=0.75, visualise_wh=512, visualise_uncropped=True,
                                     visualise_samples=False, proxy_rep_fn=None, num_samples=50, batch_size=1,
                                     result_fn=None, vis_renderer=None, batched_front_end=None, png_encoder="pil",
                                     image_decoder="pil", picture_format="png", picture_quality=95):
    """Signature of predict/predict_poseMF_shapeGaussian_net.py:19-32 plus keyword extensions.

    Called exactly like the reference (run_predict.py:77-89) it runs the reference's front end (:61-100) on the injected
    ``hrnet_model`` / ``object_detect_model`` (any callables with the reference's interfaces; the device implementation of the
    former is pose2D_hrnet.PoseHighResolutionNet) and ``edge_detect_model``
    (canny_edge_detector.CannyEdgeDetector), image files read by cv2 or PIL.  proxy_rep_fn(image_path) -> (1,18,D,D) tensor
    optionally replaces that whole front end.  result_fn(image_name, result_dict) receives the
    outputs instead of the reference's pytorch3d renderer; by default vertices / joints / uncertainties are
    saved as <save_dir>/<image>.pt.

    ``vis_renderer``: a textured_renderer.TexturedIUVRenderer built with projection_type='orthographic', render_rgb=True and
    img_wh=visualise_wh (the DensePose asset is not shipped, so the caller brings the renderer, as the evaluation's
    ``silhouette_renderer=``).  With it the reference's pictures (:149-333) are written for every image, beside the .pt / result_fn
    delivery, which does not change: <save_dir>/<stem>.png (the eight-panel figure), <stem>_uncrop.png if ``visualise_uncropped``
    and <stem>_samples.png if ``visualise_samples``.  PNG by default; ``picture_format="jpeg"`` writes <stem>.jpg, <stem>_uncrop.jpg
    and <stem>_samples.jpg instead (below).  The reference reuses the input's file name, which makes a lossy JPEG of a .jpg input and
    a PNG of a .png one; here the format is the caller's choice whatever the input was.  Without ``vis_renderer``, ``visualise_wh`` /
    ``visualise_uncropped`` / ``visualise_samples`` / ``picture_format`` have no effect.
    A custom ``proxy_rep_fn`` may return a dict with ``proxy_rep`` and, for the pictures, ``cropped_rgb`` (1,3,D,D), ``joints2D``
    (1,K,2) in crop pixels, ``image`` (3,H,W) float in [0,1], ``bbox_centre`` (2,) and ``bbox_wh`` (max(h, w) BBOX_SCALE_FACTOR),
    all on the device; a bare tensor gives black crop panels, no joint discs and no uncropped picture (one warning).
    ``png_encoder``: "pil" (the default) encodes the pictures with PIL on visualise.PngWriter's host threads; "device" makes the PNG
    files on the device (visualise.DevicePngWriter, hps_png_encode: an image's pictures in one library call, only the compressed bytes
    cross to the host); "device-dynamic" is the same route with DevicePngWriter(strategy="dynamic"): a dynamic Huffman code per segment
    and all five filters, for smaller files.  The decoded pixels are the same; the files are not (another compressor).  Anything else is
    a ValueError.
    ``picture_format``: "png" (the default) as above; "jpeg" makes baseline JPEG files on the device (visualise.DeviceJpegWriter,
    hps_jpeg_encode: an image's three pictures in one library call) at ``picture_quality`` (1 .. 100, default 95) and 4:2:0 -- libjpeg's
    settings as cv2.imwrite leaves them, so the files are what the reference writes for a .jpg input as far as the encoder goes; they
    equal PIL's ``save(quality=picture_quality)`` of the same pixels byte for byte, and have not been run against OpenCV itself.
    ``png_encoder`` must be left at its default with it (a ValueError naming both otherwise); any other ``picture_format`` is a
    ValueError.

    ``batched_front_end``: None runs the front end of a whole group of ``batch_size`` images on the device with ONE HRNet forward
    (predict_frontend.DevicePredictFrontEnd: box, crops and key points are libhps kernels, no host synchronisation of its own) when it
    can -- no ``proxy_rep_fn``, a GPU device, ``hrnet_model`` a pose2D_hrnet.PoseHighResolutionNet and an ``edge_detect_model`` with
    ``edge_map_into`` -- and the per-image route of predict_hrnet / image_utils otherwise; True demands it (HpsError when it cannot be
    used), False forbids it.

    ``image_decoder``: "pil" (the default) reads every photograph on the host (``load_rgb_image``); "device" hands the batched front
    end the files themselves: the JPEG files of a group that are in the device profile (include/hps.h: baseline, 4:4:4 / 4:2:2 / 4:2:0
    or greyscale) go up as file bytes and are decoded in one call (jpeg.DeviceJpegDecoder) to the bytes PIL gives, straight into the
    uint8 tensors the front end and the uncropped picture read; every other file takes the host route as before.  It needs the batched
    front end (HpsError where the per-image route is taken); anything else is a ValueError.
    """
    if image_decoder not in ("pil", "device"):
        raise ValueError("image_decoder is 'pil' or 'device', not %r" % (image_decoder,))
    if png_encoder not in ("pil", "device", "device-dynamic"):
        raise ValueError("png_encoder is 'pil', 'device' or 'device-dynamic', not %r" % (png_encoder,))
    if picture_format not in ("png", "jpeg"):
        raise ValueError("picture_format is 'png' or 'jpeg', not %r" % (picture_format,))
    if picture_format == "jpeg" and png_encoder != "pil":
        raise ValueError("picture_format='jpeg' writes no PNG files: leave png_encoder at its default, not %r" % (png_encoder,))
    if picture_format == "jpeg" and not 1 <= int(picture_quality) <= 100:
        raise ValueError("picture_quality is 1 .. 100, not %r" % (picture_quality,))
    on_device = png_encoder != "pil" or picture_format == "jpeg"
    suffix = ".jpg" if picture_format == "jpeg" else ".png"
    device = torch.device(device)
    batched = None
    if use_batched_front_end(batched_front_end, proxy_rep_fn, device, hrnet_model, edge_detect_model):
        from .predict_frontend import DevicePredictFrontEnd
        if device.type == "cuda":
            torch.cuda.set_device(device)
        batched = DevicePredictFrontEnd(pose_shape_cfg, hrnet_model, hrnet_cfg, edge_detect_model, object_detect_model,
                                        joints2Dvisib_threshold, device)
    if device.type == "cuda":
        torch.cuda.set_device(device)              # libhps launches on the current device's current stream
    jpeg_decoder = None
    if image_decoder == "device":
        if batched is None:
            raise _capi.HpsError("image_decoder='device' decodes a group's photographs for the batched front end, but the per-image "
                                 "route is taken here (%s); use image_decoder='pil'"
                                 % ("a proxy_rep_fn replaces the whole front end" if proxy_rep_fn is not None else
                                    "batched_front_end=False" if batched_front_end is False else
                                    "it needs a GPU, a pose2D_hrnet.PoseHighResolutionNet and an edge detector with edge_map_into"))
        from .jpeg import DeviceJpegDecoder, encode_file
        jpeg_decoder = DeviceJpegDecoder()
    pose_shape_model.eval()
    image_fnames = sorted(f for f in os.listdir(image_dir) if f.lower().endswith((".png", ".jpg", ".jpeg", ".npy")))
    if proxy_rep_fn is None and batched is None:
        proxy_rep_fn = _reference_front_end(pose_shape_cfg, hrnet_model, hrnet_cfg, edge_detect_model,
                                            object_detect_model, joints2Dvisib_threshold, device)
    os.makedirs(save_dir, exist_ok=True)
    vis = writer = None
    extras = {}                                          # image name -> what the front end kept for the pictures
    if vis_renderer is not None:
        from .visualise import DeviceJpegWriter, DevicePngWriter, PngWriter, predict_visualiser
        vis = predict_visualiser(vis_renderer, pose_shape_cfg, visualise_wh)
        if picture_format == "jpeg":
            writer = DeviceJpegWriter(quality=int(picture_quality), subsampling="420")
        else:
            writer = DevicePngWriter(strategy="dynamic" if png_encoder == "device-dynamic" else "fixed") if on_device else PngWriter()
    warned = []

    def get_proxy(name):
        """proxy_rep_fn's tensor for one image; a dict's other entries are kept for the pictures until the image is delivered."""
        fn = getattr(proxy_rep_fn, "with_extras", proxy_rep_fn) if vis is not None else proxy_rep_fn
        out = fn(os.path.join(image_dir, name))
        if isinstance(out, dict):
            if vis is not None:
                extras[name] = out
            return out["proxy_rep"]
        if vis is not None:
            extras[name] = {"proxy_rep": out}
        return out

    def front_batch(names):
        """The batched front end on one group: its (B,18,D,D) proxy representations; per-image views for the pictures are kept."""
        paths = [os.path.join(image_dir, n) for n in names]
        if jpeg_decoder is None:
            images = [load_rgb_image(p) for p in paths]
        else:                                            # the group's device-profile JPEGs in one decode call, the rest on the host
            images = [encode_file(p) if p.lower().endswith((".jpg", ".jpeg")) else None for p in paths]
            picks = [i for i, im in enumerate(images) if im is not None]
            jpeg_decoder.check(wait=False)               # earlier groups, as far as they have finished
            for i, t in zip(picks, jpeg_decoder.decode([images[i] for i in picks]) if picks else []):
                images[i] = t
            images = [im if im is not None else load_rgb_image(p) for im, p in zip(images, paths)]
        out = batched(images, with_image=vis is not None and visualise_uncropped)
        if vis is not None:
            for b, n in enumerate(names):
                extras[n] = {"proxy_rep": out["proxy_rep"][b:b + 1], "cropped_rgb": out["cropped_rgb"][b:b + 1],
                             "joints2D": out["joints2D"][b:b + 1], "image": out["image"][b] if "image" in out else None,
                             "bbox_centre": out["bbox_centre"][b], "bbox_wh": out["bbox_wh"][b:b + 1]}
        return out["proxy_rep"]

    def visualise(name, item):
        ex = extras.pop(name)
        stem = os.path.join(save_dir, os.path.splitext(name)[0])
        proxy = ex["proxy_rep"]
        if not proxy.is_cuda:
            proxy = proxy.to(device, non_blocking=True)
        crop, joints = ex.get("cropped_rgb"), ex.get("joints2D")
        pictures = []                                    # the device encoder takes an image's pictures in one call
        write = (lambda image, path: pictures.append((image, path))) if on_device else writer.write
        write(vis.figure(item, crop, proxy.float(), joints), stem + suffix)
        if visualise_uncropped:
            if all(ex.get(k) is not None for k in ("image", "bbox_centre", "bbox_wh")):
                write(vis.uncropped(ex["image"], ex["bbox_centre"], ex["bbox_wh"]), stem + "_uncrop" + suffix)
            elif not warned:
                import warnings
                warned.append(True)
                warnings.warn("predict: proxy_rep_fn gave no image / bbox_centre / bbox_wh; the uncropped pictures are skipped")
        if visualise_samples:
            write(vis.samples_figure(item, crop, proxy.float()), stem + "_samples" + suffix)
        if pictures:
            writer.write_many([image for image, _ in pictures], [path for _, path in pictures])
    # The loop is software-pipelined (InferencePipeline): while batch k's head, sampling and meshes run, batch k+1's proxy
    # representations are already staged (page-locked host tensors go up by non-blocking copies on a copy stream, StagedUpload)
    # and its encoder is enqueued.  Same results as infer() per batch.
    groups = [image_fnames[i0:i0 + batch_size] for i0 in range(0, len(image_fnames), batch_size)]
    if not groups:
        return

    def deliver(names, res):
        cols = {key: val.unbind(0) for key, val in res.items()}      # per-image views, made once per key (not 17 x B index calls)
        for k, n in enumerate(names):
            item = {key: col[k] for key, col in cols.items()}
            if result_fn is not None:
                result_fn(n, item)
            else:
                keep = ("verts_mode", "joints_mode", "verts_tpose", "unc", "cam", "glob_rotmats")
                torch.save({key: item[key].cpu() for key in keep},
                           os.path.join(save_dir, os.path.splitext(n)[0] + ".pt"))
            if vis is not None:
                visualise(n, item)

    if batch_size <= 2 and device.type == "cuda":
        # The reference's own operating point -- one image per call (:58-59) -- is latency-bound: ~50 launches of a few microseconds
        # each, and the host needs longer to issue them than the device to run them.  Each (batch, num_samples) is captured ONCE in
        # hipGraphs (GraphedInfer, two slots on two streams); the loop issues image k + 1 before it waits for image k, so two replays
        # overlap on the mostly idle chip.  Same kernels, same order, same bits as infer().
        key = ("graph", num_samples, batch_size, torch.cuda.current_device())
        cached = _PREDICT_PIPELINES.get(pose_shape_model)
        if cached is None or cached[0] != key or cached[1].smpl is not smpl_model:
            cached = (key, GraphedInfer(weakref.proxy(pose_shape_model), smpl_model, batch_size, num_samples, use_mean_shape=True, slots=2), None)
            _PREDICT_PIPELINES[pose_shape_model] = cached
        graphed = cached[1]
        pending = None

        def finish_pending(p):
            names_p, res_p, done = p
            if done is not None:
                done.synchronize()                       # host wait (a stream-side wait polls beside the next replay: see GraphedInfer.__call__)
                # a replay's outputs are the slot's static buffers, overwritten two calls later: result_fn gets tensors of its own
                # (the reference hands each image's results on before the next image, and a callback may keep them)
                res_p = {key: (val.clone() if torch.is_tensor(val) else val) for key, val in res_p.items()}
            deliver(names_p, res_p)
        for gi, names in enumerate(groups):
            items = front_batch(names) if batched is not None else [get_proxy(n).float() for n in names]
            if len(items) == batch_size and tuple(items[0].shape[-3:]) == graphed.input_shape:
                if writer is not None and graphed._slots[graphed._k % len(graphed._slots)] is None:
                    writer.drain()                       # a capture is coming: no other thread may call the runtime during it
                nxt = (names,) + graphed(items, wait=False)
            else:                                        # a last, smaller group / another image size: the eager path
                x = items if batched is not None else torch.cat([t.to(device) for t in items], dim=0)
                nxt = (names, infer(pose_shape_model, smpl_model, x, num_samples=num_samples, use_mean_shape=True), None)
            if pending is not None:
                finish_pending(pending)
            pending = nxt
            if gi % 256 == 255:
                graphed.check_sampling()
        finish_pending(pending)
        graphed.check_sampling()
        check_sampling()
        if jpeg_decoder is not None:
            jpeg_decoder.check()
        if writer is not None:
            writer.close()
        return
    # the pipeline (its streams, the encoder's frame buffers bound to them, the upload slots) is kept between calls, per model (weakly
    # referenced side table: nothing is attached to the module, so copies / pickles of it are unaffected)
    key = (num_samples, batch_size, torch.cuda.current_device())
    cached = _PREDICT_PIPELINES.get(pose_shape_model)
    if cached is None or cached[0] != key or cached[1].smpl is not smpl_model:
        # the cached pipeline refers to the model through a weak proxy: a strong reference from the table's value to its key would
        # keep the model (and the encoder's frame buffers) alive for ever
        cached = (key, InferencePipeline(weakref.proxy(pose_shape_model), smpl_model, num_samples=num_samples, use_mean_shape=True),
                  StagedUpload(slots=2, copy_streams=2))      # 1: 9.4 k, 2: 10.7 k, 3: 10.4 k, 4: 9.5 k images/s at batch 64
        _PREDICT_PIPELINES[pose_shape_model] = cached
    _, pipe, stager = cached

    def stage(names):
        if batched is not None:                          # one front-end call per group, on the caller's stream: ordered by submit()'s default event
            return pipe.submit(front_batch(names))
        items = [get_proxy(n) for n in names]
        if all(t.is_cuda for t in items):                # built on the device (the reference front end): ordered by submit()'s default event
            return pipe.submit(torch.cat([t.float() for t in items], dim=0) if len(items) > 1 else items[0].float())
        proxy, ready = stager.upload_rows([t.float() for t in items])
        ticket = pipe.submit(proxy, input_ready=ready)
        stager.release(ticket[1])
        return ticket

    with torch.cuda.stream(pipe.caller_stream(batch_size)):
        ticket = stage(groups[0])
        for gi, names in enumerate(groups):
            nxt = stage(groups[gi + 1]) if gi + 1 < len(groups) else None
            res = pipe.finish(ticket, after=nxt)
            ticket = nxt
            if result_fn is None or gi % 64 == 63:
                check_sampling()                         # synchronises; with a result_fn the check is deferred (below) so the loop stays pipelined
            deliver(names, res)
        check_sampling()
        if jpeg_decoder is not None:
            jpeg_decoder.check()
    torch.cuda.current_stream().wait_stream(pipe.caller_stream(batch_size))
    if writer is not None:
        writer.close()


def use_batched_front_end(batched_front_end, proxy_rep_fn, device, hrnet_model, edge_detect_model):
    """predict_poseMF_shapeGaussian_net's ``batched_front_end`` rule: can the device front end of a whole group run, and is it wanted."""
    from .pose2D_hrnet import PoseHighResolutionNet
    why = None
    if proxy_rep_fn is not None:
        why = "a proxy_rep_fn replaces the whole front end"
    elif torch.device(device).type != "cuda":
        why = "the device is not a GPU"
    elif not isinstance(hrnet_model, PoseHighResolutionNet):
        why = "hrnet_model is not a pose2D_hrnet.PoseHighResolutionNet"
    elif not hasattr(edge_detect_model, "edge_map_into"):
        why = "edge_detect_model has no edge_map_into"
    if batched_front_end and why is not None:
        raise _capi.HpsError("batched_front_end=True, but %s" % why)
    return why is None and batched_front_end is not False


def load_rgb_image(path):
    """predict/...:63: the image as (H,W,3) uint8 RGB.  cv2 when it is installed (what the reference uses), PIL otherwise;
    ``.npy`` files holding such an array are accepted too."""
    import numpy as np
    if path.lower().endswith(".npy"):
        return np.load(path)
    try:
        import cv2
        return cv2.cvtColor(cv2.imread(path), cv2.COLOR_BGR2RGB)
    except ImportError:
        from PIL import Image
        return np.asarray(Image.open(path).convert("RGB"))


def _reference_front_end(pose_shape_cfg, hrnet_model, hrnet_cfg, edge_detect_model, object_detect_model,
                         joints2Dvisib_threshold, device):
    """predict/predict_poseMF_shapeGaussian_net.py:61-100 assembled from the injected reference-interface objects:
    image -> person box + HRNet keypoints (predict_hrnet) -> crop to the proxy-representation size -> Canny edges and
    visibility-masked Gaussian heat-maps (the hps_canny_edges / hps_proxy_rep kernels).  Returns image_path -> (1,18,D,D)."""
    from .predict_hrnet import predict_hrnet
    from .image_utils import batch_crop_pytorch_affine
    hrnet_model.eval()
    if object_detect_model is not None:
        object_detect_model.eval()
    D = pose_shape_cfg.DATA.PROXY_REP_SIZE

    staging = {"bufs": [None, None], "events": [None, None], "k": 0}

    def upload_u8(chw):
        """(3,H,W) uint8 host array -> device, through one of two reused page-locked buffers with a non-blocking copy: a quarter
        of the bytes of the reference's float upload (:65 converts on the host first), and the host does not wait for it."""
        import numpy as np
        k = staging["k"] % 2
        staging["k"] += 1
        n = chw.size
        if staging["bufs"][k] is None or staging["bufs"][k].numel() < n:
            staging["bufs"][k] = torch.empty(n, dtype=torch.uint8).pin_memory()
        if staging["events"][k] is not None:
            staging["events"][k].synchronize()            # the copy that last used this buffer (two images ago) has finished
        staging["bufs"][k][:n].copy_(torch.from_numpy(np.ascontiguousarray(chw)).reshape(-1))
        d = staging["bufs"][k][:n].to(device, non_blocking=True)
        staging["events"][k] = torch.cuda.Event()
        staging["events"][k].record()
        return d.view(chw.shape)

    @torch.no_grad()
    def run(image_path, extras):
        rgb_u8 = load_rgb_image(image_path).transpose(2, 0, 1)
        if torch.device(device).type == "cuda":
            image = upload_u8(rgb_u8).float() / 255.0                                                               # :63-65
        else:
            image = torch.from_numpy(rgb_u8.copy()).float().to(device) / 255.0
        hr = predict_hrnet(hrnet_model=hrnet_model, hrnet_config=hrnet_cfg, object_detect_model=object_detect_model,
                           image=image, object_detect_threshold=pose_shape_cfg.DATA.BBOX_THRESHOLD,
                           bbox_scale_factor=pose_shape_cfg.DATA.BBOX_SCALE_FACTOR)                                 # :67-72
        crop_h, crop_w = hr["cropped_image"].shape[1:]
        centre = torch.tensor([[crop_h, crop_w]], dtype=torch.float32, device=device) * 0.5                        # :75-78
        height = torch.tensor([crop_h], dtype=torch.float32, device=device)                                        # :79-81
        cropped = batch_crop_pytorch_affine(input_wh=(hrnet_cfg.MODEL.IMAGE_SIZE[0], hrnet_cfg.MODEL.IMAGE_SIZE[1]),
                                            output_wh=(D, D), num_to_crop=1, device=device, joints2D=hr["joints2D"][None],
                                            rgb=hr["cropped_image"][None], bbox_centres=centre, bbox_heights=height,
                                            bbox_widths=height.clone(), orig_scale_factor=1.0)                      # :82-91
        visib = hr["joints2Dconfs"] > joints2Dvisib_threshold                                                      # :98
        visib[[0, 1, 2, 3, 4, 5, 6, 11, 12]] = True                                                                # :99
        proxy = proxy_representation(cropped["rgb"], cropped["joints2D"], visib[None], edge_detect_model, pose_shape_cfg)
        if not extras:
            return proxy
        # what the pictures need beside the network's input (:198-201, :248-250, :280-292)
        side = torch.max(hr["bbox_height"], hr["bbox_width"]).reshape(1).float() * pose_shape_cfg.DATA.BBOX_SCALE_FACTOR
        return {"proxy_rep": proxy, "cropped_rgb": cropped["rgb"], "joints2D": cropped["joints2D"], "image": image,
                "bbox_centre": hr["bbox_centre"].reshape(2).float(), "bbox_wh": side}

    def front_end(image_path):
        return run(image_path, False)

    front_end.with_extras = lambda image_path: run(image_path, True)      # predict_poseMF_shapeGaussian_net(vis_renderer=...) takes the dict
    return front_end
