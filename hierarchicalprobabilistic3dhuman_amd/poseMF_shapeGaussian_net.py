"""``PoseMFShapeGaussianNet`` with the constructor, state-dict layout and forward contract of the
reference's models/poseMF_shapeGaussian_net.py, executed by libhps.so.

    net = PoseMFShapeGaussianNet(smpl_parents=smpl.parents.tolist(), config=cfg).to(device).eval()
    net.load_state_dict(checkpoint['best_model_state_dict'])
    pose_F, pose_U, pose_S, pose_V, pose_rotmats_mode, shape_dist, glob, cam = net(proxy_rep_input)

Execution: ResNet-18 encoder (resnet.py) -> FC trunk (hps_linear) -> the 23 per-joint MLPs grouped into
kinematic depth levels (hps_head_joint_level; 8 levels for the SMPL tree instead of 23 sequential steps)
-> 3x3 SVD -> proper-SVD fix and mode (hps_head_svd_finish).

3x3 SVD (:137, "SVD is faster on CPU" in the reference).  The column signs LAPACK returns are not determined by the
mathematics, they feed the child joints' MLPs through U_proper (:126-130), and the trained weights were fitted to them
(SURVEY.md section 7 hard part 1).  Two modes, ``net.svd_mode``:
  "device" (default)  the SVD runs inside the level kernel and follows LAPACK's sgesdd step by step WITH MKL'S ROUNDINGS
                      (csrc/svd3_gesdd.h): U, S and V are bit-identical to torch.svd on this host (10^6 matrices of 22 families,
                      tests/test_host_logic.py).  MKL rounds differently on Intel and on other hosts (fused multiply-adds or
                      not -- one differently signed vector pair in 10^4 matrices between the two, i.e. the reference itself is
                      only reproducible across hosts to that level); ``svd_flavor`` = None takes the flavour of this host,
                      0 / 1 force the reference-BLAS / fused one.  The head is 11 stream-ordered launches, no host
                      synchronisation.
  "host"              the reference's very routine: MKL sgesdd on the host, one D2H / sync / H2D round trip per kinematic
                      level.

Training (the reference's step, train/train_poseMF_shapeGaussian_net.py:262-349).  With grad mode on and ``input_feats`` or a head
parameter requiring grad, the head runs inside a torch.autograd.Function: its forward launches exactly the kernels of a no_grad
call (same bits for all eight outputs, in either latency mode and either SVD mode), its backward is hps_head_forward_refine (the head
again in float64), hps_head_pose_levels_backward and hps_head_trunk_backward (csrc/head_backward.hip) and needs only the features and
the saved pose_U's signs, so the host-SVD mode is differentiable
too.  By default ``pose_U`` and ``pose_V`` are marked non-differentiable (the stage-1 loss detaches them);
``set_differentiable_factors(True)`` makes them differentiable outputs as in the reference, for its stage-2 step
(train/train_poseMF_shapeGaussian_net.py:292-320): the reparameterised sampler (sampling_utils.pose_matrix_fisher_sampling_torch) hands
its cotangents of the raw factors to the head's backward, where they join torch.svd's backward (hps_head_pose_levels_backward_factors).
With ``input`` given the encoder is part of the graph too (resnet.py: its own autograd function, device
backward kernels): the loss reaches every convolution and BatchNorm affine parameter and the input itself.  By default that is fine-tuning with
frozen BatchNorm statistics (eval mode; ``.train()`` is refused); ``set_batchnorm_training(True)`` followed by ``.train()`` is the
reference's ``model.train()`` step: batch statistics in the forward, running buffers updated on the device, the backward through the
statistics (csrc/bn_train.hip).
From the first differentiable forward on, the module compares its head parameters' ``_version`` counters with the ones recorded by
``prepare()`` on every forward (no_grad ones included) and rebuilds the kernel-side copies when an optimiser step changed them;
modules that never take the differentiable route do not look and behave as before.
"""
import os

import torch
from torch import nn
from torch.distributions import Normal

from . import _capi
from .device_optim import RefreshList, plain
from .device_state import DeviceStateModule
from .resnet import resnet18, resnet50
from .rigid_transform_utils import rotmat_to_rot6d
from .sharding import effective_cpus


# host SVD pool size: half the usable hardware threads (cgroup quota aware), shared between the ranks torchrun started on this node
_SVD_THREADS = max(2, min(16, effective_cpus() // (2 * max(1, int(os.environ.get("LOCAL_WORLD_SIZE", "1"))))))


def _host_svd_packed(f_host, usv_host):
    """SVD of n 3x3 matrices on the host (f_host (n,3,3) -> usv_host (n,21) packed [U | S | V]) through
    hps_host_svd3_packed: the same MKL sgesdd_ torch.svd calls, bit-identical factors, but the independent
    matrices are spread over a small native thread pool (torch's batched CPU SVD is a sequential loop,
    ~1.7 us per matrix)."""
    n = f_host.shape[0]
    assert f_host.is_contiguous() and usv_host.is_contiguous() and not f_host.is_cuda
    _capi.call("hps_host_svd3_packed", _capi._P(f_host.data_ptr()), _capi._P(usv_host.data_ptr()), n, _SVD_THREADS)


def immediate_parents_to_all_parents(immediate_parents):
    """models/poseMF_shapeGaussian_net.py:14-21: for every body joint (SMPL joint - 1) the list of its
    ancestors, nearest first, the root excluded.  Returned as a plain dict joint -> list."""
    all_parents = {}
    for smpl_idx in range(1, len(immediate_parents)):
        joint, parent = smpl_idx - 1, immediate_parents[smpl_idx] - 1
        all_parents[joint] = [parent] + all_parents[parent] if parent >= 0 else []
    return all_parents


class _RefinedHead:
    """The float64 pass of one differentiable forward (PoseMFShapeGaussianNet._refine), run at most once, by whichever backward asks
    first: the head's own, or the reparameterised sampler's (sampling_utils._SampleFunction), which differentiates at the float64 factors
    for the reason the head does -- the fp32 factors are off by 2^-23 / (gap of the singular values), and the sampler's second derivative
    turns that into the gradient's error.  Travels on the factor tensors a forward with set_differentiable_factors(True) returns."""

    def __init__(self, net, p, feats, pose_U, pose_S, pose_V):
        self.net, self.p = net, p
        self.feats, self.pose_U = feats.detach(), pose_U.detach()
        self.ptrs = (pose_U.data_ptr(), pose_S.data_ptr(), pose_V.data_ptr())
        self.result = None

    def get(self):
        if self.result is None:
            self.result = self.net._refine(self.p, self.feats, self.pose_U)
            self.feats = self.pose_U = None
        return self.result


class _HeadFunction(torch.autograd.Function):
    """The head (:95-162) for autograd: forward = the module's own kernel sequence, backward = the head again in float64 and the two device
    backward composites (_head_backward), without the kernels whose result ``ctx.needs_input_grad`` does not ask for.
    Inputs after ``feats``: the head parameters in the order of ``PoseMFShapeGaussianNet._head_params()``."""

    @staticmethod
    def forward(ctx, net, p, feats, *params):
        outs = net._head(feats, p)
        pose_F, pose_U, pose_S, pose_V, mode, loc, scale, glob, cam = outs
        ctx.net, ctx.p = net, p                        # p owns the kernel-side weights the backward reads
        ctx.save_for_backward(feats, pose_U, scale, *params)      # the backward evaluates the head again (in float64) from these
        ctx.refined = None
        if net.differentiable_factors:
            ctx.refined = _RefinedHead(net, p, feats, pose_U, pose_S, pose_V)
        else:
            ctx.mark_non_differentiable(pose_U, pose_V)
        ctx.set_materialize_grads(False)               # an output without a cotangent arrives as None: a NULL pointer for the kernels
        return outs

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_F, g_U, g_S, g_V, g_mode, g_loc, g_scale, g_glob, g_cam):
        feats, pose_U, scale = ctx.saved_tensors[:3]
        need = ctx.needs_input_grad
        g_feats, g_params = ctx.net._head_backward(ctx.p, feats, pose_U, scale, g_F, g_S, g_mode, g_loc, g_scale, g_glob, g_cam,
                                                   want_feats=need[2], want_params=any(need[3:]), g_U=g_U, g_V=g_V, refined=ctx.refined)
        if g_params is None:
            return (None, None, g_feats) + (None,) * len(need[3:])
        return (None, None, g_feats) + tuple(g if n else None for g, n in zip(g_params, need[3:]))


class PoseMFShapeGaussianNet(DeviceStateModule):
    SWITCHES = ("latency_mode", "svd_mode", "svd_flavor", "composite_head")

    def __init__(self, smpl_parents, config):
        super().__init__()
        self.config = config
        self.parents_dict = immediate_parents_to_all_parents(smpl_parents)
        self.num_joints = len(self.parents_dict)
        self.num_pose_params = self.num_joints * 9
        self.num_shape_params = config.MODEL.NUM_SMPL_BETAS
        self.num_glob_params = 6
        self.num_cam_params = 3
        self.register_buffer("init_glob", rotmat_to_rot6d(torch.eye(3)[None, :].float()))
        self.register_buffer("init_cam", torch.tensor([0.9, 0.0, 0.0]).float())

        # models/poseMF_shapeGaussian_net.py:53-62
        if config.MODEL.NUM_RESNET_LAYERS == 18:
            self.image_encoder = resnet18(in_channels=config.MODEL.NUM_IN_CHANNELS, pretrained=False)
            num_image_features, fc1_dim = 512, 512
        elif config.MODEL.NUM_RESNET_LAYERS == 50:          # forward only (resnet.ResNet)
            self.image_encoder = resnet50(in_channels=config.MODEL.NUM_IN_CHANNELS, pretrained=False)
            num_image_features, fc1_dim = 2048, 1024
        else:
            raise ValueError("MODEL.NUM_RESNET_LAYERS must be 18 or 50, got %r" % (config.MODEL.NUM_RESNET_LAYERS,))
        embed_dim = config.MODEL.EMBED_DIM

        self.activation = nn.ELU()
        self.fc1 = nn.Linear(num_image_features, fc1_dim)
        self.fc_shape = nn.Linear(fc1_dim, self.num_shape_params * 2)
        self.fc_glob = nn.Linear(fc1_dim, self.num_glob_params)
        self.fc_cam = nn.Linear(fc1_dim, self.num_cam_params)
        self.fc_embed = nn.Linear(num_image_features + self.num_shape_params * 2 + self.num_glob_params
                                  + self.num_cam_params, embed_dim)
        self.fc_pose = nn.ModuleList()
        for joint in range(self.num_joints):
            in_dim = embed_dim + len(self.parents_dict[joint]) * (9 + 3 + 9)
            self.fc_pose.append(nn.Sequential(nn.Linear(in_dim, embed_dim // 2), self.activation,
                                              nn.Linear(embed_dim // 2, 9)))
        # kinematic depth levels: joints whose ancestors are all in earlier levels
        depth = [len(self.parents_dict[j]) for j in range(self.num_joints)]
        self.levels = [[j for j in range(self.num_joints) if depth[j] == d] for d in range(max(depth) + 1)]
        self._pinned_bufs = {}
        self.composite_head = True     # joint loop through hps_head_pose_levels (one call) instead of per-level Python
        self.svd_mode = "device"       # "device": in-kernel gesdd-faithful SVD; "host": MKL sgesdd round trip (the routine itself)
        self.svd_flavor = None         # None: the rounding flavour of this host's MKL (calibrated); 0 / 1 force one
        self.latency_mode = False      # set_latency_mode(): encoder on direct kernels with many K slices, joint MLPs on wide workgroups
        self.differentiable_factors = False   # set_differentiable_factors(): pose_U / pose_V carry a gradient (the stage-2 step)
        self._track_versions = False   # set by the first differentiable forward: parameters may now change in place (optimiser steps)

    def set_latency_mode(self, on=True):
        """One switch for one-image-at-a-time deployments (the reference's run_predict operating point): the encoder's latency mode
        (ResNet.set_latency_mode) and 1024-thread / eight-K-slice workgroups for the joint MLPs of the head
        (HPS_HEAD_WIDE_WORKGROUPS; device SVD mode only).  A property of the model: within a mode results do not depend on the
        batch size; between the modes they differ in the last bits (other summation orders)."""
        self.latency_mode = bool(on)
        self.image_encoder.set_latency_mode(on)

    def set_batchnorm_training(self, on=True):
        """Opt in to the reference's ``model.train()`` step (train/train_poseMF_shapeGaussian_net.py:114): the encoder's BatchNorm layers
        whose ``.training`` is set run on batch statistics and update their running buffers (ResNet.set_batchnorm_training).  Off, the
        default, ``.train()`` stays refused."""
        self.image_encoder.set_batchnorm_training(on)

    def set_differentiable_encoder(self, on=True):
        """Opt a net with the Bottleneck (MODEL.NUM_RESNET_LAYERS = 50) encoder in to the encoder's backward, its training-mode
        BatchNorm, its in-place weight refresh and the training loop (ResNet.set_differentiable); a no-op for the 18-layer encoder, which
        always is."""
        self.image_encoder.set_differentiable(on)

    def set_differentiable_factors(self, on=True):
        """Opt in to ``pose_U`` / ``pose_V`` as differentiable outputs, as the reference's stage-2 step needs them
        (train/train_poseMF_shapeGaussian_net.py:292-320: the sampled rotations depend on them, utils/sampling_utils.py:105-111, 140-141).
        Off, the default, they are marked non-differentiable.  The forward's launches and bits are the same either way."""
        self.differentiable_factors = bool(on)

    def _flavor(self):
        """Rounding flavour of the in-kernel SVD: ``svd_flavor`` if set (0 reference BLAS rounding, 1 fused), else the one that
        reproduces this host's LAPACK bit for bit (_capi.svd_flavor)."""
        return _capi.svd_flavor() if self.svd_flavor is None else int(self.svd_flavor)

    def __getstate__(self):
        # copy.deepcopy / pickle: the staging buffers are page-locked host memory -- a copy makes its own
        state = super().__getstate__()
        state["_pinned_bufs"] = {}
        return state

    def _pinned(self, name, numel):
        """Reusable page-locked host staging buffer (fp32) of at least ``numel`` elements, one per (name, stream): the last
        level's upload is still in flight when forward returns, and only a later forward ON THE SAME STREAM is ordered
        behind it (its first stream synchronisation retires the copy) -- a forward on another stream gets its own buffer."""
        stream = torch.cuda.current_stream()
        key = (name, stream.cuda_stream)
        buf = self._pinned_bufs.get(key)
        if buf is None or buf.numel() < numel:
            if buf is not None:
                stream.synchronize()          # never free a staging block with a copy in flight
            buf = torch.empty(max(numel, 1024), dtype=torch.float32, pin_memory=True)
            self._pinned_bufs[key] = buf
        return buf[:numel]

    # ---- kernel-side weights; rebuilt after .to() / load_state_dict / a switch ----
    def prepare(self):
        dev = self.fc1.weight.device
        t = lambda w: w.detach().float().t().contiguous()
        c = lambda w: w.detach().float().contiguous()
        nsh, ng, nc = self.num_shape_params * 2, self.num_glob_params, self.num_cam_params
        p = {}
        p["fc1_wt"], p["fc1_b"] = t(self.fc1.weight), c(self.fc1.bias)
        # fc_shape | fc_glob | fc_cam fused into one (fc1_dim -> 29) layer; init_glob / init_cam as addend
        p["sgc_wt"] = t(torch.cat([self.fc_shape.weight, self.fc_glob.weight, self.fc_cam.weight], dim=0))
        p["sgc_b"] = c(torch.cat([self.fc_shape.bias, self.fc_glob.bias, self.fc_cam.bias]))
        p["sgc_add"] = c(torch.cat([torch.zeros(nsh, device=dev), self.init_glob.reshape(-1), self.init_cam.reshape(-1)]))
        p["embed_wt"], p["embed_b"] = t(self.fc_embed.weight), c(self.fc_embed.bias)
        w1t = [t(m[0].weight) for m in self.fc_pose]
        b1 = [c(m[0].bias) for m in self.fc_pose]
        w2 = [c(m[2].weight) for m in self.fc_pose]
        b2 = [c(m[2].bias) for m in self.fc_pose]
        p["keep"] = (w1t, b1, w2, b2)                      # owners of the device memory behind the pointer tables
        ptrs = lambda ts: torch.tensor([x.data_ptr() for x in ts], dtype=torch.int64, device=dev)
        p["w1t_ptrs"], p["b1_ptrs"], p["w2_ptrs"], p["b2_ptrs"] = ptrs(w1t), ptrs(b1), ptrs(w2), ptrs(b2)
        anc_ptr, anc_idx = [0], []
        for j in range(self.num_joints):
            anc_idx.extend(self.parents_dict[j])
            anc_ptr.append(len(anc_idx))
        p["anc_ptr"] = torch.tensor(anc_ptr, dtype=torch.int32, device=dev)
        p["anc_idx"] = torch.tensor(anc_idx if anc_idx else [0], dtype=torch.int32, device=dev)
        p["levels"] = [torch.tensor(l, dtype=torch.int32, device=dev) for l in self.levels]
        p["level_joints"] = torch.tensor([j for l in self.levels for j in l], dtype=torch.int32, device=dev)
        p["level_sizes_host"] = torch.tensor([len(l) for l in self.levels], dtype=torch.int32)
        p["max_level_size"] = max(len(l) for l in self.levels)
        if self._track_versions:
            p["versions"] = self._head_versions()
        self._prepared = p
        return p

    def _head_params(self):
        """The head's parameters in the order _HeadFunction takes them and _head_backward returns their gradients."""
        ps = [self.fc1.weight, self.fc1.bias, self.fc_shape.weight, self.fc_shape.bias, self.fc_glob.weight, self.fc_glob.bias,
              self.fc_cam.weight, self.fc_cam.bias, self.fc_embed.weight, self.fc_embed.bias]
        for m in self.fc_pose:
            ps += [m[0].weight, m[0].bias, m[2].weight, m[2].bias]
        return ps

    def _head_versions(self):
        return tuple(w._version for w in self._head_params())

    # ---- after an optimiser step that says so (device_optim.DeviceAdam): the derived weights again, in place ----
    def _refresh_list(self, p, token):
        """One hps_refresh_op per tensor prepare() / _prepare_backward derive from a parameter by more than an alias: the transposed
        copies, the fused fc_shape | fc_glob | fc_cam layer; the copies nn.Linear's own layout needs only where the parameter is not
        what the kernels read already (RefreshList.copy: nothing for an alias)."""
        ref = RefreshList(token)
        q = p.get("bwd")
        ref.transpose(self.fc1.weight, p["fc1_wt"])
        ref.copy(self.fc1.bias, p["fc1_b"])
        nt, row = p["sgc_b"].numel(), 0
        for m in (self.fc_shape, self.fc_glob, self.fc_cam):
            ref.transpose(m.weight, p["sgc_wt"], offset=row, ld=nt)
            ref.copy(m.bias, p["sgc_b"], offset=row)
            if q is not None:
                ref.copy(m.weight, q["sgc_w"], offset=row * m.weight.shape[1])
            row += m.weight.shape[0]
        ref.transpose(self.fc_embed.weight, p["embed_wt"])
        ref.copy(self.fc_embed.bias, p["embed_b"])
        if q is not None:
            ref.copy(self.fc1.weight, q["fc1_w"])
            ref.copy(self.fc_embed.weight, q["embed_w"])
        w1t, b1, w2, b2 = p["keep"]
        for j, m in enumerate(self.fc_pose):
            ref.transpose(m[0].weight, w1t[j])
            ref.copy(m[0].bias, b1[j])
            ref.copy(m[2].weight, w2[j])
            ref.copy(m[2].bias, b2[j])
        return ref

    def refresh_weights(self):
        """The encoder's refresh (ResNet.refresh_weights), then the head's: every kernel-side copy of a head parameter written again
        in place (hps_weights_refresh) and the version counters recorded, so that the next forward keeps the prepared state with its
        pointer tables.  Without a prepared state: nothing to do."""
        self.image_encoder.refresh_weights()
        p = self._prepared
        if p is None:
            return
        params = self._head_params()
        if not all(w.is_cuda and plain(w) for w in params):
            self.invalidate()
            return
        token = (tuple(w.data_ptr() for w in params), "bwd" in p)
        ref = self._device_state.get("refresh")
        if ref is not None and ref.token[0] != token[0]:
            self.invalidate()
            return
        if ref is None or ref.token != token:
            ref = self._device_state["refresh"] = self._refresh_list(p, token)
        ref.run()
        p["versions"] = self._head_versions()

    def _prepare_backward(self, p):
        """What only the backward needs, built at the first backward of a prepared state: the weights in nn.Linear's own layout (the
        forward holds them transposed), the descendant table (who reads joint a's U_proper / S_proper / mode, and at which position of
        its ancestor list) and the offsets of the joints' MLP inputs."""
        q = p.get("bwd")
        if q is not None:
            return q
        dev = self.fc1.weight.device
        c = lambda w: w.detach().float().contiguous()
        i32 = lambda v: torch.tensor(v if v else [0], dtype=torch.int32, device=dev)
        nj, embed_dim = self.num_joints, self.config.MODEL.EMBED_DIM
        desc_ptr, desc_joint, desc_pos = [0], [], []
        for a in range(nj):
            for d in range(nj):
                if a in self.parents_dict[d]:
                    desc_joint.append(d)
                    desc_pos.append(self.parents_dict[d].index(a))
            desc_ptr.append(len(desc_joint))
        in_off = [0]
        for j in range(nj):
            in_off.append(in_off[-1] + embed_dim + 21 * len(self.parents_dict[j]))
        q = dict(fc1_w=c(self.fc1.weight), embed_w=c(self.fc_embed.weight),
                 sgc_w=c(torch.cat([self.fc_shape.weight, self.fc_glob.weight, self.fc_cam.weight], dim=0)),
                 desc_ptr=i32(desc_ptr), desc_joint=i32(desc_joint), desc_pos=i32(desc_pos), in_off=i32(in_off),
                 in_off_host=in_off, total_in=in_off[-1])
        p["bwd"] = q
        return q

    def _refine(self, p, feats, pose_U):
        """hps_head_forward_refine: the head again in float64 from the fp32 features (signs of the singular vectors from ``pose_U``), the
        values the backward differentiates at.  Returns its outputs by name."""
        B, dev = feats.shape[0], feats.device
        nj, embed_dim = self.num_joints, self.config.MODEL.EMBED_DIM
        nt = 2 * self.num_shape_params + self.num_glob_params + self.num_cam_params
        nf, hidden = feats.shape[1], p["fc1_wt"].shape[1]
        P, VP, s = _capi.ptr, _capi._P, _capi.stream()
        f32 = dict(device=dev, dtype=torch.float32)
        f64 = dict(device=dev, dtype=torch.float64)
        D = lambda t: _capi.ptr(t, torch.float64)
        delta = float(self.config.MODEL.DELTA_I_WEIGHT) if self.config.MODEL.DELTA_I else 0.0
        x_f, sgc_f, embed_f = torch.empty(B, hidden, **f32), torch.empty(B, nt, **f32), torch.empty(B, embed_dim, **f32)
        x_d, sgc_d, embed_d = torch.empty(B, hidden, **f64), torch.empty(B, nt, **f64), torch.empty(B, embed_dim, **f64)
        Up_d, Sp_d, mode_d = torch.empty(B, nj, 9, **f64), torch.empty(B, nj, 3, **f64), torch.empty(B, nj, 9, **f64)
        U_d, S_d, V_d = torch.empty(B, nj, 9, **f64), torch.empty(B, nj, 3, **f64), torch.empty(B, nj, 9, **f64)
        _capi.call("hps_head_forward_refine", P(feats), nf, P(p["fc1_wt"]), P(p["fc1_b"]), P(p["sgc_wt"]), P(p["sgc_b"]), P(p["sgc_add"]),
                   P(p["embed_wt"]), P(p["embed_b"]), _capi.iptr(p["level_joints"]), VP(p["level_sizes_host"].data_ptr()),
                   len(p["levels"]), _capi.iptr(p["anc_ptr"]), _capi.iptr(p["anc_idx"]), VP(p["w1t_ptrs"].data_ptr()),
                   VP(p["b1_ptrs"].data_ptr()), VP(p["w2_ptrs"].data_ptr()), VP(p["b2_ptrs"].data_ptr()), delta, P(pose_U), P(x_f),
                   P(sgc_f), P(embed_f), D(x_d), D(sgc_d), D(embed_d), D(Up_d), D(Sp_d), D(mode_d), D(U_d), D(S_d), D(V_d), B, nf, hidden,
                   nt, embed_dim, embed_dim // 2, nj, s)
        return dict(x_f=x_f, sgc_f=sgc_f, embed_f=embed_f, embed_d=embed_d, Up_d=Up_d, Sp_d=Sp_d, mode_d=mode_d, U_d=U_d, S_d=S_d, V_d=V_d)

    def _head_backward(self, p, feats, pose_U, scale, g_F, g_S, g_mode, g_loc, g_scale, g_glob, g_cam, want_feats=True, want_params=True,
                       g_U=None, g_V=None, refined=None):
        """(g_feats, parameter gradients in _head_params() order) from the cotangents of pose_F, pose_S, pose_rotmats_mode, the
        Gaussian's loc / scale, glob and cam, and of the raw factors pose_U / pose_V (``g_U`` / ``g_V``) (None = zero): hps_head_forward_refine (the forward again in float64, signs of the singular
        vectors from the saved pose_U), hps_head_pose_levels_backward_factors, then hps_head_trunk_backward.  ``want_feats`` / ``want_params``
        False (frozen features / all head parameters frozen): that result is None and its kernels are not launched.  ``refined``: the
        step's _RefinedHead when the sampler's backward may already have run the float64 pass (it is run once)."""
        q = self._prepare_backward(p)
        B, dev = feats.shape[0], feats.device
        nj, embed_dim = self.num_joints, self.config.MODEL.EMBED_DIM
        nsh, ng, nc = self.num_shape_params, self.num_glob_params, self.num_cam_params
        nt = 2 * nsh + ng + nc
        nf, hidden = feats.shape[1], p["fc1_wt"].shape[1]
        P, VP, s = _capi.ptr, _capi._P, _capi.stream()
        f32 = dict(device=dev, dtype=torch.float32)
        G = lambda g: None if g is None else _capi.f32c(g)
        g_F, g_S, g_mode, g_loc, g_scale, g_glob, g_cam = G(g_F), G(g_S), G(g_mode), G(g_loc), G(g_scale), G(g_glob), G(g_cam)
        g_U, g_V = G(g_U), G(g_V)
        tail = embed_dim // 2 + 9 * (embed_dim // 2) + 9
        D = lambda t: _capi.ptr(t, torch.float64)
        r = refined.get() if refined is not None else self._refine(p, feats, pose_U)
        x_f, sgc_f, embed_f, embed_d = r["x_f"], r["sgc_f"], r["embed_f"], r["embed_d"]
        Up_d, Sp_d, mode_d, U_d, S_d, V_d = r["Up_d"], r["Sp_d"], r["mode_d"], r["U_d"], r["S_d"], r["V_d"]
        g_embed = torch.empty(B, embed_dim, **f32)
        # one flat buffer for the 92 fc_pose gradients (one allocation, one launch); the tensors handed out are views of it
        g_pose = torch.empty((embed_dim // 2) * q["total_in"] + nj * tail, **f32) if want_params else None
        ws = torch.empty(_capi.query_workspace(_capi.WS_HEAD_LEVELS_BWD, B, q["total_in"], nj) // 4, **f32)
        _capi.call("hps_head_pose_levels_backward_factors", D(embed_d), embed_dim, embed_dim // 2, _capi.iptr(p["level_joints"]),
                   VP(p["level_sizes_host"].data_ptr()), len(p["levels"]), _capi.iptr(p["anc_ptr"]), _capi.iptr(p["anc_idx"]),
                   _capi.iptr(q["desc_ptr"]), _capi.iptr(q["desc_joint"]), _capi.iptr(q["desc_pos"]), _capi.iptr(q["in_off"]),
                   VP(p["w1t_ptrs"].data_ptr()), VP(p["b1_ptrs"].data_ptr()), VP(p["w2_ptrs"].data_ptr()), D(Up_d), D(Sp_d),
                   D(mode_d), D(U_d), D(S_d), D(V_d), P(g_F), P(g_S), P(g_mode), P(g_U), P(g_V), P(g_embed), P(g_pose), P(ws), B, nj,
                   q["total_in"], s)
        E = lambda *shape: torch.empty(*shape, **f32) if want_params else None
        g_feats = torch.empty(B, nf, **f32) if want_feats else None
        g_fc1_w, g_fc1_b = E(hidden, nf), E(hidden)
        g_sgc_w, g_sgc_b = E(nt, hidden), E(nt)
        g_embed_w, g_embed_b = E(embed_dim, nf + nt), E(embed_dim)
        ws2 = torch.empty(_capi.query_workspace(_capi.WS_HEAD_TRUNK_BWD, B, nf + hidden + embed_dim, nt) // 4, **f32)
        _capi.call("hps_head_trunk_backward", P(feats), nf, P(x_f), P(sgc_f), P(embed_f), P(scale), P(q["fc1_w"]), P(q["sgc_w"]),
                   P(q["embed_w"]), P(g_embed), P(g_loc), P(g_scale), P(g_glob), P(g_cam), P(g_feats), P(g_fc1_w), P(g_fc1_b),
                   P(g_sgc_w), P(g_sgc_b), P(g_embed_w), P(g_embed_b), P(ws2), B, nf, hidden, nsh, ng, nc, embed_dim, s)
        if not want_params:
            return g_feats, None
        a, b = 2 * nsh, 2 * nsh + ng
        grads = [g_fc1_w, g_fc1_b, g_sgc_w[:a], g_sgc_b[:a], g_sgc_w[a:b], g_sgc_b[a:b], g_sgc_w[b:], g_sgc_b[b:], g_embed_w, g_embed_b]
        hid = embed_dim // 2
        for j in range(nj):
            o = hid * q["in_off_host"][j] + j * tail
            in_dim = q["in_off_host"][j + 1] - q["in_off_host"][j]
            grads += [g_pose[o:o + hid * in_dim].view(hid, in_dim), g_pose[o + hid * in_dim:o + hid * in_dim + hid],
                      g_pose[o + hid * in_dim + hid:o + hid * in_dim + hid + 9 * hid].view(9, hid), g_pose[o + hid * in_dim + 10 * hid:o + hid * in_dim + 10 * hid + 9]]
        return g_feats, grads

    # ------------------------------------------------------------------------------------------
    def _trunk(self, feats, p):
        """(embed, the Gaussian over the betas, glob, cam) of _trunk_launch."""
        embed, loc, scale, glob, cam = self._trunk_launch(feats, p)
        return embed, Normal(loc=loc, scale=scale, validate_args=False), glob, cam

    def _trunk_launch(self, feats, p):
        """:95-110: fc1 / ELU, the Gaussian over the betas, glob, cam, the embedding -- three launches (hps_head_trunk); the Gaussian's
        mean / exp(log std), glob and cam come out contiguous: no concatenation buffer, no torch.exp, no clones on the head's stream.
        Returns embed, loc, scale, glob, cam."""
        B, dev = feats.shape[0], feats.device
        nsh, ng, nc = self.num_shape_params * 2, self.num_glob_params, self.num_cam_params
        embed_dim = self.config.MODEL.EMBED_DIM
        P, s = _capi.ptr, _capi.stream()
        f32 = dict(device=dev, dtype=torch.float32)
        nf = feats.shape[1]
        hidden = p["fc1_wt"].shape[1]
        x = torch.empty(B, hidden, **f32)
        sgc = torch.empty(B, nsh + ng + nc, **f32)
        embed = torch.empty(B, embed_dim, **f32)
        shape_mean = torch.empty(B, self.num_shape_params, **f32)
        shape_scale = torch.empty(B, self.num_shape_params, **f32)
        glob = torch.empty(B, ng, **f32)
        cam = torch.empty(B, nc, **f32)
        _capi.call("hps_head_trunk", P(feats), nf, P(p["fc1_wt"]), P(p["fc1_b"]), P(p["sgc_wt"]), P(p["sgc_b"]), P(p["sgc_add"]),
                   P(p["embed_wt"]), P(p["embed_b"]), P(x), P(sgc), P(embed), P(shape_mean), P(shape_scale), P(glob), P(cam), B, nf,
                   hidden, self.num_shape_params, ng, nc, embed_dim, s)
        return embed, shape_mean, shape_scale, glob, cam

    def _pose_buffers(self, B, dev):
        """pose_F, pose_U, pose_S, pose_V, U_proper, S_proper, mode: every joint is in exactly one level and ancestors come from earlier
        levels, so all entries are written before they are read -- no zero fill (seven launches less on the head's stream)."""
        f32 = dict(device=dev, dtype=torch.float32)
        nj = self.num_joints
        return (torch.empty(B, nj, 3, 3, **f32), torch.empty(B, nj, 3, 3, **f32), torch.empty(B, nj, 3, **f32),
                torch.empty(B, nj, 3, 3, **f32), torch.empty(B, nj, 3, 3, **f32), torch.empty(B, nj, 3, **f32),
                torch.empty(B, nj, 3, 3, **f32))

    def forward(self, input, input_feats=None):
        """models/poseMF_shapeGaussian_net.py:85-162.  input: (B,C,D,D); ``input_feats`` skips the encoder.

        Differentiable with respect to ``input_feats`` and the head's parameters (module docstring); ``pose_U`` / ``pose_V`` carry a
        gradient only after ``set_differentiable_factors(True)``.  With ``input`` given the chain goes on through the encoder (ResNet.forward is differentiable with respect to its
        input and its convolution / BatchNorm affine parameters, eval-mode statistics)."""
        if input_feats is None:
            input_feats = self.image_encoder(input)
        _capi.require_device(input_feats, "input_feats")
        differentiable = torch.is_grad_enabled() and (input_feats.requires_grad or any(w.requires_grad for w in self._head_params()))
        if differentiable:
            self._track_versions = True
        if self._track_versions and self._prepared is not None and self._prepared.get("versions") != self._head_versions():
            self.invalidate()                                     # an optimiser step (or any in-place edit) since prepare()
        p = self._prepared or self.prepare()
        feats = _capi.f32c(input_feats)
        if differentiable:
            outs = _HeadFunction.apply(self, p, feats, *self._head_params())
            refined = outs[1].grad_fn.refined if outs[1].grad_fn is not None else None
            if refined is not None:                           # for the sampler's backward (sampling_utils._SampleFunction)
                for t in outs[1:4]:
                    t._hps_refined = refined
        else:
            outs = self._head(feats, p)
        pose_F, pose_U, pose_S, pose_V, mode, loc, scale, glob, cam = outs
        return pose_F, pose_U, pose_S, pose_V, mode, Normal(loc=loc, scale=scale, validate_args=False), glob, cam

    def _head(self, feats, p):
        """The head's launches on fp32 contiguous features: (pose_F, pose_U, pose_S, pose_V, mode, loc, scale, glob, cam)."""
        B = feats.shape[0]
        dev = feats.device
        nj = self.num_joints
        embed_dim = self.config.MODEL.EMBED_DIM
        P, s = _capi.ptr, _capi.stream()
        f32 = dict(device=dev, dtype=torch.float32)
        embed, loc, scale, glob, cam = self._trunk_launch(feats, p)

        # hierarchical pose prediction (:121-160), one kinematic level at a time
        pose_F, pose_U, pose_S, pose_V, U_proper, S_proper, mode = self._pose_buffers(B, dev)
        delta = float(self.config.MODEL.DELTA_I_WEIGHT) if self.config.MODEL.DELTA_I else 0.0
        stream = torch.cuda.current_stream()
        if self.svd_mode not in ("device", "host"):
            raise ValueError("svd_mode must be 'device' or 'host'")
        device_svd = self.svd_mode == "device"
        if self.composite_head:
            # the whole joint loop in one call across the C ABI (csrc/composite.hip: same launches, same order)
            sizes = p["level_sizes_host"]
            max_n = p["max_level_size"]
            VP = _capi._P
            if device_svd:
                f_dev = usv_dev = None
                fh = uh = None
            else:
                n_f = _capi.query_workspace(_capi.WS_HEAD_F, B, max_n) // 4
                n_usv = _capi.query_workspace(_capi.WS_HEAD_USV, B, max_n) // 4
                f_dev = torch.empty(n_f, **f32)
                usv_dev = torch.empty(n_usv, **f32)
                fh, uh = VP(self._pinned("f", n_f).data_ptr()), VP(self._pinned("usv", n_usv).data_ptr())
            _capi.call("hps_head_pose_levels", P(embed), embed_dim, embed_dim // 2, _capi.iptr(p["level_joints"]),
                       VP(sizes.data_ptr()), len(p["levels"]), _capi.iptr(p["anc_ptr"]), _capi.iptr(p["anc_idx"]),
                       VP(p["w1t_ptrs"].data_ptr()), VP(p["b1_ptrs"].data_ptr()), VP(p["w2_ptrs"].data_ptr()),
                       VP(p["b2_ptrs"].data_ptr()), P(U_proper), P(S_proper), P(mode), delta, P(pose_F), P(pose_U), P(pose_S),
                       P(pose_V), P(f_dev), P(usv_dev), fh, uh, B, nj, _SVD_THREADS,
                       ((_capi.SVD_DEVICE_FMA if self._flavor() == _capi.SVD_ROUNDING_FMA else _capi.SVD_DEVICE) |
                        (_capi.HEAD_WIDE_WORKGROUPS if self.latency_mode else 0)) if device_svd else _capi.SVD_HOST, s)
            return pose_F, pose_U, pose_S, pose_V, mode, loc, scale, glob, cam
        for lvl in p["levels"]:
            n_level = lvl.numel()
            if device_svd:
                _capi.call("hps_head_joint_level_svd", P(embed), embed_dim, embed_dim // 2, _capi.iptr(lvl), n_level,
                           _capi.iptr(p["anc_ptr"]), _capi.iptr(p["anc_idx"]),
                           _capi._P(p["w1t_ptrs"].data_ptr()), _capi._P(p["b1_ptrs"].data_ptr()),
                           _capi._P(p["w2_ptrs"].data_ptr()), _capi._P(p["b2_ptrs"].data_ptr()),
                           P(U_proper), P(S_proper), P(mode), delta, P(pose_F), P(pose_U), P(pose_S), P(pose_V), B, nj,
                           self._flavor() | (_capi.HEAD_WIDE_WORKGROUPS if self.latency_mode else 0), s)
                continue
            f_level = torch.empty(B, n_level, 3, 3, **f32)
            _capi.call("hps_head_joint_level", P(embed), embed_dim, embed_dim // 2, _capi.iptr(lvl), n_level,
                       _capi.iptr(p["anc_ptr"]), _capi.iptr(p["anc_idx"]),
                       _capi._P(p["w1t_ptrs"].data_ptr()), _capi._P(p["b1_ptrs"].data_ptr()),
                       _capi._P(p["w2_ptrs"].data_ptr()), _capi._P(p["b2_ptrs"].data_ptr()),
                       P(U_proper), P(S_proper), P(mode), delta, P(pose_F), P(f_level), B, nj, s)
            # host LAPACK SVD of the level's B * n_level 3x3 matrices (:137), see module docstring.
            # Pinned staging buffers; the stream synchronisation also retires the previous level's upload.
            f_host = self._pinned("f", B * n_level * 9).view(B * n_level, 3, 3)
            f_host.copy_(f_level.view(B * n_level, 3, 3), non_blocking=True)
            stream.synchronize()
            usv_host = self._pinned("usv", B * n_level * 21).view(B * n_level, 21)
            _host_svd_packed(f_host, usv_host)
            usv = torch.empty(B, n_level, 21, **f32)
            usv.view(B * n_level, 21).copy_(usv_host, non_blocking=True)
            _capi.call("hps_head_svd_finish", P(usv), _capi.iptr(lvl), n_level, P(pose_U), P(pose_S), P(pose_V),
                       P(U_proper), P(S_proper), P(mode), B, nj, s)
        return pose_F, pose_U, pose_S, pose_V, mode, loc, scale, glob, cam
