"""Device counterpart of the reference's losses/matrix_fisher_loss.py: ``LogMFNormConstant``, ``matrix_fisher_nll`` and
``PoseMFShapeGaussianLoss`` over libhps.so (include/hps.h: hps_mf_log_norm_const, hps_mf_nll, hps_mf_loss_forward / _backward).

Same names, arguments and results as the reference, with no host round trip and no boolean-mask gather: the loss is two launches
forward and one backward.  Inputs must be device tensors (CPU tensors raise ``HpsError``); the kernels read and write fp32 (other
float dtypes are converted, gradients come back in the input's dtype) and compute in fp64 inside.

One documented difference: targets are constants.  A target that requires grad raises ``ValueError`` instead of silently getting
no gradient.
"""
import ctypes

import torch
from torch import nn

from . import _capi

_REDUCTIONS = {"mean": _capi.MF_REDUCTION_MEAN, "sum": _capi.MF_REDUCTION_SUM}


def _constant(t, what):
    if isinstance(t, torch.Tensor) and t.requires_grad:
        raise ValueError("%s is a target and must not require grad (the device loss differentiates the predictions only)" % what)
    return t


def _f32(t, what):
    _capi.require_device(t, what)
    return _capi.f32c(t)


def _vis_bytes(vis, what):
    _capi.require_device(vis, what)
    if vis.dtype != torch.bool:
        vis = vis != 0
    return vis.contiguous().view(torch.uint8)


def _reduction(loss_config):
    red = loss_config.REDUCTION
    if red not in _REDUCTIONS:
        raise ValueError("%r is not a valid value for loss_config.REDUCTION ('mean' or 'sum')" % (red,))
    return _REDUCTIONS[red]


class LogMFNormConstant(torch.autograd.Function):
    """log c(S) = log c_bar(S) + tr(S) of the matrix-Fisher distribution (losses/matrix_fisher_loss.py:134-192): proper singular
    values (N, 3) -> (N,), with the reference's 512-node trapezoid rule; backward gives d log c / dS."""

    @staticmethod
    def forward(ctx, S):
        if S.dim() != 2 or S.shape[1] != 3:
            raise ValueError("S must be (N, 3), got %s" % (tuple(S.shape),))
        s = _f32(S, "S")
        log_c = torch.empty(s.shape[0], dtype=torch.float32, device=s.device)
        _capi.call("hps_mf_log_norm_const", _capi.ptr(s, what="S"), s.shape[0], _capi.ptr(log_c), None, None, _capi.stream())
        ctx.save_for_backward(s)
        ctx.in_dtype = S.dtype
        return log_c

    @staticmethod
    def backward(ctx, grad_log_c):
        s, = ctx.saved_tensors
        g = _capi.f32c(grad_log_c)
        grad_S = torch.empty_like(s)
        _capi.call("hps_mf_log_norm_const", _capi.ptr(s, what="S"), s.shape[0], None, _capi.ptr(g, what="grad_log_c"),
                   _capi.ptr(grad_S), _capi.stream())
        return grad_S.to(ctx.in_dtype)


class _MatrixFisherNLL(torch.autograd.Function):
    @staticmethod
    def forward(ctx, F, S, U, V, R, overreg):
        f, s, u, v, r = (_f32(t, w) for t, w in ((F, "pred_F"), (S, "pred_S"), (U, "pred_U"), (V, "pred_V"), (R, "target_R")))
        nll = torch.empty(f.shape[0], dtype=torch.float32, device=f.device)
        _capi.call("hps_mf_nll", _capi.ptr(f), _capi.ptr(u), _capi.ptr(s), _capi.ptr(v), _capi.ptr(r), f.shape[0], overreg,
                   _capi.ptr(nll), None, None, None, _capi.stream())
        ctx.save_for_backward(f, s, u, v, r)
        ctx.overreg, ctx.dtypes = overreg, (F.dtype, S.dtype)
        return nll

    @staticmethod
    def backward(ctx, grad_nll):
        f, s, u, v, r = ctx.saved_tensors
        need_F, need_S = ctx.needs_input_grad[:2]
        gF = torch.empty_like(f) if need_F else None
        gS = torch.empty_like(s) if need_S else None
        if need_F or need_S:
            g = _capi.f32c(grad_nll)
            _capi.call("hps_mf_nll", _capi.ptr(f), _capi.ptr(u), _capi.ptr(s), _capi.ptr(v), _capi.ptr(r), f.shape[0], ctx.overreg,
                       None, _capi.ptr(g, what="grad_nll"), _capi.ptr(gF), _capi.ptr(gS), _capi.stream())
        return (gF.to(ctx.dtypes[0]) if need_F else None, gS.to(ctx.dtypes[1]) if need_S else None, None, None, None, None)


def matrix_fisher_nll(pred_F, pred_U, pred_S, pred_V, target_R, overreg=1.025):
    """NLL of target_R under the matrix-Fisher distribution with parameter pred_F (losses/matrix_fisher_loss.py:195-228).
    pred_F, pred_U, pred_V, target_R (*, 3, 3), pred_S (*, 3); every leading dimension is flattened into rows -> (N,).
    s3 is multiplied by det(U V^T) (its value, as in the reference); U and V get no gradient."""
    _constant(target_R, "target_R")
    F, U, V, R = (t.reshape(-1, 3, 3) for t in (pred_F, pred_U, pred_V, target_R))
    S = pred_S.reshape(-1, 3)
    n = F.shape[0]
    if not (U.shape[0] == V.shape[0] == R.shape[0] == S.shape[0] == n):
        raise ValueError("matrix_fisher_nll: %d F rows, %d U, %d S, %d V, %d R" % (n, U.shape[0], S.shape[0], V.shape[0], R.shape[0]))
    return _MatrixFisherNLL.apply(F, S, U.detach(), V.detach(), R, float(overreg))


_PRED_KEYS = ("pose_params_F", "pose_params_S", "shape_loc", "shape_scale", "joints2D", "glob_rotmats", "verts", "joints3D")
_GRAD_FIELDS = ("g_pose_F", "g_pose_S", "g_shape_loc", "g_shape_scale", "g_joints2d", "g_glob_rotmats", "g_verts", "g_joints3d")


class _PoseMFShapeGaussianLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, F, S, loc, scale, j2d, glob, verts, j3d, consts, reduction, img_wh, overreg, weights):
        preds = [_f32(t, k) for t, k in zip((F, S, loc, scale, j2d, glob, verts, j3d), _PRED_KEYS)]
        U, V, tR, tS, tJ2, vis, tG, tV, tJ3 = consts
        f, s, loc32, scale32, j2, g3, v3, j3 = preds
        n_pose = f.numel() // 9
        if f.numel() != 9 * n_pose or s.numel() != 3 * n_pose or U.numel() != 9 * n_pose or V.numel() != 9 * n_pose or \
                tR.numel() != 9 * n_pose:
            raise ValueError("pose: F, U, V, target rotmats (N, 3, 3) and S (N, 3) must agree")
        if loc32.dim() != 2 or loc32.shape != scale32.shape or tuple(tS.shape) != tuple(loc32.shape):
            raise ValueError("shape_params: loc, scale and target must all be (B, num_betas)")
        if j2.dim() != 4 or j2.shape[-1] != 2 or tuple(tJ2.shape) != (j2.shape[0], j2.shape[2], 2) or \
                tuple(vis.shape) != (j2.shape[0], j2.shape[2]):
            raise ValueError("joints2D: predictions (B, Ns, K, 2), targets (B, K, 2), visibility (B, K)")
        for p, t, k in ((g3, tG, "glob_rotmats"), (v3, tV, "verts"), (j3, tJ3, "joints3D")):
            if tuple(p.shape) != tuple(t.shape):
                raise ValueError("%s: prediction %s and target %s differ in shape" % (k, tuple(p.shape), tuple(t.shape)))
        a = _capi.MfLossArgs()
        a.struct_bytes, a.reduction = ctypes.sizeof(_capi.MfLossArgs), reduction
        a.n_pose, a.shape_B, a.n_shape = n_pose, loc32.shape[0], loc32.numel()
        a.j2d_B, a.Ns, a.K = j2.shape[0], j2.shape[1], j2.shape[2]
        a.n_glob, a.n_verts, a.n_joints3d = g3.numel(), v3.numel(), j3.numel()
        a.img_wh, a.overreg = img_wh, overreg
        a.weights[:] = weights
        for name, t in zip(("pose_F", "pose_S", "shape_loc", "shape_scale", "joints2d", "glob_rotmats", "verts", "joints3d"), preds):
            setattr(a, name, t.data_ptr())
        for name, t in (("pose_U", U), ("pose_V", V), ("t_pose_rotmats", tR), ("t_shape", tS), ("t_joints2d", tJ2),
                        ("t_joints2d_vis", vis), ("t_glob_rotmats", tG), ("t_verts", tV), ("t_joints3d", tJ3)):
            setattr(a, name, t.data_ptr())
        ws = torch.empty(_capi.query_workspace(_capi.WS_MF_LOSS, n_pose), dtype=torch.uint8, device=f.device)
        total = torch.empty((), dtype=torch.float32, device=f.device)
        _capi.call("hps_mf_loss_forward", ctypes.addressof(a), _capi.ptr(ws, torch.uint8, "workspace"), _capi.ptr(total), _capi.stream())
        # the backward launch reads the fp32 operands, the per-row values the forward left in the workspace and its visible count
        ctx.args, ctx.ws, ctx.keep = a, ws, (preds, consts)
        ctx.in_meta = [(t.dtype, t.shape) for t in (F, S, loc, scale, j2d, glob, verts, j3d)]
        return total

    @staticmethod
    def backward(ctx, grad_total):
        a, preds = ctx.args, ctx.keep[0]
        grads = []
        for need, field, p in zip(ctx.needs_input_grad[:8], _GRAD_FIELDS, preds):
            g = torch.empty_like(p) if need else None
            setattr(a, field, g.data_ptr() if need else None)
            grads.append(g)
        g_total = _capi.f32c(grad_total)
        _capi.call("hps_mf_loss_backward", ctypes.addressof(a), _capi.ptr(ctx.ws, torch.uint8, "workspace"),
                   _capi.ptr(g_total, what="grad_output"), _capi.stream())
        out = [None if g is None else g.view(shape).to(dtype) for g, (dtype, shape) in zip(grads, ctx.in_meta)]
        return tuple(out) + (None,) * 5


class PoseMFShapeGaussianLoss(nn.Module):
    """NLL of the matrix-Fisher pose distribution + NLL of the Gaussian shape distribution + MSE of joints2D (visible joints) and
    global rotations + MSE of vertices and joints3D (losses/matrix_fisher_loss.py:231-301), one fused device pass.

    loss_config: REDUCTION ('mean' or 'sum'; anything else raises ValueError), MF_OVERREG and WEIGHTS.{POSE, SHAPE, JOINTS2D,
    GLOB_ROTMATS, VERTS3D, JOINTS3D} -- configs.get_cfg_defaults().LOSS.STAGE1 / STAGE2.  forward(target_dict, pred_dict) takes
    the reference's keys and returns the weighted total (a 0-dim fp32 tensor); pred_dict['shape_params'] is a
    torch.distributions.Normal whose loc and scale receive gradients."""

    def __init__(self, loss_config, img_wh):
        super(PoseMFShapeGaussianLoss, self).__init__()
        self.loss_config = loss_config
        self.img_wh = img_wh
        _reduction(loss_config)

    def forward(self, target_dict, pred_dict):
        cfg = self.loss_config
        reduction = _reduction(cfg)
        targets = [target_dict[k] for k in ("pose_params_rotmats", "shape_params", "joints2D", "joints2D_vis", "glob_rotmats", "verts",
                                            "joints3D")]
        for t, k in zip(targets, ("pose_params_rotmats", "shape_params", "joints2D", "joints2D_vis", "glob_rotmats", "verts", "joints3D")):
            _constant(t, "target_dict['%s']" % k)
        dist = pred_dict["shape_params"]
        preds = (pred_dict["pose_params_F"], pred_dict["pose_params_S"], dist.loc, dist.scale, pred_dict["joints2D"],
                 pred_dict["glob_rotmats"], pred_dict["verts"], pred_dict["joints3D"])
        tR, tS, tJ2, vis, tG, tV, tJ3 = targets
        consts = (_f32(pred_dict["pose_params_U"].detach(), "pose_params_U"), _f32(pred_dict["pose_params_V"].detach(), "pose_params_V"),
                  _f32(tR, "pose_params_rotmats"), _f32(tS, "shape_params"), _f32(tJ2, "joints2D"), _vis_bytes(vis, "joints2D_vis"),
                  _f32(tG, "glob_rotmats"), _f32(tV, "verts"), _f32(tJ3, "joints3D"))
        w = cfg.WEIGHTS
        weights = tuple(float(x) for x in (w.POSE, w.SHAPE, w.JOINTS2D, w.GLOB_ROTMATS, w.VERTS3D, w.JOINTS3D))
        return _PoseMFShapeGaussianLossFn.apply(*preds, consts, reduction, float(self.img_wh), float(cfg.MF_OVERREG), weights)
