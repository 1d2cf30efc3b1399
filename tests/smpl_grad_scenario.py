"""Seeded cases and reference gradients of the SMPL backward tests (tests/test_smpl_backward_host.py, tests/test_gpu_smpl_backward.py).

The truth is torch autograd through oracle.ref_cpu.smpl_forward on float64 SMPLParams; the same in float32 is "the reference's own
fp32".  The model is smpl_data.synthetic_smpl_model(0), as in conftest's smpl_assets.  The loss of a case is
sum(gV * vertices) + sum(gJ * joints) with standard-normal cotangents gV, gJ, so its gradients are the vector-Jacobian products the
device backward computes.  References are computed once per case and shared (callers must not modify them).
"""
import functools

import torch

from hierarchicalprobabilistic3dhuman_amd import configs, smpl_data
from oracle import ref_cpu as O

INPUTS = ("global_orient", "body_pose", "betas", "transl")
NB = 10
EPS32 = 2.0 ** -23


@functools.lru_cache(maxsize=None)
def model():
    return smpl_data.synthetic_smpl_model(0)


@functools.lru_cache(maxsize=None)
def params(dtype):
    return O.SMPLParams(model(), smpl_data.load_extra_joint_regressors(None), configs.SMPLX_EXTRA_VERTEX_IDS, dtype=dtype)


@functools.lru_cache(maxsize=None)
def case(M, pose2rot, transl, zero_row=None, betas_rows=None, seed=0):
    """fp32 CPU inputs and cotangents.  pose2rot: axis-angle (M, 3) / (M, 69), else rotation matrices (M, 1, 3, 3) / (M, 23, 3, 3).
    zero_row: that mesh's rotation vectors are all zero.  betas_rows: rows of betas (default M)."""
    g = torch.Generator().manual_seed(1000 + 7 * M + 2 * int(pose2rot) + int(transl) + 100 * seed)
    aa = torch.randn(M, 24, 3, generator=g, dtype=torch.float64) * 0.3
    if zero_row is not None:
        aa[zero_row] = 0.0
    if pose2rot:
        glob, body = aa[:, 0].reshape(M, 3), aa[:, 1:].reshape(M, 69)
    else:
        R = O.batch_rodrigues(aa.reshape(-1, 3)).view(M, 24, 3, 3)
        glob, body = R[:, :1], R[:, 1:]
    c = dict(global_orient=glob.float().contiguous(), body_pose=body.float().contiguous(),
             betas=torch.randn(M if betas_rows is None else betas_rows, NB, generator=g),
             transl=torch.randn(M, 3, generator=g) if transl else None,
             gV=torch.randn(M, 6890, 3, generator=g), gJ=torch.randn(M, 90, 3, generator=g), pose2rot=pose2rot, M=M)
    return c


def forward_loss(c, dtype, inputs, use_gV=True, use_gJ=True):
    """The case's loss in ``dtype`` for the given input dict (tensors of that dtype)."""
    out = O.smpl_forward(params(dtype), betas=inputs["betas"], body_pose=inputs["body_pose"], global_orient=inputs["global_orient"],
                         pose2rot=c["pose2rot"], transl=inputs.get("transl"))
    loss = 0.0
    if use_gV:
        loss = loss + (c["gV"].to(dtype) * out["vertices"]).sum()
    if use_gJ:
        loss = loss + (c["gJ"].to(dtype) * out["joints"]).sum()
    return loss


def leaves(c, dtype, device="cpu"):
    return {k: c[k].detach().clone().to(device=device, dtype=dtype).requires_grad_(True) for k in INPUTS if c[k] is not None}


def _grads(key, dtype, use_gV, use_gJ):
    c = case(*key)
    x = leaves(c, dtype)
    forward_loss(c, dtype, x, use_gV, use_gJ).backward()
    return {k: v.grad.double() for k, v in x.items()}


@functools.lru_cache(maxsize=None)
def reference(key, use_gV=True, use_gJ=True):
    """(g64, g32): gradients by the float64 oracle and by the same oracle in float32, dicts over the case's inputs (float64 tensors)."""
    return _grads(key, torch.float64, use_gV, use_gJ), _grads(key, torch.float32, use_gV, use_gJ)


def bound(g64, g32):
    """The accuracy rule: four times the reference's own fp32 error, or four fp32 roundings of the largest entry, whichever is larger
    (the factor 4 is the project's margin for a summation order other than the reference's, as in tests/test_gpu_philox.py)."""
    return 4.0 * max(float((g32 - g64).abs().max()), EPS32 * float(g64.abs().max()))


def check(name, g_dev, g64, g32):
    """Prints the figures, then asserts the accuracy rule for one gradient tensor."""
    err = float((g_dev.detach().cpu().double().reshape(g64.shape) - g64).abs().max())
    ref_err, scale = float((g32 - g64).abs().max()), float(g64.abs().max())
    print("%-14s max|dev - f64| = %.3e  max|cpu32 - f64| = %.3e  max|g64| = %.3e  dev/(2^-23 max|g64|) = %.2f  cpu32/(..) = %.2f"
          % (name, err, ref_err, scale, err / (EPS32 * scale), ref_err / (EPS32 * scale)))
    assert err <= bound(g64, g32), (name, err, bound(g64, g32))
    return err / (EPS32 * scale)
