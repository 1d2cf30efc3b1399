"""Seeded cases and reference gradients of the stage-2 tests (tests/test_stage2_host.py, tests/test_gpu_stage2.py): the reparameterised
matrix-Fisher sampler (utils/sampling_utils.py:21, 51-53, 103-141) restated with torch operations in a given dtype, on top of
head_grad_scenario (the head, its weights, the feature rule with the gap filter) and smpl_grad_scenario.bound / check.

Two forms of the same function of (pose_U, pose_S, pose_V):
  (a) ``sample_true``    eps and w are given; the accept mask is computed under no_grad, the first N accepted proposals are kept in
                         proposal order, then y = Gaussian_std * eps, q = y / ||y||, R = U_p quat_to_rotmat(q) V_p^T.
  (b) ``sample_pinned``  the accepted unit quaternions q are given as constants: eps_eff = q / Gaussian_std.detach(),
                         y = Gaussian_std * eps_eff, and the rest as in (a).
(b) is "the function the device evaluated", pinned on the device's own quaternions the way the head reference is pinned on the
device's pose_U: eps_eff is eps / ||y||, a constant multiple of the noise of the accepted proposal, and ||y|| cancels in q, so (b) has
the derivative of (a) (tests/test_stage2_host.py holds the two together to 1e-10).

Noise of a case: ``noise(B, N, seed)`` draws, from a generator seeded with ``seed``, per image and per joint randn(8 N, 4) and then
rand(8 N) -- the order of the reference's loop (:128-137, :51, :60) and so the very numbers pose_matrix_fisher_sampling_torch(...,
sample_on_cpu=True) uploads after torch.manual_seed(seed).  det U and det V enter as the values torch.det returns (:105), constants.
"""
import functools
import math

import torch

import head_grad_scenario as HS
from smpl_grad_scenario import EPS32, bound, check  # noqa: F401  (the accuracy rule, imported and not copied)

B_ACG = 1.5                 # the envelope's hyper-parameter b (:78)
OVERSAMPLING = 8            # :79
MIN_MARGIN = 1e-5           # |w - ratio| of every evaluated proposal: an fp32 accept test cannot decide otherwise
FP32_CAP = 256.0            # the fp32 restatement's own worst-tensor error in 2^-23 max|g| (the cap of the BatchNorm row)
# (recipe, B, N, noise seed, feature seed): the host-noise cases the GPU tests use; the conditions on them are asserted by
# tests/test_stage2_host.py.  The default recipe's singular values lie close together (gaps from 0.03): with the feature seed of the
# head tests the fp32 restatement's own error is 450-500 x 2^-23 max|g|, above the cap, so that case takes the rows of seed 7 (84-90).
CASES = (("spread", 3, 8, 11, HS.FEATURE_SEED), ("spread", 1, 70, 12, HS.FEATURE_SEED), ("default", 5, 3, 13, 7))


def m_star(b=B_ACG):
    return math.exp(-(4.0 - b) / 2.0) * (4.0 / b) ** 2         # :125


def quat_to_rotmat(q):
    """utils/rigid_transform_utils.py:113-133 for (..., 4) quaternions (w, x, y, z), its renormalisation included -> (..., 3, 3)."""
    q = q / q.norm(dim=-1, keepdim=True)
    w, x, y, z = q.unbind(-1)
    rows = [w * w + x * x - y * y - z * z, 2 * x * y - 2 * w * z, 2 * w * y + 2 * x * z,
            2 * w * z + 2 * x * y, w * w - x * x + y * y - z * z, 2 * y * z - 2 * w * x,
            2 * x * z - 2 * w * y, 2 * w * x + 2 * y * z, w * w - x * x - y * y + z * z]
    return torch.stack(rows, dim=-1).reshape(q.shape[:-1] + (3, 3))


def proper(U, S, V):
    """:103-111: (U_p, S_p, V_p); det U, det V are constants."""
    dU, dV = torch.det(U.detach()), torch.det(V.detach())
    one = torch.ones_like(dU)
    Up = U * torch.stack([one, one, dU], dim=-1)[..., None, :]
    Vp = V * torch.stack([one, one, dV], dim=-1)[..., None, :]
    Sp = S * torch.stack([one, one, dU * dV], dim=-1)
    return Up, Sp, Vp


def acg(Sp, b=B_ACG):
    """:118-124: (A, Omega, Gaussian_std), each (B, J, 4)."""
    A = 2.0 * torch.stack([torch.zeros_like(Sp[..., 0]), Sp[..., 1] + Sp[..., 2], Sp[..., 0] + Sp[..., 2], Sp[..., 0] + Sp[..., 1]], dim=-1)
    Omega = 1.0 + 2.0 * A / b
    return A, Omega, Omega ** (-0.5)


@functools.lru_cache(maxsize=None)
def noise(B, N, seed, nj=23):
    """(eps (B, nj, 8 N, 4), w (B, nj, 8 N)) fp32 in the reference's drawing order (module docstring)."""
    g = torch.Generator().manual_seed(seed)
    n_prop = N * OVERSAMPLING
    eps, w = torch.empty(B, nj, n_prop, 4), torch.empty(B, nj, n_prop)
    for i in range(B):
        for j in range(nj):
            eps[i, j] = torch.randn(n_prop, 4, generator=g)
            w[i, j] = torch.rand(n_prop, generator=g)
    return eps, w


def _rotations(Up, Vp, q):
    """:139-141 for q (B, N, J, 4)."""
    return torch.matmul(Up[:, None], torch.matmul(quat_to_rotmat(q), Vp[:, None].transpose(-1, -2)))


def sample_true(U, S, V, eps, w, N, b=B_ACG):
    """Form (a) in the dtype of U.  Returns R (B, N, J, 3, 3), q (B, N, J, 4) and a dict: ``keep`` (B, J, 8 N) the kept proposals,
    ``margin`` the least |w - ratio| over the evaluated proposals (those up to each call's N-th accept)."""
    dtype = U.dtype
    Up, Sp, Vp = proper(U, S, V)
    A, Omega, sd = acg(Sp, b)
    y = sd[:, :, None, :] * eps.to(dtype)                                              # :52
    x = y / y.norm(dim=-1, keepdim=True)                                               # :53
    with torch.no_grad():
        p_bing = torch.exp(-(x * x * A[:, :, None, :]).sum(-1))                        # :56
        p_acg = (x * x * Omega[:, :, None, :]).sum(-1) ** (-2)                         # :57
        ratio = p_bing / (m_star(b) * p_acg)
        acc = w.to(dtype) < ratio                                                      # :61
        count = acc.long().cumsum(-1)
        assert bool((count[..., -1] >= N).all()), "a call of this case has fewer than N accepted proposals"
        keep = acc & (count <= N)                                                      # :64-65
        evaluated = (count - acc.long()) < N
        margin = float((w.to(dtype) - ratio).abs()[evaluated].min())
        idx = keep.nonzero()[:, 2].view(U.shape[0], U.shape[1], N)
    q = torch.gather(x, 2, idx[..., None].expand(-1, -1, -1, 4)).transpose(1, 2)       # (B, N, J, 4)
    return _rotations(Up, Vp, q), q, dict(keep=keep, margin=margin)


def sample_pinned(U, S, V, q, b=B_ACG):
    """Form (b) in the dtype of U on the constant unit quaternions q (B, N, J, 4)."""
    Up, Sp, Vp = proper(U, S, V)
    sd = acg(Sp, b)[2][:, None]                                                        # (B, 1, J, 4)
    eps_eff = q.detach().to(device=U.device, dtype=U.dtype) / sd.detach()
    y = sd * eps_eff
    return _rotations(Up, Vp, y / y.norm(dim=-1, keepdim=True))


def factor_vjp(U32, S32, V32, q, g_R, dtype):
    """Gradients (float64) of <g_R, sample_pinned(U, S, V, q)> with respect to the leaves U, S, V in ``dtype``."""
    leaves = [t.detach().cpu().to(dtype).clone().requires_grad_(True) for t in (U32, S32, V32)]
    R = sample_pinned(*leaves, q.detach().cpu())
    grads = torch.autograd.grad((g_R.detach().cpu().to(dtype) * R).sum(), leaves)
    return {k: g.double() for k, g in zip(("pose_U", "pose_S", "pose_V"), grads)}


def head_vjp(sd32, feats32, pin_U, dtype, loss_fn):
    """Gradients (float64 tensors) of loss_fn(out) by autograd through HS.head in ``dtype``, signs pinned on pin_U: dict over "feats"
    and the parameter names.  loss_fn takes HS.head's output dict (tensors of ``dtype``) and returns a scalar."""
    sd = {k: v.detach().to(dtype).clone() for k, v in sd32.items()}
    names = HS.param_names(sd)
    for k in names:
        sd[k].requires_grad_(True)
    feats = feats32.detach().to(dtype).clone().requires_grad_(True)
    out = HS.head(sd, feats, None if pin_U is None else pin_U.detach().cpu())
    leaves = [feats] + [sd[k] for k in names]
    grads = torch.autograd.grad(loss_fn(out), leaves, allow_unused=True)
    return {k: (torch.zeros_like(l) if g is None else g).double() for k, l, g in zip(["feats"] + names, leaves, grads)}


def sampler_loss(form, g_R, N=None, eps=None, w=None, q=None, cot=None):
    """loss_fn for head_vjp: <g_R, R> with R by form "a" (eps, w, N) or "b" (q), plus <cot[k], out[k]> for the outputs in ``cot``."""
    def fn(out):
        dtype = out["pose_U"].dtype
        if form == "a":
            R = sample_true(out["pose_U"], out["pose_S"], out["pose_V"], eps, w, N)[0]
        else:
            R = sample_pinned(out["pose_U"], out["pose_S"], out["pose_V"], q)
        loss = (g_R.detach().cpu().to(dtype) * R).sum()
        for k, c in (cot or {}).items():
            loss = loss + (c.detach().cpu().to(dtype) * out[k]).sum()
        return loss
    return fn


@functools.lru_cache(maxsize=None)
def cot_R(B, N, seed=0, nj=23):
    return torch.randn(B, N, nj, 3, 3, generator=torch.Generator().manual_seed(900 + 31 * B + N + seed))


@functools.lru_cache(maxsize=None)
def cot_factors(B, seed=0):
    """Standard-normal cotangents on the raw factors pose_U / pose_V."""
    g = torch.Generator().manual_seed(500 + 17 * B + seed)
    return {"pose_U": torch.randn(B, 23, 3, 3, generator=g), "pose_V": torch.randn(B, 23, 3, 3, generator=g)}


@functools.lru_cache(maxsize=None)
def host_case(recipe, B, N, seed, feature_seed=HS.FEATURE_SEED):
    """What the host conditions and the forms test need of a case, computed once: the fp32 head run whose pose_U pins the signs, form
    (a) in float64 and float32 on the case's noise."""
    sd32, feats = HS.state(recipe), HS.features(recipe, B, feature_seed)[0]
    eps, w = noise(B, N, seed)
    with torch.no_grad():
        pin = HS.head(sd32, feats)["pose_U"]
        o64 = HS.head({k: v.double() for k, v in sd32.items()}, feats.double(), pin)
        o32 = HS.head(sd32, feats, pin)
        R64, q64, info64 = sample_true(o64["pose_U"], o64["pose_S"], o64["pose_V"], eps, w, N)
        R32, q32, info32 = sample_true(o32["pose_U"], o32["pose_S"], o32["pose_V"], eps, w, N)
    return dict(sd32=sd32, feats=feats, pin=pin, eps=eps, w=w, q64=q64, q32=q32, info64=info64, info32=info32)


def worst_ratio(g, g64):
    """max over the tensors of max|g - g64| / (2^-23 max|g64|) (tensors nothing reaches are skipped)."""
    worst = 0.0
    for k in g64:
        scale = float(g64[k].abs().max())
        if scale > 0.0:
            worst = max(worst, float((g[k] - g64[k]).abs().max()) / (EPS32 * scale))
    return worst
