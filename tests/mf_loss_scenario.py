"""Seeded inputs of the matrix-Fisher loss fixtures (tests/golden/make_mf_loss_golden.py writes the reference's results for them to
tests/golden/mf_loss_vectors.npz; tests/test_gpu_mf_loss.py rebuilds them).  Only torch.rand draws from a seeded CPU generator and
elementwise + - * / sqrt are used, so every CPU rebuilds the same bits and the large inputs need not be committed.

Pose parameters follow what torch.svd hands the loss: U, V rotations -- V with its last column negated in about half the rows, so
that det(U V^T) = -1 there -- S sorted in decreasing order, F = U diag(S) V^T.
"""
from types import SimpleNamespace

import torch

J, NB, K2D, P3D = 23, 10, 17, 14
WEIGHT_NAMES = ("POSE", "SHAPE", "JOINTS2D", "GLOB_ROTMATS", "VERTS3D", "JOINTS3D")
STAGES = {"STAGE1": (1.005, (80.0, 50.0, 5000.0, 5000.0, 0.0, 0.0)),
          "STAGE2": (1.005, (10.0, 80.0, 30000.0, 5000.0, 5000.0, 5000.0))}
# prediction leaves that receive gradients, in the order of the fixture keys loss_<case>_g<name>
GRAD_NAMES = ("F", "S", "loc", "scale", "joints2D", "glob_rotmats", "verts", "joints3D")


def _onehot(k):
    return tuple(1.0 if i == k else 0.0 for i in range(6))


# case -> recipe; weights override the stage's; vis: "random" (75 % visible), "first_none" (item 0 without a visible joint), "none"
LOSS_CASES = {
    "s1_mean_ns1": dict(seed=100, B=2, Ns=1, V=40, stage="STAGE1", reduction="mean"),
    "s1_sum_ns9": dict(seed=101, B=3, Ns=9, V=40, stage="STAGE1", reduction="sum"),
    "s2_mean_ns9": dict(seed=102, B=4, Ns=9, V=40, stage="STAGE2", reduction="mean", vis="first_none"),
    "s2_sum_ns1": dict(seed=103, B=2, Ns=1, V=40, stage="STAGE2", reduction="sum"),
    **{"onehot%d" % k: dict(seed=110 + k, B=3, Ns=9, V=40, stage="STAGE2", reduction="mean", weights=_onehot(k)) for k in range(6)},
    "novis_mean": dict(seed=120, B=2, Ns=9, V=40, stage="STAGE1", reduction="mean", vis="none"),
    "novis_sum": dict(seed=121, B=2, Ns=9, V=40, stage="STAGE2", reduction="sum", vis="none"),
    "b72": dict(seed=130, B=72, Ns=9, V=6890, stage="STAGE2", reduction="mean"),
}
IMG_WH = 256


def loss_config(case):
    c = LOSS_CASES[case]
    overreg, weights = STAGES[c["stage"]]
    weights = c.get("weights", weights)
    return SimpleNamespace(REDUCTION=c["reduction"], MF_OVERREG=overreg,
                           WEIGHTS=SimpleNamespace(**dict(zip(WEIGHT_NAMES, weights))))


def rotmats(g, n):
    """(n, 3, 3) rotation matrices from uniform quaternions q: the quadratic form of q divided by |q|^2 (no square root -- torch's
    vectorised sqrt is not correctly rounded, and its bits differ between CPU instruction sets)."""
    q = torch.rand(n, 4, generator=g) * 2.0 - 1.0
    w, x, y, z = q.unbind(-1)
    n2 = w * w + x * x + y * y + z * z
    r = [w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y),
         2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x),
         2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]
    return (torch.stack(r, -1) / n2[:, None]).view(n, 3, 3)


def pose_params(g, n):
    """F, U, S, V of n rows as torch.svd returns them, plus target rotations R."""
    U = rotmats(g, n)
    V = rotmats(g, n)
    flip = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    V[:, :, 2] = V[:, :, 2] * flip[:, None]
    conc = torch.where(torch.rand(n, 1, generator=g) < 0.15, 40.0, 1.0)        # a few rows of high concentration (up to 2000)
    S = torch.sort(torch.rand(n, 3, generator=g) * 50.0, dim=1, descending=True).values * conc
    US = U * S[:, None, :]
    F = US[:, :, None, 0] * V[:, None, :, 0] + US[:, :, None, 1] * V[:, None, :, 1] + US[:, :, None, 2] * V[:, None, :, 2]
    return F, U, S, V, rotmats(g, n)


def loss_inputs(case):
    """(pred, target) dicts of fp32 CPU tensors for LOSS_CASES[case]; pred carries the Normal's loc / scale as 'shape_loc' /
    'shape_scale' (make_dicts builds the distribution)."""
    c = LOSS_CASES[case]
    B, Ns, V = c["B"], c["Ns"], c["V"]
    g = torch.Generator().manual_seed(c["seed"])
    F, U, S, Vm, R = pose_params(g, B * J)
    loc = torch.rand(B, NB, generator=g) * 2.0 - 1.0
    scale = torch.rand(B, NB, generator=g) * 0.9 + 0.1
    t_shape = torch.rand(B, NB, generator=g) * 4.0 - 2.0
    j2d = torch.rand(B, Ns, K2D, 2, generator=g) * 2.4 - 1.2
    t_j2d = torch.rand(B, K2D, 2, generator=g) * IMG_WH
    vis = torch.rand(B, K2D, generator=g) < 0.75
    if c.get("vis") == "first_none":
        vis[0] = False
    elif c.get("vis") == "none":
        vis[:] = False
    glob = torch.rand(B, 3, 3, generator=g) * 2.0 - 1.0
    t_glob = rotmats(g, B)
    verts = torch.rand(B, V, 3, generator=g) - 0.5
    t_verts = verts + (torch.rand(B, V, 3, generator=g) - 0.5) * 0.1
    j3d = torch.rand(B, P3D, 3, generator=g) - 0.5
    t_j3d = j3d + (torch.rand(B, P3D, 3, generator=g) - 0.5) * 0.1
    pred = dict(pose_params_F=F.view(B, J, 3, 3), pose_params_U=U.view(B, J, 3, 3), pose_params_S=S.view(B, J, 3),
                pose_params_V=Vm.view(B, J, 3, 3), shape_loc=loc, shape_scale=scale, joints2D=j2d, glob_rotmats=glob, verts=verts,
                joints3D=j3d)
    target = dict(pose_params_rotmats=R.view(B, J, 3, 3), shape_params=t_shape, joints2D=t_j2d, joints2D_vis=vis,
                  glob_rotmats=t_glob, verts=t_verts, joints3D=t_j3d)
    return pred, target


def make_dicts(pred, target, dtype=torch.float32, device="cpu"):
    """The loss's (target_dict, pred_dict) in `dtype` on `device`, and the prediction leaves (GRAD_NAMES order) requiring grad."""
    cast = lambda t: t.to(device=device, dtype=dtype) if t.dtype.is_floating_point else t.to(device)
    leaves = [cast(pred[k]).requires_grad_(True) for k in ("pose_params_F", "pose_params_S", "shape_loc", "shape_scale", "joints2D",
                                                           "glob_rotmats", "verts", "joints3D")]
    F, S, loc, scale, j2d, glob, verts, j3d = leaves
    pred_dict = dict(pose_params_F=F, pose_params_U=cast(pred["pose_params_U"]), pose_params_S=S,
                     pose_params_V=cast(pred["pose_params_V"]), shape_params=torch.distributions.Normal(loc, scale), joints2D=j2d,
                     glob_rotmats=glob, verts=verts, joints3D=j3d)
    target_dict = {k: cast(v) for k, v in target.items()}
    return target_dict, pred_dict, leaves
