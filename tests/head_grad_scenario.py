"""Seeded cases and reference gradients of the head backward tests (tests/test_head_backward_host.py, tests/test_gpu_head_backward.py).

A plain float64 run of the head is NOT a valid reference for its gradient: LAPACK's sgesdd and dgesdd choose the signs of the singular
vectors independently, the signs enter the child joints' MLP inputs through U_proper (models/poseMF_shapeGaussian_net.py:126-130), and
so the fp32 and the float64 head are different functions.  The reference here restates the head with torch operations in a given
dtype and, after every torch.svd, multiplies column k of U and V by sign<U[:, k], U_pin[:, k]>, where U_pin is the pose_U of the run
under test (the device's; on the CPU the fp32 restatement's own).  A pinned sign is a constant factor of +-1, it changes no
derivative: the pinned float64 autograd is the truth for the function the device evaluates.  det U and det V enter as +-1 constants
(:139-140).

Weights: the package's net under torch.manual_seed(0) with default initialisation on the kinematic tree of
smpl_data.synthetic_smpl_model(0); recipe "default" as is (F near I, every matrix proper, small gaps), recipe "spread" with every
fc_pose[j][2] weight and bias multiplied by 4 (singular values 0.05-4, about one matrix in eight improper).
Features: 4 B + 8 candidate rows torch.rand(., 512) from a seeded generator; the first B rows whose float64 forward has
min(s1^2 - s2^2, s2^2 - s3^2, s3) >= 0.02 for all 23 joints are used (torch.svd's backward divides by these gaps); at least a
quarter of the candidates must pass, so the filter cannot hide a failure.
The accuracy rule is smpl_grad_scenario.bound / check.  References are computed once per case and shared (callers must not modify
them).
``head`` also takes another kinematic tree and a HeadOps (the steps tests/head_forward_scenario.py evaluates in other summation
orders, or deliberately wrong); the gradient tests pass neither.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from hierarchicalprobabilistic3dhuman_amd import configs, smpl_data
from hierarchicalprobabilistic3dhuman_amd.poseMF_shapeGaussian_net import PoseMFShapeGaussianNet, immediate_parents_to_all_parents
from smpl_grad_scenario import bound, check  # noqa: F401  (the accuracy rule, imported and not copied)

OUTPUTS = ("pose_F", "pose_S", "mode", "loc", "scale", "glob", "cam")          # the seven differentiable outputs
MIN_GAP = 0.02
FEATURE_SEED = 5
HEAD_PREFIXES = ("fc1.", "fc_shape.", "fc_glob.", "fc_cam.", "fc_embed.", "fc_pose.")


@functools.lru_cache(maxsize=None)
def parents():
    kt = np.asarray(smpl_data.synthetic_smpl_model(0)["kintree_table"])[0].astype(np.int64)
    return tuple([-1] + [int(p) for p in kt[1:]])


def make_net(recipe, tree=None, config=None):
    """A fresh net of the recipe (CPU, eval mode); tree: immediate parents (default parents()), config: default get_cfg_defaults()."""
    assert recipe in ("default", "spread")
    torch.manual_seed(0)
    net = PoseMFShapeGaussianNet(list(parents() if tree is None else tree), configs.get_cfg_defaults() if config is None else config).eval()
    if recipe == "spread":
        with torch.no_grad():
            for m in net.fc_pose:
                m[2].weight.mul_(4.0)
                m[2].bias.mul_(4.0)
    return net


@functools.lru_cache(maxsize=None)
def state(recipe):
    """fp32 state dict of the recipe's head (parameters and the init_glob / init_cam buffers)."""
    sd = make_net(recipe).state_dict()
    return {k: v.clone() for k, v in sd.items() if k.startswith(HEAD_PREFIXES) or k in ("init_glob", "init_cam")}


def param_names(sd):
    return [k for k in sd if k.startswith(HEAD_PREFIXES)]


class HeadOps:
    """The steps of ``head`` that tests/head_forward_scenario.py evaluates in other (legitimate or deliberately wrong) ways.  The
    defaults are the head as the reference states it; the backward tests never pass another."""

    def linear(self, x, w, b, name, addend=None):
        """Layer ``name`` ("fc1", "fc_shape", "fc_glob", "fc_cam", "fc_embed", "fc_pose.<j>.0", "fc_pose.<j>.2"); addend: init_glob /
        init_cam."""
        y = F.linear(x, w, b)
        return y if addend is None else y + addend

    def scale(self, log_std):
        return torch.exp(log_std)

    def ancestors(self, a):
        """The order in which a joint's ancestors enter its input (nearest first, the root excluded)."""
        return a

    def child_input(self, embed, up, sp, mode):
        """(B, .) blocks: the embedding and the ancestors' U_proper (9 each), S_proper (3 each), mode (9 each)."""
        return torch.cat([embed, up, sp, mode], dim=1)

    def svd(self, Fj):
        """(U, S, V) of the (B, 3, 3) matrices, singular values descending, any column signs."""
        return torch.svd(Fj)

    def pin_sign(self, dots, joint):
        """Column signs from dots = <U[:, k], U_pin[:, k]> (B, 3)."""
        assert float(dots.abs().min()) >= 0.99, ("singular vectors of joint %d do not match the pinned run" % joint, float(dots.abs().min()))
        return torch.sign(dots)

    def proper(self, U, S, V, dU, dV):
        """(U_proper, S_proper, mode) from the raw factors and the constants det U, det V = +-1 (B,)."""
        one = torch.ones_like(dU)
        Up = U * torch.stack([one, one, dU], dim=1)[:, None, :]
        Vp = V * torch.stack([one, one, dV], dim=1)[:, None, :]
        Sp = S * torch.stack([one, one, dU * dV], dim=1)
        return Up, Sp, torch.matmul(Up, Vp.transpose(-1, -2))


def head(sd, feats, pin_U=None, num_betas=10, delta_i_weight=None, tree=None, ops=None):
    """models/poseMF_shapeGaussian_net.py:95-162 restated in the dtype of ``sd`` / ``feats``; pin_U (B,NJ,3,3): the factors whose
    column signs the SVDs are pinned to; tree: immediate parents (default parents(), 23 body joints); ops: a HeadOps.  Returns a
    dict: the OUTPUTS plus pose_U, pose_V and the intermediate x, sgc = [shape_params | glob | cam], embed, u_proper, s_proper."""
    if delta_i_weight is None:
        cfg = configs.get_cfg_defaults()
        delta_i_weight = float(cfg.MODEL.DELTA_I_WEIGHT) if cfg.MODEL.DELTA_I else 0.0
    ops = HeadOps() if ops is None else ops
    anc = immediate_parents_to_all_parents(list(parents() if tree is None else tree))
    B, nj = feats.shape[0], len(anc)
    x = F.elu(ops.linear(feats, sd["fc1.weight"], sd["fc1.bias"], "fc1"))
    shape_params = ops.linear(x, sd["fc_shape.weight"], sd["fc_shape.bias"], "fc_shape")
    loc, scale = shape_params[:, :num_betas], ops.scale(shape_params[:, num_betas:])
    glob = ops.linear(x, sd["fc_glob.weight"], sd["fc_glob.bias"], "fc_glob", sd["init_glob"])
    cam = ops.linear(x, sd["fc_cam.weight"], sd["fc_cam.bias"], "fc_cam", sd["init_cam"])
    sgc = torch.cat([shape_params, glob, cam], dim=1)
    embed = F.elu(ops.linear(torch.cat([feats, sgc], dim=1), sd["fc_embed.weight"], sd["fc_embed.bias"], "fc_embed"))
    eye = torch.eye(3, dtype=feats.dtype)
    Fs, Us, Ss, Vs, Ups, Sps, modes = [], [], [], [], [], [], []
    for j in range(nj):
        a = ops.ancestors(anc[j])
        inp = embed
        if a:
            inp = ops.child_input(embed, *[torch.stack([t[i] for i in a], dim=1).reshape(B, -1) for t in (Ups, Sps, modes)])
        h = F.elu(ops.linear(inp, sd["fc_pose.%d.0.weight" % j], sd["fc_pose.%d.0.bias" % j], "fc_pose.%d.0" % j))
        Fj = ops.linear(h, sd["fc_pose.%d.2.weight" % j], sd["fc_pose.%d.2.bias" % j], "fc_pose.%d.2" % j).view(-1, 3, 3) + delta_i_weight * eye
        U, S, V = ops.svd(Fj)
        if pin_U is not None:
            dots = (U.detach() * pin_U[:, j].to(U.dtype)).sum(dim=1)                  # <U[:, k], U_pin[:, k]> per column
            sign = ops.pin_sign(dots, j)[:, None, :]
            U, V = U * sign, V * sign
        one = torch.ones(B, dtype=feats.dtype)
        dU = torch.where(torch.det(U.detach()) < 0, -one, one)
        dV = torch.where(torch.det(V.detach()) < 0, -one, one)
        Up, Sp, mode = ops.proper(U, S, V, dU, dV)
        Fs.append(Fj); Us.append(U); Ss.append(S); Vs.append(V); Ups.append(Up); Sps.append(Sp)
        modes.append(mode)
    st = lambda ts: torch.stack(ts, dim=1)
    return dict(pose_F=st(Fs), pose_U=st(Us), pose_S=st(Ss), pose_V=st(Vs), mode=st(modes), loc=loc, scale=scale, glob=glob, cam=cam,
                x=x, sgc=sgc, embed=embed, u_proper=st(Ups), s_proper=st(Sps))


def min_gap(pose_S):
    """min over the joints of min(s1^2 - s2^2, s2^2 - s3^2, s3), per image."""
    s2 = pose_S.double() ** 2
    g = torch.minimum(torch.minimum(s2[..., 0] - s2[..., 1], s2[..., 1] - s2[..., 2]), pose_S.double()[..., 2])
    return g.min(dim=1).values


def improper_share(out):
    """Share of the (image, joint) matrices with det U det V = -1."""
    d = torch.det(out["pose_U"].double()) * torch.det(out["pose_V"].double())
    return float((d < 0).double().mean())


def select_features(sd, B, seed=FEATURE_SEED, **head_args):
    """The feature rule for the fp32 state ``sd`` (``head_args``: tree, num_betas of ``head``): (fp32 features (B, fc1's width), kept,
    candidates), the first B of 4 B + 8 candidate rows whose float64 forward passes the gap filter."""
    n = 4 * B + 8
    cand = torch.rand(n, sd["fc1.weight"].shape[1], generator=torch.Generator().manual_seed(seed))
    sd64 = {k: v.double() for k, v in sd.items()}
    with torch.no_grad():
        gaps = min_gap(head(sd64, cand.double(), **head_args)["pose_S"])
    keep = gaps >= MIN_GAP
    kept = int(keep.sum())
    assert 4 * kept >= n, "only %d of %d candidate rows pass the gap filter" % (kept, n)
    rows = cand[keep][:B].contiguous()
    assert rows.shape[0] == B and float(gaps[keep][:B].min()) >= MIN_GAP
    return rows, kept, n


@functools.lru_cache(maxsize=None)
def features(recipe, B, seed=FEATURE_SEED):
    """(fp32 features (B,512), kept, candidates): the first B candidate rows that pass the gap filter."""
    return select_features(state(recipe), B, seed)


@functools.lru_cache(maxsize=None)
def cotangents(B, seed=0):
    """Standard-normal cotangents on the seven differentiable outputs."""
    g = torch.Generator().manual_seed(77 + 13 * B + seed)
    shapes = dict(pose_F=(B, 23, 3, 3), pose_S=(B, 23, 3), mode=(B, 23, 3, 3), loc=(B, 10), scale=(B, 10), glob=(B, 6), cam=(B, 3))
    return {k: torch.randn(shapes[k], generator=g) for k in OUTPUTS}


def vjp(sd32, feats32, pin_U, cot, dtype):
    """Gradients (float64 tensors) of sum_k <cot[k], out[k]> by autograd through ``head`` in ``dtype``: dict over "feats" and the
    parameter names."""
    sd = {k: v.detach().to(dtype).clone() for k, v in sd32.items()}
    names = param_names(sd)
    for k in names:
        sd[k].requires_grad_(True)
    feats = feats32.detach().to(dtype).clone().requires_grad_(True)
    out = head(sd, feats, pin_U)
    loss = sum((cot[k].to(dtype) * out[k]).sum() for k in cot)
    leaves = [feats] + [sd[k] for k in names]
    grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    return {k: (torch.zeros_like(l) if g is None else g).double() for k, l, g in zip(["feats"] + names, leaves, grads)}


_REFERENCES = {}


def reference(key, sd32, feats32, pin_U, cot):
    """(g64, g32) for the case ``key`` (any hashable naming weights, features, pinned run and cotangents), computed once."""
    if key not in _REFERENCES:
        pin = pin_U.detach().cpu()
        cot = {k: v.detach().cpu() for k, v in cot.items()}
        _REFERENCES[key] = (vjp(sd32, feats32, pin, cot, torch.float64), vjp(sd32, feats32, pin, cot, torch.float32))
    return _REFERENCES[key]


def rot6d(x):
    """utils/rigid_transform_utils.py:80-94 restated, the cross product along dim 1 for every n."""
    x = x.view(-1, 3, 2)
    a1, a2 = x[:, :, 0], x[:, :, 1]
    b1 = F.normalize(a1, dim=1)
    b2 = F.normalize(a2 - torch.einsum("bi,bi->b", b1, a2).unsqueeze(-1) * b1, dim=1)
    b3 = torch.cross(b1, b2, dim=1)
    return torch.stack((b1, b2, b3), dim=-1)


@functools.lru_cache(maxsize=None)
def rot6d_case(n):
    g = torch.Generator().manual_seed(300 + n)
    return torch.randn(n, 6, generator=g), torch.randn(n, 3, 3, generator=g)


@functools.lru_cache(maxsize=None)
def rot6d_reference(n):
    x, cot = rot6d_case(n)
    out = []
    for dtype in (torch.float64, torch.float32):
        xx = x.to(dtype).clone().requires_grad_(True)
        (rot6d(xx) * cot.to(dtype)).sum().backward()
        out.append(xx.grad.double())
    return tuple(out)
