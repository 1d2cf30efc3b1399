"""Seeded cases, float64 truth and the accuracy rules of the distribution head's forward tests
(tests/test_head_forward_scenario_host.py, tests/test_gpu_head_forward.py).  Nothing here touches a device.

The restatement is head_grad_scenario.head (imported, with its ``tree`` and ``ops`` arguments): the head in any dtype on any
kinematic tree, the SVD column signs pinned to the pose_U of the run under test, so that a float64 truth exists despite LAPACK's
free sign choice.

Trees (immediate parents, a parent before its child, index 0 the root):
    smpl     head_grad_scenario.parents(): 23 body joints, 8 levels
    chain7   one joint per level, up to 6 ancestors
    star6    one level of six joints without ancestors (anc_idx is the placeholder)
    mixed12  5 levels of 3, 3, 2, 2, 2 joints
    single   one body joint: carries the trunk-only cases at widths the module cannot produce
Weights: the package's net under torch.manual_seed(0) (head_grad_scenario.make_net), recipes "default" and "spread" (every
fc_pose[j][2] times 4: improper matrices, so the proper-SVD fix does work); ``widths`` = (num_feats, hidden, num_shape, num_glob,
num_cam, embed_dim, joint hidden) instead builds nn.Linear layers of those widths under a seeded generator.
Features: head_grad_scenario.select_features (4 B + 8 candidates, the first B whose float64 forward has
min(s1^2 - s2^2, s2^2 - s3^2, s3) >= 0.02 on every joint; at least a quarter must pass).

Truth: the float64 restatement pinned to pose_U of the run under test, its 3x3 SVDs evaluated in 40-digit arithmetic (mpmath, which
torch's sympy brings along) and rounded to float64.  LAPACK's dgesdd is not accurate enough to be the truth of the float64 rule: on
star6 / default / B = 5 its U lies 5.5e-14 from the 40-digit factors of the same matrices (gaps s1 - s2 of 0.01 amplify its backward
error), 8.1 units of that rule, where a one-sided Jacobi SVD in float64 lies 2.3e-15 from them.  The family of legitimate fp32 evaluations, pinned alike:
    a   torch fp32 on the CPU
    b   every linear layer summed in contiguous K slices in order (ceil(K / slices) columns each, csrc/head.hip's split): 16 slices
        in the trunk, 2 in the joint MLPs
    c   as b with 8 slices in the joint MLPs (the wide workgroups' order)
    d   ONE strictly sequential chain per sum, every product formed in float64 and the sum rounded to fp32 after each addition
        (conv_scenario's y_seq32): in the fp32 rule for hps_linear's single-layer cases only; for the whole head it is the yardstick of
        the float64 pass on the device, see below
Accuracy rule per output tensor (smpl_grad_scenario.bound, imported, widened over the family as conv_scenario does; 4 is the
project's margin for another summation order; nothing of the code under test enters):
    bound   = 4 max(e_a, e_b, e_c[, e_d], 2^-23 max|y64|)          e_m = max|y_m - y64|
Float64 rule (hps_head_forward_refine; same conditioning, the yardstick scaled by the ratio of the unit roundings, 8 instead of 4
because both sides carry float64 roundings):
    bound64 = 8 * 2^-29 * max(e_a, 2^-23 max|y64|)
The sliced float64 restatement is held to exactly that.  hps_head_forward_refine sums every layer as one strictly sequential chain
(512 and 541 terms in the trunk) that starts at bias + addend, so that each addition of the glob and cam columns rounds at the size of
init_glob / init_cam (1 and 0.9) -- a legitimate order that the yardstick e_a, torch's blocked sums with the bias last, does not
represent: its fused fc_shape | fc_glob | fc_cam outputs lie at 9.4 units of the e_a-only rule on star6 / default / B = 5 (2.7e-15,
12 float64 roundings of 1 after 512 additions) and at 4.4 to 5.4 elsewhere.  For that entry point the order joins the family as
member d of the whole head,
    bound64 = 8 * 2^-29 * max(e_a, e_d, 2^-23 max|y64|),
and the factor stays.
Outputs held: pose_F, pose_U, pose_S, pose_V, mode, loc, scale, glob, cam, and x, sgc = [shape_params | glob | cam], embed,
u_proper, s_proper where an entry point exposes them.

Measured, in units of max(e_family, 2^-23 max|y64|) for the fp32 rule (bound at 4) and of 2^-29 max(e_a[, e_d], 2^-23 max|y64|)
for the float64 rule (bound at 8); the tests print every figure.
  CPU, every tree and recipe at B = 9:
    members b and c in max(e_a, 2^-23 max|y64|), worst output per tree: smpl 1.49 (mode), chain7 3.47 (pose_V; pose_U 3.25, the
      other outputs <= 1.25), star6 1.25 (loc), mixed12 1.90 (pose_V); over all of them 0.38 to 3.47
    sliced float64 against the truth (e_a only): 1.17 to 2.51; with LAPACK's dgesdd as the truth's SVD instead: pose_U 8.69 on
      mixed12 / default
    every mutant on its named outputs: 4.5e3 to 7.6e6; where it cannot act (no ancestors, no improper matrix): <= 1.0
    kept candidate rows: 24 to 44 of 44; improper share under "spread": smpl 0.145, chain7 0.143, mixed12 0.120, star6 0
  MI355X, the device cases, worst over product / per-level / host-SVD / latency form:
    per tree: smpl 1.98 (mode), chain7 3.58 (mode, spread B = 1), star6 1.43 (mode), mixed12 2.00 (pose_U)
    per output: pose_F 1.79, pose_U 2.00, pose_S 1.50, pose_V 1.90, mode 3.58, loc 0.80, scale 0.87, glob 0.95, cam 1.02
    hps_head_forward_refine (a and d): smpl 1.62 (pose_S), chain7 2.85 (pose_U), star6 2.29 (pose_S), mixed12 1.59 (sgc);
      with e_a alone: sgc 9.4 on star6, 4.4 to 5.4 on smpl and chain7, the other outputs 0.5 to 4.0
    hps_linear 0.15 to 0.90; hps_head_trunk at other widths 0.11 to 0.93; joint levels at embed_dim 40: 0.24 to 1.22, with det U = -1
      forced through hps_head_svd_finish 0.40 to 1.46
"""
import functools
import hashlib

import torch
import torch.nn.functional as F

import head_grad_scenario as HS
from hierarchicalprobabilistic3dhuman_amd import configs
from hierarchicalprobabilistic3dhuman_amd.rigid_transform_utils import rotmat_to_rot6d
from smpl_grad_scenario import bound as _bound  # the accuracy rule, imported and not copied

EPS32 = 2.0 ** -23
TREES = {"smpl": None, "chain7": (-1, 0, 1, 2, 3, 4, 5, 6), "star6": (-1, 0, 0, 0, 0, 0, 0),
         "mixed12": (-1, 0, 0, 1, 1, 2, 3, 3, 5, 6, 8, 10, 10), "single": (-1, 0)}
DEEP_TREES = ("smpl", "chain7", "mixed12")
NET_OUTPUTS = ("pose_F", "pose_U", "pose_S", "pose_V", "mode", "loc", "scale", "glob", "cam")
ALL_OUTPUTS = NET_OUTPUTS + ("x", "sgc", "embed", "u_proper", "s_proper")
# (tree, recipe, B, NUM_SMPL_BETAS) of the whole-head and refine tests on the device: B crosses the tiles of 8 (trunk) and 4 (levels)
DEVICE_CASES = [("smpl", "spread", 9, 10), ("smpl", "default", 3, 10), ("chain7", "spread", 1, 10), ("star6", "default", 5, 10),
                ("mixed12", "spread", 4, 10), ("mixed12", "spread", 13, 10), ("chain7", "default", 2, 3)]
TRUNK_SLICES, JOINT_SLICES, WIDE_SLICES = 16, 2, 8          # csrc/head.hip: LKS, NT / HID of the product and of the wide form

def tree(name):
    return HS.parents() if name == "smpl" else TREES[name]


def levels(name):
    """The tree's body joints grouped by depth, as the module does."""
    from hierarchicalprobabilistic3dhuman_amd.poseMF_shapeGaussian_net import immediate_parents_to_all_parents
    anc = immediate_parents_to_all_parents(list(tree(name)))
    depth = [len(anc[j]) for j in range(len(anc))]
    return [[j for j in range(len(anc)) if depth[j] == d] for d in range(max(depth) + 1)]


def config(num_betas=10):
    cfg = configs.get_cfg_defaults()
    cfg.MODEL.NUM_SMPL_BETAS = num_betas
    return cfg


def make_net(tree_name, recipe, num_betas=10):
    """A fresh net of the package on the tree (CPU, eval mode)."""
    return HS.make_net(recipe, tree(tree_name), config(num_betas))


def _custom_state(tree_name, recipe, widths):
    nf, hidden, nsh, ng, nc, embed_dim, hid = widths
    assert ng == 6 and nc == 3, "init_glob / init_cam are the module's"
    from hierarchicalprobabilistic3dhuman_amd.poseMF_shapeGaussian_net import immediate_parents_to_all_parents
    anc = immediate_parents_to_all_parents(list(tree(tree_name)))
    sd = {}
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(1000 + sum(widths))

        def layer(name, k, n, gain=1.0):
            m = torch.nn.Linear(k, n)
            sd[name + ".weight"], sd[name + ".bias"] = m.weight.detach() * gain, m.bias.detach() * gain

        layer("fc1", nf, hidden)
        layer("fc_shape", hidden, 2 * nsh)
        layer("fc_glob", hidden, ng)
        layer("fc_cam", hidden, nc)
        layer("fc_embed", nf + 2 * nsh + ng + nc, embed_dim)
        for j in range(len(anc)):
            layer("fc_pose.%d.0" % j, embed_dim + 21 * len(anc[j]), hid)
            layer("fc_pose.%d.2" % j, hid, 9, 4.0 if recipe == "spread" else 1.0)
    sd["init_glob"] = rotmat_to_rot6d(torch.eye(3)[None, :].float())
    sd["init_cam"] = torch.tensor([0.9, 0.0, 0.0])
    return sd


@functools.lru_cache(maxsize=None)
def state(tree_name, recipe, num_betas=10, widths=None):
    """fp32 state dict of the head (callers must not modify it)."""
    assert recipe in ("default", "spread")
    if widths is not None:
        assert widths[2] == num_betas
        return _custom_state(tree_name, recipe, widths)
    sd = make_net(tree_name, recipe, num_betas).state_dict()
    return {k: v.clone() for k, v in sd.items() if k.startswith(HS.HEAD_PREFIXES) or k in ("init_glob", "init_cam")}


@functools.lru_cache(maxsize=None)
def case(tree_name, recipe, B, num_betas=10, widths=None):
    sd = state(tree_name, recipe, num_betas, widths)
    feats, kept, n = HS.select_features(sd, B, tree=tree(tree_name), num_betas=num_betas)
    return dict(key=(tree_name, recipe, B, num_betas, widths), sd=sd, tree=tree(tree_name), tree_name=tree_name, recipe=recipe,
                num_betas=num_betas, feats=feats, kept=kept, candidates=n, B=B)


def chain_linear(x, w, b, addend=None):
    """F.linear (+ addend) of fp32 operands as one strictly sequential chain over K that starts at bias + addend, the order of
    hps_head_forward_refine's sums: exact products, one rounding to fp32 per addition."""
    assert x.dtype == torch.float32
    xd, wd = x.double(), w.double().t().contiguous()
    acc = (b if addend is None else b + addend.reshape(-1)).double().expand(x.shape[0], -1)     # holds fp32 values
    for k in range(x.shape[1]):
        acc = (acc + xd[:, k:k + 1] * wd[k:k + 1]).float().double()
    return acc.float()


def sliced_linear(x, w, b, slices, drop=None):
    """F.linear with the K columns summed in ``slices`` contiguous slices of ceil(K / slices) in order, the bias last (the dtype's
    own arithmetic).  drop = q: slice q loses its last element (a mutant)."""
    K = x.shape[1]
    chunk = -(-K // slices)
    acc = torch.zeros(x.shape[0], w.shape[0], dtype=x.dtype)
    for q in range(slices):
        lo = min(K, q * chunk)
        hi = min(K, lo + chunk)
        if drop == q:
            assert hi > lo
            hi -= 1
        if hi > lo:
            acc = acc + x[:, lo:hi] @ w[:, lo:hi].t()
    return acc + b


# mutant -> (the outputs it must break the bound on, needs a tree with ancestors, needs improper matrices, needs two images)
MUTANTS = {
    "ancestors_farthest_first": (("pose_F",), True, False, False),
    "child_input_U_mode_S": (("pose_F",), True, False, False),
    "s_proper_without_sign": (("s_proper", "pose_F"), True, True, False),
    "u_proper_third_column_not_flipped": (("u_proper", "mode"), False, False, False),
    "mode_from_raw_U_Vt": (("mode",), True, True, False),
    "delta_i_weight_left_out": (("pose_F",), False, False, False),
    "init_glob_left_out": (("glob",), False, False, False),
    "init_cam_left_out": (("cam",), False, False, False),
    "scale_without_exp": (("scale",), False, False, False),
    "fc_embed_last_input_column_dropped": (("embed", "pose_F"), False, False, False),
    "trunk_slice_last_element_dropped": (("x", "loc"), False, False, False),
    "joint_slice_last_element_dropped": (("pose_F",), False, False, False),
    "last_image_given_its_neighbours_ancestors": (("pose_F",), True, False, True),
}


class Ops(HS.HeadOps):
    """trunk / joint: K slices of the linear layers (None: torch's own order, "chain": chain_linear); strict False: a run that need not line up with the pinned
    factors (the mutants); mutant: one of MUTANTS."""

    def __init__(self, trunk=None, joint=None, strict=True, mutant=None, exact_svd=False):
        assert mutant is None or mutant in MUTANTS
        self.trunk, self.joint, self.strict, self.mutant, self.exact_svd = trunk, joint, strict, mutant, exact_svd

    def svd(self, Fj):
        return exact_svd(Fj) if self.exact_svd else torch.svd(Fj)

    def linear(self, x, w, b, name, addend=None):
        slices = self.joint if name.startswith("fc_pose.") else self.trunk
        drop = None
        if self.mutant == "trunk_slice_last_element_dropped" and name == "fc1":
            slices, drop = slices or TRUNK_SLICES, 3
        if self.mutant == "joint_slice_last_element_dropped" and name.endswith(".0"):
            slices, drop = slices or JOINT_SLICES, 0
        if slices == "chain":
            return chain_linear(x, w, b, addend)
        y = F.linear(x, w, b) if slices is None else sliced_linear(x, w, b, slices, drop)
        return y if addend is None else y + addend

    def scale(self, log_std):
        return log_std if self.mutant == "scale_without_exp" else torch.exp(log_std)

    def ancestors(self, a):
        return a[::-1] if self.mutant == "ancestors_farthest_first" else a

    def child_input(self, embed, up, sp, mode):
        if self.mutant == "last_image_given_its_neighbours_ancestors":
            up, sp, mode = (torch.cat([t[:-1], t[-2:-1]], dim=0) for t in (up, sp, mode))
        if self.mutant == "child_input_U_mode_S":
            return torch.cat([embed, up, mode, sp], dim=1)
        return torch.cat([embed, up, sp, mode], dim=1)

    def pin_sign(self, dots, joint):
        if self.strict:
            return super().pin_sign(dots, joint)
        return torch.where(dots < 0, -torch.ones_like(dots), torch.ones_like(dots))

    def proper(self, U, S, V, dU, dV):
        Up, Sp, mode = super().proper(U, S, V, dU, dV)
        if self.mutant == "s_proper_without_sign":
            Sp = S
        if self.mutant == "u_proper_third_column_not_flipped":
            Up = U
            mode = torch.matmul(U, (V * torch.stack([torch.ones_like(dV), torch.ones_like(dV), dV], dim=1)[:, None, :]).transpose(-1, -2))
        if self.mutant == "mode_from_raw_U_Vt":
            mode = torch.matmul(U, V.transpose(-1, -2))
        return Up, Sp, mode


def exact_svd(Fj):
    """(U, S, V) of float64 (B, 3, 3) matrices: the SVD of the given entries in 40-digit arithmetic, rounded to float64."""
    import mpmath
    assert Fj.dtype == torch.float64
    U, S, V = torch.empty_like(Fj), torch.empty(Fj.shape[0], 3, dtype=torch.float64), torch.empty_like(Fj)
    with mpmath.workdps(40):
        for b, m in enumerate(Fj.tolist()):
            u, s, vt = mpmath.svd_r(mpmath.matrix(m))
            order = sorted(range(3), key=lambda k: -s[k])
            for k, o in enumerate(order):
                S[b, k] = float(s[o])
                for i in range(3):
                    U[b, i, k], V[b, i, k] = float(u[i, o]), float(vt[o, i])
    return U, S, V


def run(c, dtype=torch.float32, pin_U=None, ops=None):
    """The restatement on the case in ``dtype``."""
    sd = {k: v.to(dtype) for k, v in c["sd"].items()}
    with torch.no_grad():
        return HS.head(sd, c["feats"].to(dtype), pin_U, num_betas=c["num_betas"], tree=c["tree"], ops=ops)


def mutant_run(c, mutant):
    """The fp32 restatement with one mutation (its own signs).  LAPACK's gesdd returns det U = +1 on these matrices (two Householder
    reflections from the left), so the third column of U is never flipped with its signs: that mutant runs pinned to the
    restatement's own pose_U with the first column negated -- as valid a sign choice, with det U = -1 throughout."""
    sd = dict(c["sd"])
    delta = None
    if mutant == "u_proper_third_column_not_flipped":
        pin = run(c)["pose_U"].clone()
        pin[..., 0] = -pin[..., 0]
        out = run(c, torch.float32, pin, Ops(strict=False, mutant=mutant))
        assert bool((torch.det(out["pose_U"].double()) < 0)[:, levels(c["tree_name"])[0]].all())      # the joints without ancestors at least
        return out
    if mutant == "delta_i_weight_left_out":
        delta = 0.0
    if mutant in ("init_glob_left_out", "init_cam_left_out"):
        k = "init_glob" if "glob" in mutant else "init_cam"
        sd[k] = torch.zeros_like(sd[k])
    if mutant == "fc_embed_last_input_column_dropped":
        w = sd["fc_embed.weight"].clone()
        w[:, -1] = 0.0
        sd["fc_embed.weight"] = w
    with torch.no_grad():
        return HS.head(sd, c["feats"], None, num_betas=c["num_betas"], delta_i_weight=delta, tree=c["tree"], ops=Ops(mutant=mutant))


_REFERENCES = {}


def reference(c, pin_U, strict=True):
    """(y64, family): the float64 truth and the fp32 family {"a", "b", "c"} of the case, all pinned to ``pin_U`` (the pose_U of the run
    under test), computed once per (case, pinned factors) and shared: callers must not modify them."""
    pin = pin_U.detach().cpu().float().reshape(c["B"], -1, 3, 3).contiguous()
    key = (c["key"], strict, hashlib.sha1(pin.numpy().tobytes()).hexdigest())
    if key not in _REFERENCES:
        y64 = run(c, torch.float64, pin, Ops(strict=strict, exact_svd=strict))       # the mutants miss by factors of 10^3 and more
        fam = {"a": run(c, torch.float32, pin, Ops(strict=strict)),
               "b": run(c, torch.float32, pin, Ops(TRUNK_SLICES, JOINT_SLICES, strict)),
               "c": run(c, torch.float32, pin, Ops(TRUNK_SLICES, WIDE_SLICES, strict))}
        _REFERENCES[key] = (y64, fam)
    return _REFERENCES[key]


def member_d(c, pin_U):
    """Family member d of the whole head (every linear layer by chain_linear), pinned to ``pin_U``; computed once, kept with the
    reference."""
    fam = reference(c, pin_U)[1]
    if "d" not in fam:
        fam["d"] = run(c, torch.float32, pin_U.detach().cpu().float().reshape(c["B"], -1, 3, 3), Ops("chain", "chain"))
    return fam["d"]


def bound(y64, members):
    """The accuracy rule widened over the family: 4 max(e_m over the members, 2^-23 max|y64|)."""
    return max(_bound(y64, m.double()) for m in members)


def bound64(y64, members):
    """members: [y_a], for the device's float64 pass [y_a, y_d]."""
    return 8.0 * 2.0 ** -29 * bound(y64, members) / 4.0


def _check_one(tag, name, y, y64, members, labels, rule64=False):
    y = y.detach().cpu().double().reshape(y64.shape)
    err, scale = float((y - y64).abs().max()), float(y64.abs().max())
    errs = [float((m.double() - y64).abs().max()) for m in members]
    if rule64:
        unit, b = 2.0 ** -29 * max(errs + [EPS32 * scale]), bound64(y64, members)
    else:
        unit, b = max(errs + [EPS32 * scale]), bound(y64, members)
    print("%-40s %-9s max|run - f64| = %.3e  max|y64| = %.3e  %s  run / unit = %.2f (bound %d)"
          % (tag, name, err, scale, "  ".join("e_%s = %.3e" % (l, e) for l, e in zip(labels, errs)), err / unit, 8 if rule64 else 4))
    assert err == err and err <= b, (tag, name, err, b)
    return err / unit


def ratios(out, c, pin_U, names=None, rule64=False, strict=True):
    """err / unit per output of the run ``out`` (dict) against the truth pinned to ``pin_U``, without asserting."""
    y64, fam = reference(c, pin_U, strict)
    res = {}
    for name in (names or [k for k in ALL_OUTPUTS if k in out]):
        y = out[name].detach().cpu().double().reshape(y64[name].shape)
        err, scale = float((y - y64[name]).abs().max()), float(y64[name].abs().max())
        errs = [float((fam[m][name].double() - y64[name]).abs().max()) for m in ("a", "b", "c")]
        unit = 2.0 ** -29 * max(errs[0], EPS32 * scale) if rule64 else max(errs + [EPS32 * scale])
        res[name] = err / unit if err == err else float("inf")
    return res


def check(tag, out, c, pin_U=None, names=None, rule64=False, chain=False):
    """Prints the figures, then asserts the rule for every output of the run ``out`` (a dict; ``names``: these outputs only) against
    the truth pinned to ``pin_U`` (default: the run's own pose_U).  rule64: the float64 rule, with ``chain`` its yardstick holds member
    d beside a (module docstring).  Returns {output: err / unit}."""
    pin_U = out["pose_U"] if pin_U is None else pin_U
    y64, fam = reference(c, pin_U)
    labels = ("a", "b", "c") if not rule64 else ("a", "d") if chain else ("a",)
    if "d" in labels:
        member_d(c, pin_U)
    res = {}
    for name in (names or [k for k in ALL_OUTPUTS if k in out]):
        res[name] = _check_one(tag, name, out[name], y64[name], [fam[m][name] for m in labels], labels, rule64)
    print("%s worst: %s" % (tag, {k: round(v, 2) for k, v in res.items()}))
    return res


# ---- hps_linear's single-layer cases -----------------------------------------------------------------------------------------
ACT_NONE, ACT_ELU, ACT_RELU = 0, 1, 2


def activate(v, act):
    return F.elu(v) if act == ACT_ELU else F.relu(v) if act == ACT_RELU else v


@functools.lru_cache(maxsize=None)
def linear_case(K, N, B, act, addend):
    """Mixed-sign x (B, K), wt (K, N) as the kernel holds it, bias, addend or None; y64 and the family members a and d."""
    g = torch.Generator().manual_seed(9000 + 131 * K + 17 * N + 3 * B + act + 7 * int(addend))
    x, wt = torch.randn(B, K, generator=g), (torch.rand(K, N, generator=g) * 2 - 1) / K ** 0.5 * 2.0
    bias, add = torch.randn(N, generator=g) * 0.5, (torch.randn(N, generator=g) if addend else None)
    pre64 = x.double() @ wt.double() + bias.double() + (add.double() if addend else 0.0)
    y64 = activate(pre64, act)
    pre_a = F.linear(x, wt.t().contiguous(), bias)
    y_a = activate(pre_a + add if addend else pre_a, act)
    acc = torch.zeros(B, N, dtype=torch.float64)                                    # holds fp32 values
    xd, wd = x.double(), wt.double()
    for k in range(K):
        acc = (acc + xd[:, k:k + 1] * wd[k:k + 1]).float().double()                 # exact product, one rounding to fp32
    y_d = activate(acc.float() + (bias + add if addend else bias), act)
    return dict(x=x, wt=wt, bias=bias, addend=add, y64=y64, y_a=y_a, y_d=y_d, act=act, K=K, N=N, B=B)


def check_linear(tag, y, lc):
    return _check_one(tag, "y", y, lc["y64"], [lc["y_a"], lc["y_d"]], "ad")
