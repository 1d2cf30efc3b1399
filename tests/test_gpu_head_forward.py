"""GPU: the distribution head's forward kernels (csrc/head.hip, hps_head_pose_levels of csrc/composite.hip) and the float64 forward of
the backward (hps_head_forward_refine, csrc/head_backward.hip) against the pinned float64 truth of head_forward_scenario, on four
kinematic trees and at widths the module cannot produce.  Rule per output tensor: max|dev - y64| <= 4 max(e_a, e_b, e_c[, e_d],
2^-23 max|y64|); for the float64 pass 8 * 2^-29 max(e_a, 2^-23 max|y64|).  Every test prints the measured ratios."""
import pytest
import torch

import head_forward_scenario as FS
from hierarchicalprobabilistic3dhuman_amd import _capi

pytestmark = pytest.mark.gpu

HPS_E_UNSUPPORTED = -2
SENTINEL = -777.25
_NETS = {}


def net_of(tree, recipe, num_betas, dev):
    """The case's net on the device, shared by the tests (they restore every switch they touch)."""
    key = (tree, recipe, num_betas)
    if key not in _NETS:
        _NETS[key] = FS.make_net(tree, recipe, num_betas).to(dev)
    return _NETS[key]


def forward(net, feats, **switches):
    """The net's nine outputs as a dict, with the given switches (latency=..., composite_head=..., svd_mode=...) for this call only."""
    latency = switches.pop("latency", False)
    old = {k: getattr(net, k) for k in switches}
    try:
        for k, v in switches.items():
            setattr(net, k, v)
        net.set_latency_mode(latency)
        with torch.no_grad():
            pose_F, pose_U, pose_S, pose_V, mode, shape_dist, glob, cam = net(None, input_feats=feats)
    finally:
        for k, v in old.items():
            setattr(net, k, v)
        net.set_latency_mode(False)
    return dict(pose_F=pose_F, pose_U=pose_U, pose_S=pose_S, pose_V=pose_V, mode=mode, loc=shape_dist.loc, scale=shape_dist.scale,
                glob=glob, cam=cam)


@pytest.mark.parametrize("tree,recipe,B,num_betas", FS.DEVICE_CASES)
def test_whole_head_against_the_pinned_float64_truth(dev, tree, recipe, B, num_betas):
    """The product path (composite, device SVD) and, where the tree has several levels, the per-level form, the host-SVD form and the
    latency form (wide workgroups), each against the truth pinned to its own pose_U; the forms the project declares bit-identical are
    compared bit for bit."""
    c = FS.case(tree, recipe, B, num_betas)
    net, feats = net_of(tree, recipe, num_betas, dev), c["feats"].to(dev)
    assert net.levels == FS.levels(tree) and net.num_shape_params == num_betas
    tag = "%s %s B=%d" % (tree, recipe, B)
    product = forward(net, feats)
    worst = FS.check(tag + " product", product, c)
    assert all(product[k].shape == v.shape for k, v in FS.reference(c, product["pose_U"])[0].items() if k in product)
    if len(net.levels) > 1:
        per_level = forward(net, feats, composite_head=False)
        host = forward(net, feats, svd_mode="host")
        latency = forward(net, feats, latency=True)
        for name, form in (("per-level", per_level), ("host SVD", host), ("latency", latency)):
            for k, v in FS.check("%s %s" % (tag, name), form, c).items():
                worst[k] = max(worst[k], v)
        for k in product:
            assert torch.equal(per_level[k], product[k]), ("composite against per-level", k)
            assert torch.equal(host[k], product[k]), ("host SVD against device SVD", k)
    print("%s worst over the forms in max(e_family, 2^-23 max|y64|): %s" % (tag, {k: round(v, 2) for k, v in worst.items()}))


def refine(net, feats, pose_U):
    """hps_head_forward_refine as the backward calls it: (float64 outputs under the scenario's names, the fp32 x, sgc, embed)."""
    p = net._prepared or net.prepare()
    B, dev = feats.shape[0], feats.device
    nj, embed_dim = net.num_joints, net.config.MODEL.EMBED_DIM
    nt = 2 * net.num_shape_params + net.num_glob_params + net.num_cam_params
    nf, hidden = feats.shape[1], p["fc1_wt"].shape[1]
    P, VP, D = _capi.ptr, _capi._P, lambda t: _capi.ptr(t, torch.float64)
    f32, f64 = dict(device=dev, dtype=torch.float32), dict(device=dev, dtype=torch.float64)
    delta = float(net.config.MODEL.DELTA_I_WEIGHT) if net.config.MODEL.DELTA_I else 0.0
    x_f, sgc_f, embed_f = torch.empty(B, hidden, **f32), torch.empty(B, nt, **f32), torch.empty(B, embed_dim, **f32)
    x_d, sgc_d, embed_d = torch.empty(B, hidden, **f64), torch.empty(B, nt, **f64), torch.empty(B, embed_dim, **f64)
    Up_d, Sp_d, mode_d = torch.empty(B, nj, 9, **f64), torch.empty(B, nj, 3, **f64), torch.empty(B, nj, 9, **f64)
    U_d, S_d, V_d = torch.empty(B, nj, 9, **f64), torch.empty(B, nj, 3, **f64), torch.empty(B, nj, 9, **f64)
    _capi.call("hps_head_forward_refine", P(feats), nf, P(p["fc1_wt"]), P(p["fc1_b"]), P(p["sgc_wt"]), P(p["sgc_b"]), P(p["sgc_add"]),
               P(p["embed_wt"]), P(p["embed_b"]), _capi.iptr(p["level_joints"]), VP(p["level_sizes_host"].data_ptr()),
               len(p["levels"]), _capi.iptr(p["anc_ptr"]), _capi.iptr(p["anc_idx"]), VP(p["w1t_ptrs"].data_ptr()),
               VP(p["b1_ptrs"].data_ptr()), VP(p["w2_ptrs"].data_ptr()), VP(p["b2_ptrs"].data_ptr()), delta, P(pose_U.contiguous()), P(x_f),
               P(sgc_f), P(embed_f), D(x_d), D(sgc_d), D(embed_d), D(Up_d), D(Sp_d), D(mode_d), D(U_d), D(S_d), D(V_d), B, nf, hidden,
               nt, embed_dim, embed_dim // 2, nj, _capi.stream())
    return (dict(x=x_d, sgc=sgc_d, embed=embed_d, u_proper=Up_d, s_proper=Sp_d, mode=mode_d, pose_U=U_d, pose_S=S_d, pose_V=V_d),
            dict(x=x_f, sgc=sgc_f, embed=embed_f))


@pytest.mark.parametrize("tree,recipe,B,num_betas", FS.DEVICE_CASES)
def test_forward_refine_against_the_pinned_float64_truth(dev, tree, recipe, B, num_betas):
    """The float64 forward every head gradient is evaluated at, pinned to the forward's pose_U: its nine float64 outputs by bound64 with
    the sequential chain in the yardstick (the kernel sums every layer as one chain; head_forward_scenario's docstring has the figures), its fp32 outputs equal to the rounded float64 ones bit for bit."""
    c = FS.case(tree, recipe, B, num_betas)
    net, feats = net_of(tree, recipe, num_betas, dev), c["feats"].to(dev)
    pose_U = forward(net, feats)["pose_U"]
    out_d, out_f = refine(net, feats, pose_U)
    res = FS.check("%s %s B=%d refine" % (tree, recipe, B), out_d, c, pose_U, rule64=True, chain=True)
    print("%s %s B=%d refine worst in 2^-29 max(e_a, e_d, 2^-23 max|y64|): %.2f" % (tree, recipe, B, max(res.values())))
    for k, v in out_f.items():
        assert torch.equal(v, out_d[k].float()), k


# K, N, B, act, addend, padded rows (ldx = K + 3, ldo = N + 2): every K, N, B, act of the issue at least once, K = 1792 (the largest
# the LDS tile takes) with the widest and the narrowest N, K < 16 (empty K slices) with every act
LINEAR_CASES = [(1, 1, 1, 0, False, True), (1, 17, 9, 1, True, True), (7, 15, 8, 1, True, True), (7, 16, 9, 2, False, False),
                (16, 16, 9, 2, False, True), (16, 1, 8, 0, True, True), (17, 17, 1, 0, True, True), (17, 29, 8, 2, True, False),
                (113, 29, 8, 1, False, True), (113, 15, 1, 2, True, True), (541, 29, 9, 0, True, True), (541, 16, 8, 1, False, True),
                (1792, 17, 9, 2, True, True), (1792, 1, 1, 1, False, True), (1792, 29, 8, 0, False, False)]


def _linear_buffers(lc, pad, dev):
    """x with NaN in the padding columns and in one guard row behind row B - 1; out with the sentinel in every element."""
    B, K, N = lc["B"], lc["K"], lc["N"]
    ldx, ldo = (K + 3, N + 2) if pad else (K, N)
    x = torch.full((B + 1, ldx), float("nan"))
    x[:B, :K] = lc["x"]
    out = torch.full((B + 1, ldo), SENTINEL, device=dev)
    return x.to(dev), out, ldx, ldo


@pytest.mark.parametrize("K,N,B,act,addend,pad", LINEAR_CASES)
def test_hps_linear_against_float64(dev, K, N, B, act, addend, pad):
    lc = FS.linear_case(K, N, B, act, addend)
    x, out, ldx, ldo = _linear_buffers(lc, pad, dev)
    P = _capi.ptr
    wt, bias, add = lc["wt"].to(dev), lc["bias"].to(dev), lc["addend"].to(dev) if addend else None
    _capi.call("hps_linear", P(x), ldx, P(wt), P(bias), P(add), P(out), ldo, B, K, N, act, _capi.stream())
    FS.check_linear("hps_linear K=%d N=%d B=%d act=%d addend=%d ldx=%d ldo=%d" % (K, N, B, act, addend, ldx, ldo), out[:B, :N], lc)
    if act:
        assert bool((lc["y64"] <= 0).any()) or K * N * B == 1             # the activation cuts
    # the NaN padding and guard row were not read (no NaN above), the padding columns and the guard row of out were not written
    assert torch.equal(out[:B, N:], torch.full((B, ldo - N), SENTINEL, device=dev))
    assert torch.equal(out[B], torch.full((ldo,), SENTINEL, device=dev))


def test_hps_linear_refuses_a_k_beyond_the_lds_tile(dev):
    K, N, B = 1793, 16, 2
    x, wt, bias = torch.randn(B, K, device=dev), torch.randn(K, N, device=dev), torch.randn(N, device=dev)
    out = torch.full((B, N), SENTINEL, device=dev)
    P = _capi.ptr
    rc = _capi.load().hps_linear(P(x), K, P(wt), P(bias), None, P(out), N, B, K, N, 0, _capi.stream())
    torch.cuda.synchronize()
    assert rc == HPS_E_UNSUPPORTED
    assert torch.equal(out, torch.full((B, N), SENTINEL, device=dev))
    # the largest K it takes is the one above: 1792 rows of 8 images beside the 16 x 8 x 16 partial sums are exactly 64 KiB


def kernel_weights(sd, nj, dev):
    """The state dict in the layout of the C ABI (PoseMFShapeGaussianNet.prepare): transposed trunk weights, the fused
    fc_shape | fc_glob | fc_cam layer with init_glob / init_cam as addend, pointer tables of the joint MLPs."""
    t = lambda w: w.t().contiguous().to(dev)
    c = lambda w: w.contiguous().to(dev)
    nsh2 = sd["fc_shape.weight"].shape[0]
    p = dict(fc1_wt=t(sd["fc1.weight"]), fc1_b=c(sd["fc1.bias"]),
             sgc_wt=t(torch.cat([sd["fc_shape.weight"], sd["fc_glob.weight"], sd["fc_cam.weight"]], dim=0)),
             sgc_b=c(torch.cat([sd["fc_shape.bias"], sd["fc_glob.bias"], sd["fc_cam.bias"]])),
             sgc_add=c(torch.cat([torch.zeros(nsh2), sd["init_glob"].reshape(-1), sd["init_cam"].reshape(-1)])),
             embed_wt=t(sd["fc_embed.weight"]), embed_b=c(sd["fc_embed.bias"]))
    w1t = [t(sd["fc_pose.%d.0.weight" % j]) for j in range(nj)]
    b1 = [c(sd["fc_pose.%d.0.bias" % j]) for j in range(nj)]
    w2 = [c(sd["fc_pose.%d.2.weight" % j]) for j in range(nj)]
    b2 = [c(sd["fc_pose.%d.2.bias" % j]) for j in range(nj)]
    ptrs = lambda ts: torch.tensor([x.data_ptr() for x in ts], dtype=torch.int64, device=dev)
    p.update(keep=(w1t, b1, w2, b2), w1t_ptrs=ptrs(w1t), b1_ptrs=ptrs(b1), w2_ptrs=ptrs(w2), b2_ptrs=ptrs(b2))
    return p


def run_trunk(c, p, widths, dev, pad=True):
    """hps_head_trunk on the case's features (ldf > num_feats: NaN padding columns and a NaN guard row): dict of its seven outputs."""
    nf, hidden, nsh, ng, nc, embed_dim, _ = widths
    B, nt = c["B"], 2 * nsh + ng + nc
    ldf = nf + 5 if pad else nf
    feats = torch.full((B + 1, ldf), float("nan"))
    feats[:B, :nf] = c["feats"]
    feats = feats.to(dev)
    E = lambda *shape: torch.full(shape, SENTINEL, device=dev)
    out = dict(x=E(B, hidden), sgc=E(B, nt), embed=E(B, embed_dim), loc=E(B, nsh), scale=E(B, nsh), glob=E(B, ng), cam=E(B, nc))
    P = _capi.ptr
    _capi.call("hps_head_trunk", P(feats), ldf, P(p["fc1_wt"]), P(p["fc1_b"]), P(p["sgc_wt"]), P(p["sgc_b"]), P(p["sgc_add"]),
               P(p["embed_wt"]), P(p["embed_b"]), P(out["x"]), P(out["sgc"]), P(out["embed"]), P(out["loc"]), P(out["scale"]),
               P(out["glob"]), P(out["cam"]), B, nf, hidden, nsh, ng, nc, embed_dim, _capi.stream())
    return out


@pytest.mark.parametrize("B", [1, 9])
@pytest.mark.parametrize("widths", [(40, 24, 1, 6, 3, 20, 128), (512, 512, 10, 6, 3, 256, 128)], ids=lambda w: "x".join(map(str, w[:6])))
def test_hps_head_trunk_at_other_widths(dev, widths, B):
    c = FS.case("single", "default", B, widths[2], widths)
    out = run_trunk(c, kernel_weights(c["sd"], 1, dev), widths, dev)
    pin = FS.run(c)["pose_U"]                                       # the trunk's outputs do not depend on the pinned factors
    FS.check("hps_head_trunk %s B=%d" % (widths[:6], B), out, c, pin)          # x, sgc, embed, loc, scale (against exp in float64), glob, cam
    nsh, ng = widths[2], widths[3]
    assert torch.equal(out["loc"], out["sgc"][:, :nsh])
    assert torch.equal(out["glob"], out["sgc"][:, 2 * nsh:2 * nsh + ng]) and torch.equal(out["cam"], out["sgc"][:, 2 * nsh + ng:])


LEVELS_CASE = ("mixed12", "spread", 5, 2, (24, 16, 2, 6, 3, 40, 128))
POSE_BUFFERS = (("pose_F", 9), ("pose_U", 9), ("pose_S", 3), ("pose_V", 9), ("u_proper", 9), ("s_proper", 3), ("mode", 9))


def run_levels(c, p, embed, form, dev):
    """The joint loop through the C ABI, one call per kinematic level, on sentinel-filled buffers.  form "device":
    hps_head_joint_level_svd; "host": hps_head_joint_level + hps_host_svd3_packed + hps_head_svd_finish; "host_flipped": as "host"
    with the first column of every U and V negated before the finish (a valid SVD with det U = -1, which LAPACK's own signs never
    give: the proper fix's flip of U's third column).  After every level the rows of all other joints must be what they were."""
    tree_name, B = c["tree_name"], c["B"]
    levels = FS.levels(tree_name)
    nj, embed_dim, hid = len(c["tree"]) - 1, embed.shape[1], 128
    from hierarchicalprobabilistic3dhuman_amd.poseMF_shapeGaussian_net import immediate_parents_to_all_parents
    anc = immediate_parents_to_all_parents(list(c["tree"]))
    anc_ptr, anc_idx = [0], []
    for j in range(nj):
        anc_idx.extend(anc[j])
        anc_ptr.append(len(anc_idx))
    anc_ptr = torch.tensor(anc_ptr, dtype=torch.int32, device=dev)
    anc_idx = torch.tensor(anc_idx if anc_idx else [0], dtype=torch.int32, device=dev)
    buf = {k: torch.full((B, nj, w), SENTINEL, device=dev) for k, w in POSE_BUFFERS}
    P, VP, I, s = _capi.ptr, _capi._P, _capi.iptr, _capi.stream()
    tables = (VP(p["w1t_ptrs"].data_ptr()), VP(p["b1_ptrs"].data_ptr()), VP(p["w2_ptrs"].data_ptr()), VP(p["b2_ptrs"].data_ptr()))
    for lvl in levels:
        ids, n = torch.tensor(lvl, dtype=torch.int32, device=dev), len(lvl)
        before = {k: v.clone() for k, v in buf.items()}
        if form == "device":
            _capi.call("hps_head_joint_level_svd", P(embed), embed_dim, hid, I(ids), n, I(anc_ptr), I(anc_idx), *tables, P(buf["u_proper"]),
                       P(buf["s_proper"]), P(buf["mode"]), 1.0, P(buf["pose_F"]), P(buf["pose_U"]), P(buf["pose_S"]), P(buf["pose_V"]), B, nj,
                       _capi.svd_flavor(), s)
        else:
            f_level = torch.full((B, n, 9), SENTINEL, device=dev)
            _capi.call("hps_head_joint_level", P(embed), embed_dim, hid, I(ids), n, I(anc_ptr), I(anc_idx), *tables, P(buf["u_proper"]),
                       P(buf["s_proper"]), P(buf["mode"]), 1.0, P(buf["pose_F"]), P(f_level), B, nj, s)
            assert torch.equal(f_level, buf["pose_F"][:, lvl])                  # the level's matrices, packed (image, slot)
            f_host = f_level.cpu().contiguous()
            usv_host = torch.empty(B * n, 21)
            _capi.call("hps_host_svd3_packed", VP(f_host.data_ptr()), VP(usv_host.data_ptr()), B * n, 2)
            if form == "host_flipped":
                usv_host[:, [0, 3, 6, 12, 15, 18]] *= -1.0
            usv = usv_host.to(dev)
            _capi.call("hps_head_svd_finish", P(usv), I(ids), n, P(buf["pose_U"]), P(buf["pose_S"]), P(buf["pose_V"]), P(buf["u_proper"]),
                       P(buf["s_proper"]), P(buf["mode"]), B, nj, s)
        others = [j for j in range(nj) if j not in lvl]
        for k in buf:
            assert torch.equal(buf[k][:, others], before[k][:, others]), (form, "level", lvl, k, "rows of other joints were written")
            assert not bool((buf[k][:, lvl] == SENTINEL).any()), (form, "level", lvl, k, "rows of the level were left out")
    return buf


def test_joint_levels_through_the_c_abi_at_embed_dim_40(dev):
    """Both level entry points on mixed12 with embed_dim = 40 (in_dim 40 ... 124, no multiple of the 8-wide unroll; B = 5 ends in a
    partial tile of one image whose gather is clamped to row B - 1), the embedding from hps_head_trunk at widths of its own."""
    tree_name, recipe, B, nsh, widths = LEVELS_CASE
    c = FS.case(*LEVELS_CASE)
    nj = len(c["tree"]) - 1
    p = kernel_weights(c["sd"], nj, dev)
    trunk = run_trunk(c, p, widths, dev)
    runs = {}
    for form in ("device", "host", "host_flipped"):
        buf = run_levels(c, p, trunk["embed"], form, dev)
        runs[form] = dict(trunk, **buf)
        FS.check("levels %s" % form, runs[form], c)
    for k, _ in POSE_BUFFERS:
        assert torch.equal(runs["host"][k], runs["device"][k]), ("host SVD against device SVD", k)
    flipped = runs["host_flipped"]
    assert bool((torch.det(flipped["pose_U"].view(B, nj, 3, 3).double()) < 0).all())
    assert bool((torch.det(flipped["u_proper"].view(B, nj, 3, 3).double()) > 0).all())
    assert bool((torch.det(flipped["mode"].view(B, nj, 3, 3).double()) > 0).all())


def test_joint_levels_refuse_a_tree_beyond_the_lds_tile(dev):
    """num_body_joints = 200: the largest MLP input (40 + 21 x 200 values for 4 images) does not fit the LDS; refused before any launch."""
    c = FS.case(*LEVELS_CASE)
    nj, B = len(c["tree"]) - 1, c["B"]
    p = kernel_weights(c["sd"], nj, dev)
    embed = torch.randn(B, 40, device=dev)
    ids = torch.tensor(FS.levels("mixed12")[0], dtype=torch.int32, device=dev)
    anc_ptr, anc_idx = torch.zeros(nj + 1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    buf = {k: torch.full((B, 200, w), SENTINEL, device=dev) for k, w in POSE_BUFFERS}     # sized for the joint count that is passed
    f_level = torch.full((B, len(ids), 9), SENTINEL, device=dev)
    P, VP, I, s = _capi.ptr, _capi._P, _capi.iptr, _capi.stream()
    tables = (VP(p["w1t_ptrs"].data_ptr()), VP(p["b1_ptrs"].data_ptr()), VP(p["w2_ptrs"].data_ptr()), VP(p["b2_ptrs"].data_ptr()))
    lib = _capi.load()
    rc = lib.hps_head_joint_level_svd(P(embed), 40, 128, I(ids), len(ids), I(anc_ptr), I(anc_idx), *tables, P(buf["u_proper"]), P(buf["s_proper"]),
                                      P(buf["mode"]), 1.0, P(buf["pose_F"]), P(buf["pose_U"]), P(buf["pose_S"]), P(buf["pose_V"]), B, 200,
                                      _capi.svd_flavor(), s)
    assert rc == HPS_E_UNSUPPORTED
    rc = lib.hps_head_joint_level(P(embed), 40, 128, I(ids), len(ids), I(anc_ptr), I(anc_idx), *tables, P(buf["u_proper"]), P(buf["s_proper"]),
                                  P(buf["mode"]), 1.0, P(buf["pose_F"]), P(f_level), B, 200, s)
    assert rc == HPS_E_UNSUPPORTED
    torch.cuda.synchronize()
    for k, v in buf.items():
        assert bool((v == SENTINEL).all()), k
    assert bool((f_level == SENTINEL).all())
