"""GPU: the three SMPL backward entry points -- hps_smpl_lbs_backward, hps_smpl_blend_backward, hps_smpl_pose_prep_backward
(csrc/smpl_backward.hip) -- against the float64 definition of include/hps.h at vertex, joint, weight, mesh, regressor-row, blend-row and
blend-column counts and on kinematic trees other than SMPL's (tests/smpl_backward_scenario.py: cases, references, rule), through the C ABI;
and one chain hps_smpl_pose_prep -> hps_smpl_blend -> the three backward calls, as SMPL._backward strings them, on a 13-joint tree.

Every output is allocated with one guard mesh or row behind it and pre-filled with a sentinel, every workspace with guard floats behind
the queried size: after the call the guards and every element the ABI says is not written hold the sentinel exactly, and the live outputs
are finite.  Every call is made twice (same bits), and chosen meshes are run alone with M = 1 (same bits as in the batch).

The rule is mesh_scenario.check over the families of smpl_backward_scenario: err <= 4 * max(e_members..., 2^-23 max|y64|) per output tensor.
Worst err / (2^-23 max|y64|) measured on an MI355X per entry point and output tensor over the cases below, with the references' own ratios
and the bound of the case in which it occurred (measured values, not limits):

    hps_smpl_lbs_backward (11 cases + the large one)
        g_vposed   1.46   references 1.04 1.04, bound 4.17   (M = 17, V = 257, J = 22, K = 12, 66 regressor rows)
        g_a        4.98   references 4.50 5.33, bound 21.3   (the large case: 66 000 vertices in 516 chunks); the other cases 0.03 to 1.77
                          where their references have 0.03 to 2.30 -- most of it is the rounding of gV' = g_verts + C^T g_joints to fp32,
                          which every fp32 evaluation shares, so the kernel and both references often agree to two digits
        g_transl   1.99   references 0.80 0.53, bound 4.00   (M = 130, V = 385, J = 31: ONE ones row, chains of 128 terms); 0.29 to 1.06
                          in the other cases, 0.38 in the large one
    hps_smpl_blend_backward (9 cases)
        g_xt       6.95   references 3.72 3.72, bound 14.9   (kp = 208, np = 384, M = 127); 1.60 to 6.85 in the others, whose references have
                          0.44 to 4.15: the largest of kp x M sums of 123 to 1146 terms each, against the largest |sum|
    hps_smpl_pose_prep_backward (11 cases x {all cotangents, g_joints NULL, g_xt NULL}, and the zero-rotation meshes alone)
        g_glob     2.41   references 2.25, bound 8.99        (32-joint chain, M = 70); zero-rotation mesh alone 3.52 of 18.45 (the same chain)
        g_body     3.25   references 2.90, bound 11.6        (32-joint chain, M = 70, g_xt NULL); zero-rotation mesh alone 1.25 of 5.36
        g_betas    3.59   references 2.58, bound 10.3        (32-joint chain, M = 70, g_joints NULL); zero-rotation mesh alone 2.58 of 4.00
    the chain on the mixed tree
        hps_smpl_pose_prep  xt 0.24 (0.30, 4.00)   a 2.08 (2.48, 9.93)   j_posed 1.77 (2.05, 8.19)
        gradients           transl 0.27 (0.43, 4.00)   glob 1.06 (0.82, 4.00)   body 0.99 (1.26, 5.03)   betas 1.17 (1.07, 4.27)

Within half of their bound came: g_xt of hps_smpl_blend_backward at (kp, np, M) = (224, 512, 128) with 6.85 of 13.2, (304, 1152, 300) with 6.22
of 10.5 and (464, 1152, 129) with 5.37 of 10.6 -- one MFMA chain per 512-column slice is a longer fp32 chain than the blocked sums of the
references; and g_betas of hps_smpl_pose_prep_backward, which adds its 3 J joint terms one after another: 2.71 of 4.00 (SMPL tree, g_joints
NULL), 2.91 of 5.20 (star, one coefficient), 2.41 and 2.04 of 4.00 (mixed tree), and 2.58, 2.41 and 2.31 of 4.00 on the zero-rotation meshes
of the star, the mixed tree and the chain run alone.  Nothing failed, and no kernel was changed.
"""
import pytest
import torch

import smpl_backward_scenario as B
from hierarchicalprobabilistic3dhuman_amd import _capi

pytestmark = pytest.mark.gpu
SENT = -777.25
GUARD = 64
HPS_E_BADARG, HPS_E_UNSUPPORTED = -1, -2
P, IP = _capi.ptr, _capi.iptr


def _workspace(what, d0, d1, d2, dev):
    """A workspace of the queried size with GUARD sentinel floats behind it -> (buffer, live floats)."""
    nbytes = _capi.query_workspace(what, d0, d1, d2)
    assert nbytes > 0 and nbytes % 4 == 0
    return torch.full((nbytes // 4 + GUARD,), SENT, device=dev), nbytes // 4


def _untouched(t, what):
    assert bool((t == SENT).all()), what + ": written where the ABI writes nothing"


def _check(name, y_dev, y64, *family):
    if y64.numel():
        assert bool(torch.isfinite(y_dev).all()), name + ": not finite"
        B.check(name, y_dev, y64, *family)


def _on(dev, t):
    """The tensor on the device; an empty one becomes a one-element dummy (the entry points want non-null pointers)."""
    if t is None:
        return None
    if t.numel() == 0:
        return torch.zeros(1, dtype=t.dtype, device=dev)
    return t.to(dev).contiguous()


# ---------------------------------------------------------------------------------------------------------------------------------
# (a) hps_smpl_lbs_backward
# ---------------------------------------------------------------------------------------------------------------------------------
def _lbs_args(c, dev):
    ptr, row, val = c["csrt"]
    return dict(a=_on(dev, c["a"]), w_idx=_on(dev, c["w_idx"]), w_val=_on(dev, c["w_val"]), gv=_on(dev, c["g_verts"]), gj=_on(dev, c["g_joints"]),
                ptr=_on(dev, ptr), row=_on(dev, row), val=_on(dev, val))


def _lbs_buffers(c, dev):
    M, V, J, ld = c["M"], c["V"], c["J"], c["ld"]
    vp = torch.full((M + 1, ld), SENT, device=dev)
    vp[:M, :3 * V] = c["v_posed"].reshape(M, 3 * V).to(dev)
    return vp, torch.full((M + 1, J, 12), SENT, device=dev), torch.full((M + 1, 3), SENT, device=dev)


def _lbs(c, dev, o=None):
    """One call -> (g_vposed (M, V, 3), g_a (M, J, 12), g_transl (M, 3) or None), after the guard checks."""
    M, V, J, ld = c["M"], c["V"], c["J"], c["ld"]
    o = _lbs_args(c, dev) if o is None else o
    vp, g_a, g_tr = _lbs_buffers(c, dev)
    ws, n_ws = _workspace(_capi.WS_SMPL_LBS_BWD, M, V, J, dev)
    with_gj = o["gj"] is not None
    _capi.call("hps_smpl_lbs_backward", P(vp), ld, P(o["a"]), IP(o["w_idx"]), P(o["w_val"]), c["K"], J, P(o["gv"]), P(o["gj"]), c["n_rows"],
               IP(o["ptr"]) if with_gj else None, IP(o["row"]) if with_gj else None, P(o["val"]) if with_gj else None, P(g_a),
               P(g_tr) if c["want_transl"] else None, P(ws), M, V, _capi.stream())
    torch.cuda.synchronize()
    what = "hps_smpl_lbs_backward %s" % (c["key"],)
    _untouched(vp[M:], what + " v_posed behind M")
    _untouched(g_a[M:], what + " g_a behind M")
    _untouched(g_tr[M:] if c["want_transl"] else g_tr, what + " g_transl")
    _untouched(ws[n_ws:], what + " workspace")
    assert bool((vp[:M, 3 * V:] == 0).all()), what + ": the columns [3 V, ld) are not zero"
    assert bool(torch.isfinite(vp[:M]).all()) and bool(torch.isfinite(g_a[:M]).all())
    return vp[:M, :3 * V].reshape(M, V, 3).clone(), g_a[:M].clone(), g_tr[:M].clone() if c["want_transl"] else None


def _lbs_check(c, out):
    ref = B.lbs_reference(c)
    tag = "hps_smpl_lbs_backward %s " % (c["key"][:9],)
    for name, y in zip(("g_vposed", "g_a", "g_transl"), out):
        if y is not None:
            _check(tag + name, y, *ref[name])


def _same_bits(x, y, what):
    for name, p, q in zip(("g_vposed", "g_a", "g_transl"), x, y):
        assert (p is None and q is None) or torch.equal(p, q), "%s: %s differs" % (what, name)


def _lbs_case_test(key, dev, alone):
    c = B.lbs_case(*key)
    o = _lbs_args(c, dev)
    out = _lbs(c, dev, o)
    _lbs_check(c, out)
    _same_bits(out, _lbs(c, dev, o), "second run")
    for m in alone:                                                       # hps.h: "a mesh's result does not depend on M"
        one = _lbs(B.one_mesh(c, m), dev)
        _same_bits([None if y is None else y[m:m + 1] for y in out], one, "mesh %d alone" % m)


@pytest.mark.parametrize("key", B.LBS_CASES, ids=lambda k: "M%d-V%d-J%d-K%d-rows%d-gv%d-gj%d-tr%d-ld%s" % k)
def test_lbs_backward_at_other_shapes(key, dev):
    """(a) the rule for g_vposed (read from the in-place v_posed), g_a and g_transl; zero padding columns; guards; repeatable bits; mesh 0,
    the last mesh and one in the middle of a group alone give the bits they have in the batch."""
    M = key[0]
    _lbs_case_test(key, dev, sorted({0, M - 1, min(M - 1, 8 * ((M - 1) // 8) + 3), M // 2}))


def test_lbs_backward_with_two_mesh_groups_per_workgroup(dev):
    """(a) the large case: 516 chunks cap the grid at four workgroups per chunk over five mesh groups, so a workgroup walks two groups (the
    prefetch under the MFMA phase, the reuse of its LDS buffers and the barrier between them) and the last one holds a ragged group of
    five.  Mesh 8 is the first mesh of a workgroup's second group, mesh 35 lies in the ragged one."""
    assert B.lbs_launch_geometry(*B.LBS_LARGE_CASE[:2]) == (4, 2, 3)
    _lbs_case_test(B.LBS_LARGE_CASE, dev, (0, 8, 11, 35, 36))


def test_lbs_backward_refusals_leave_the_outputs_alone(dev):
    """num_joints = 32, K = 5 and n_rows = 97 are refused with real buffers, and nothing is written."""
    c = B.lbs_case(*B.LBS_CASES[3])
    M, V, J, ld = c["M"], c["V"], c["J"], c["ld"]
    o = _lbs_args(c, dev)
    lib = _capi.load()
    for K, joints, n_rows, code in ((c["K"], 32, c["n_rows"], None), (5, J, c["n_rows"], None),
                                    (c["K"], J, 97, HPS_E_UNSUPPORTED)):
        vp, g_a, g_tr = _lbs_buffers(c, dev)
        before = vp.clone()
        ws, _ = _workspace(_capi.WS_SMPL_LBS_BWD, M, V, J, dev)
        rc = lib.hps_smpl_lbs_backward(P(vp), ld, P(o["a"]), IP(o["w_idx"]), P(o["w_val"]), K, joints, P(o["gv"]), P(o["gj"]), n_rows, IP(o["ptr"]),
                                       IP(o["row"]), P(o["val"]), P(g_a), P(g_tr), P(ws), M, V, _capi.stream())
        torch.cuda.synchronize()
        assert rc in (HPS_E_BADARG, HPS_E_UNSUPPORTED) and (code is None or rc == code) and lib.hps_last_error(), (K, joints, n_rows, rc)
        assert torch.equal(vp, before)
        for t in (g_a, g_tr, ws):
            _untouched(t, "refused call")


# ---------------------------------------------------------------------------------------------------------------------------------
# (b) hps_smpl_blend_backward
# ---------------------------------------------------------------------------------------------------------------------------------
def _blend(bc, bmat, g, M, dev):
    """One call on the rows g (M, ld_g) -> g_xt (kp, mp), after the guard checks."""
    kp, np_ = bc["kp"], bc["np"]
    mp = _capi.query_workspace(_capi.WS_SMPL_MP, M)
    g_xt = torch.full((kp + 1, mp), SENT, device=dev)
    ws, n_ws = _workspace(_capi.WS_SMPL_BLEND_BWD, M, kp, np_, dev)
    _capi.call("hps_smpl_blend_backward", P(bmat), P(g), P(g_xt), P(ws), M, kp, mp, np_, bc["ld_g"], _capi.stream())
    torch.cuda.synchronize()
    what = "hps_smpl_blend_backward %s" % (bc["key"],)
    _untouched(g_xt[kp:], what + " behind kp")
    _untouched(ws[n_ws:], what + " workspace")
    assert bool(torch.isfinite(g_xt[:kp]).all()), what + ": not finite (the NaN columns [np, ld_g) reached the output?)"
    assert bool((g_xt[:kp, M:] == 0).all()), what + ": the columns [M, mp) are not zero"
    assert bool((g_xt[bc["rows"]:kp] == 0).all()), what + ": the rows behind the data rows are not zero"
    return g_xt[:kp].clone()


@pytest.mark.parametrize("key", B.BLEND_CASES, ids=lambda k: "kp%d-np%d-M%d-ld+%d" % k)
def test_blend_backward_at_other_shapes(key, dev):
    """(b) one partly filled, one exact and two row tiles; whole, partial and several slices; the rule; zero padding; repeatable bits; a
    column of the batch is the M = 1 call of that mesh; the NaN behind np never reaches the output."""
    bc = B.blend_case(*key)
    M = bc["M"]
    assert bc["ld_g"] == bc["np"] or bool(torch.isnan(bc["g_vposed"][:, bc["np"]:]).all())
    bmat, g = bc["bmat"].to(dev), bc["g_vposed"].to(dev)
    g_xt = _blend(bc, bmat, g, M, dev)
    _check("hps_smpl_blend_backward %s g_xt" % (key,), g_xt[:, :M], *B.blend_reference(bc))
    assert torch.equal(g_xt, _blend(bc, bmat, g, M, dev))
    for m in sorted({0, M - 1, M // 2}):
        one = _blend(bc, bmat, g[m:m + 1].contiguous(), 1, dev)
        assert torch.equal(one[:, 0], g_xt[:, m]), "mesh %d alone" % m


# ---------------------------------------------------------------------------------------------------------------------------------
# (c) hps_smpl_pose_prep_backward
# ---------------------------------------------------------------------------------------------------------------------------------
POSE_OUTPUTS = ("g_glob", "g_body", "g_betas")


def _pose_args(pc, dev):
    M, J = pc["M"], pc["J"]
    body = pc["body"] if J > 1 else torch.zeros(M, 9)                      # (a single joint: a non-null dummy, never read)
    return dict(glob=_on(dev, pc["glob"]), body=_on(dev, body), betas=_on(dev, pc["betas"]), jt=_on(dev, pc["j_template"]),
                js=_on(dev, pc["j_shapedirs"]), parents=torch.tensor(pc["parents"], dtype=torch.int32, device=dev),
                depth=torch.tensor(pc["depth"], dtype=torch.int32, device=dev), g_a=_on(dev, pc["g_a"]), gj=_on(dev, pc["g_joints"]),
                gxt=_on(dev, pc["g_xt"]))


def _pose_forward_args(pc, o):
    return (P(o["glob"]), P(o["body"]), int(pc["rotmat"]), P(o["betas"]), pc["nb"], P(o["jt"]), P(o["js"]), IP(o["parents"]), IP(o["depth"]),
            pc["J"])


def _pose(pc, o, dev, use_gj=True, use_gxt=True, want=POSE_OUTPUTS):
    """One call -> {g_glob, g_body, g_betas: (M, n) or None}, after the guard checks."""
    M, J, nb = pc["M"], pc["J"], pc["nb"]
    per = 9 if pc["rotmat"] else 3
    widths = dict(g_glob=per, g_body=per * (J - 1), g_betas=nb)
    bufs = {k: torch.full((M + 1, max(n, 1)), SENT, device=dev) for k, n in widths.items()}
    _capi.call("hps_smpl_pose_prep_backward", *_pose_forward_args(pc, o), P(o["g_a"]), P(o["gj"]) if use_gj else None, pc["n_rows"],
               P(o["gxt"]) if use_gxt else None, pc["mp"], *[P(bufs[k]) if k in want else None for k in POSE_OUTPUTS], M, _capi.stream())
    torch.cuda.synchronize()
    out = {}
    for k, n in widths.items():
        what = "hps_smpl_pose_prep_backward %s %s" % (pc["key"], k)
        if k in want and n:
            _untouched(bufs[k][M:], what + " behind M")
            assert bool(torch.isfinite(bufs[k][:M]).all()), what + ": not finite"
            out[k] = bufs[k][:M].clone()
        else:
            _untouched(bufs[k], what)
            out[k] = None if k not in want else bufs[k][:M, :0].clone()
    return out


def _pose_check(pc, out, use_gj=True, use_gxt=True, tag=""):
    ref = B.pose_reference(pc, use_gj, use_gxt)
    for k in POSE_OUTPUTS:
        _check("hps_smpl_pose_prep_backward %s %s%s" % (pc["key"], tag, k), out[k], *ref[k])


def _equal_outputs(x, y, what, rows=slice(None)):
    for k in POSE_OUTPUTS:
        if x[k] is not None and y[k] is not None:
            assert torch.equal(x[k][rows], y[k]), "%s: %s differs" % (what, k)


@pytest.mark.parametrize("key", B.POSE_CASES, ids=lambda k: "%s-nb%d-M%d-rotmat%d-rows%d" % k)
def test_pose_prep_backward_on_other_trees(key, dev):
    """(c) the SMPL tree, a chain of depth 31, a star of 31 children, chain7, a mixed tree and a single joint: the rule per gradient tensor,
    with g_joints NULL and with g_xt NULL too; each output NULL in turn leaves the others' bits alone; guards; repeatable bits; a mesh alone
    has the bits it has in the batch; the M = 1 call of the all-zero-rotation mesh is finite and obeys the rule of its own references."""
    pc = B.pose_case(*key)
    M = pc["M"]
    o = _pose_args(pc, dev)
    out = _pose(pc, o, dev)
    _pose_check(pc, out)
    _equal_outputs(out, _pose(pc, o, dev), "second run")
    _pose_check(pc, _pose(pc, o, dev, use_gj=False), use_gj=False, tag="g_joints=NULL ")
    _pose_check(pc, _pose(pc, o, dev, use_gxt=False), use_gxt=False, tag="g_xt=NULL ")
    for absent in POSE_OUTPUTS:
        _equal_outputs(out, _pose(pc, o, dev, want=tuple(k for k in POSE_OUTPUTS if k != absent)), absent + " = NULL")
    for m in sorted({0, M - 1, M // 2}):
        one_pc = B.one_pose(pc, m)
        one = _pose(one_pc, _pose_args(one_pc, dev), dev)
        _equal_outputs(out, one, "mesh %d alone" % m, rows=slice(m, m + 1))
        if m == pc["zero_mesh"]:
            assert not one_pc["glob"].any() and not one_pc["body"].any()
            _pose_check(one_pc, one, tag="zero rotations ")


# ---------------------------------------------------------------------------------------------------------------------------------
# (d) the chain
# ---------------------------------------------------------------------------------------------------------------------------------
def test_chain_on_a_mixed_tree(dev):
    """(d) hps_smpl_pose_prep, hps_smpl_blend, then the three backward calls as SMPL._backward strings them: 13 joints, V = 300, K = 8, 16
    shape coefficients, kp = 128, M = 9, five regressor rows, against float64 autograd through the composite.  The forward stage's own
    outputs (xt, a, j_posed: hps_smpl_pose_prep on a tree other than SMPL's) are held to the rule first, so a failure names its stage."""
    cc = B.chained_case()
    pc, M, V, J, n_rows, np_ = cc["pose"], cc["M"], cc["V"], cc["J"], cc["n_rows"], cc["np"]
    kp, mp, rows = pc["kp"], pc["mp"], pc["rows"]
    assert (J, kp, rows) == (13, 128, 124)
    o = _pose_args(pc, dev)
    s = _capi.stream()
    xt = torch.full((kp + 1, mp), SENT, device=dev)
    xt[:kp, M:] = float("nan")                                            # (SMPL._backward allocates it with torch.empty)
    a, j_posed = torch.full((M + 1, J, 12), SENT, device=dev), torch.full((M + 1, J, 3), SENT, device=dev)
    fwd = _pose_forward_args(pc, o)
    _capi.call("hps_smpl_pose_prep", *fwd, P(xt), kp, mp, P(a), P(j_posed), None, M, s)
    torch.cuda.synchronize()
    for t, what in ((xt[kp:], "xt"), (a[M:], "a"), (j_posed[M:], "j_posed")):
        _untouched(t, "hps_smpl_pose_prep " + what)
    assert bool(torch.isnan(xt[:kp, M:]).all()) and bool((xt[rows:kp, :M] == 0).all())
    stage = {}
    for dtype in (torch.float64, torch.float32):
        with torch.no_grad():
            x = {k: pc[k].to(dtype) for k in ("glob", "body", "betas")}
            for k, y in zip(("xt", "a", "j_posed"), B.pose_prep(pc, dtype, x["glob"], x["body"], x["betas"])):
                stage.setdefault(k, []).append(y.double().contiguous())
    _check("hps_smpl_pose_prep mixed12 xt", xt[:rows, :M], *stage["xt"])
    _check("hps_smpl_pose_prep mixed12 a", a[:M], *stage["a"])
    _check("hps_smpl_pose_prep mixed12 j_posed", j_posed[:M], *stage["j_posed"])

    bmat, vt = cc["bmat"].to(dev), cc["v_template"].reshape(-1).contiguous().to(dev)
    ld = np_
    v_posed = torch.full((M + 1, ld), SENT, device=dev)
    _capi.call("hps_smpl_blend", P(xt), P(bmat), P(vt), P(v_posed), M, 3 * V, kp, mp, np_, ld, s)
    w_idx, w_val = cc["w_idx"].to(dev), cc["w_val"].to(dev)
    ptr, row, val = (_on(dev, t) for t in cc["csrt"])
    g_verts, g_joints = cc["g_verts"].to(dev), cc["g_joints"].to(dev)
    g_a, g_tr = torch.full((M + 1, J, 12), SENT, device=dev), torch.full((M + 1, 3), SENT, device=dev)
    ws, n_ws = _workspace(_capi.WS_SMPL_LBS_BWD, M, V, J, dev)
    _capi.call("hps_smpl_lbs_backward", P(v_posed), ld, P(a), IP(w_idx), P(w_val), cc["K"], J, P(g_verts), P(g_joints), n_rows, IP(ptr), IP(row),
               P(val), P(g_a), P(g_tr), P(ws), M, V, s)
    g_xt = torch.full((kp + 1, mp), SENT, device=dev)
    ws2, n_ws2 = _workspace(_capi.WS_SMPL_BLEND_BWD, M, kp, np_, dev)
    _capi.call("hps_smpl_blend_backward", P(bmat), P(v_posed), P(g_xt), P(ws2), M, kp, mp, np_, ld, s)
    per = {k: torch.full((M + 1, n), SENT, device=dev) for k, n in (("glob", 3), ("body", 3 * (J - 1)), ("betas", pc["nb"]))}
    _capi.call("hps_smpl_pose_prep_backward", *fwd, P(g_a), P(g_joints), n_rows, P(g_xt), mp, P(per["glob"]), P(per["body"]), P(per["betas"]),
               M, s)
    torch.cuda.synchronize()
    for t, what in ((v_posed[M:], "v_posed"), (g_a[M:], "g_a"), (g_tr[M:], "g_transl"), (ws[n_ws:], "lbs workspace"), (g_xt[kp:], "g_xt"),
                    (ws2[n_ws2:], "blend workspace")) + tuple((per[k][M:], "g_" + k) for k in per):
        _untouched(t, "chain: " + what)
    ref = B.chained_reference()
    _check("chain transl", g_tr[:M], *ref["transl"])
    for k in ("glob", "body", "betas"):
        _check("chain " + k, per[k][:M], *ref[k])
