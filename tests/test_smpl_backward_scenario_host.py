"""The cases, references and rule of the SMPL backward-kernel tests (tests/smpl_backward_scenario.py) on the host: every reference of every
GPU case stays inside its bound, the closed forms are what float64 autograd gives, the kernel-ordered references are the same function as
the float64 one, the CSR helper round-trips, the rule fails the defects a backward kernel can have -- and the launch geometry of
hps_smpl_lbs_backward, restated, gives the large case (and no other) a workgroup that walks two mesh groups."""
import pytest
import torch

import smpl_backward_scenario as B

LBS_ALL = B.LBS_CASES + [B.LBS_LARGE_CASE]


def _inside(tag, y64, *family):
    """Each member's error in units of 2^-23 max|y64|, printed; every member inside the bound, and no further than eight roundings."""
    if y64.numel() == 0:
        return
    assert torch.isfinite(y64).all(), tag
    unit = B.EPS32 * float(y64.abs().max())
    b = B.bound(y64, *family)
    errs = [float((y - y64).abs().max()) for y in family]
    print("%-70s references/(2^-23 max|y64|) = %s  bound/(..) = %.2f" % (tag, " ".join("%.2f" % (e / unit) for e in errs), b / unit))
    for e in errs:
        # (a reference that drifted to many roundings would widen the rule unnoticed)
        assert e <= b and e <= 8.0 * unit, (tag, e / unit)


@pytest.mark.parametrize("key", LBS_ALL, ids=str)
def test_every_reference_of_every_lbs_case_is_inside_its_bound(key):
    c = B.lbs_case(*key)
    for name, (y64, y32, ych) in B.lbs_reference(c).items():
        _inside("lbs %s %s" % (key, name), y64, y32, ych)


def test_every_reference_of_every_blend_and_pose_case_is_inside_its_bound():
    for key in B.BLEND_CASES:
        _inside("blend %s g_xt" % (key,), *B.blend_reference(B.blend_case(*key)))
    for key in B.POSE_CASES:
        pc = B.pose_case(*key)
        for use_gj, use_gxt in ((True, True), (False, True), (True, False)):
            for name, (y64, y32) in B.pose_reference(pc, use_gj, use_gxt).items():
                _inside("pose %s gj=%d gxt=%d %s" % (key, use_gj, use_gxt, name), y64, y32)
    for name, (y64, y32) in B.chained_reference().items():
        _inside("chained %s" % name, y64, y32)


def _same(x, y, tol=1e-12):
    x, y = x.detach(), y.detach()
    return float((x - y).abs().max()) <= tol * max(float(y.abs().max()), 1e-300)


@pytest.mark.parametrize("key", B.LBS_CASES, ids=str)
def test_lbs_closed_form_is_what_float64_autograd_gives(key):
    c = B.lbs_case(*key)
    ref, auto = B.lbs_reference(c), B.lbs_autograd(c)
    for name in ("g_vposed", "g_a", "g_transl"):
        assert _same(ref[name][0], auto[name]), name


def test_blend_closed_form_is_what_float64_autograd_gives():
    bc = B.blend_case(240, 640, 129, 36)
    xt = torch.zeros(bc["kp"], bc["M"], dtype=torch.float64, requires_grad=True)
    (bc["g_vposed"][:, :bc["np"]].double() * (xt.t() @ bc["bmat"].double())).sum().backward()
    assert _same(B.blend_reference(bc)[0], xt.grad)


def test_pose_restatement_with_a_cut_is_the_oracles_chain_when_nothing_is_cut():
    pc = B.pose_case("mixed12", 1, 9, True, 0)
    x = B.pose_leaves(pc, torch.float64)
    xt, a, posed = B.pose_prep(pc, torch.float64, x["glob"], x["body"], x["betas"])
    R = torch.cat([x["glob"].view(9, 1, 3, 3), x["body"].view(9, -1, 3, 3)], dim=1)
    joints = pc["j_template"].double()[None] + torch.einsum("jcl,ml->mjc", pc["j_shapedirs"].double(), x["betas"])
    posed2, A2 = B._rigid_transform_with_cut(R, joints, pc["parents"], None)
    assert _same(posed2, posed) and _same(A2[:, :, :3].reshape(9, -1, 12), a)
    assert xt.shape == (pc["rows"], 9) and torch.equal(xt[:1], x["betas"].t())


@pytest.mark.parametrize("key", [B.LBS_CASES[4], B.LBS_CASES[6], B.LBS_CASES[5]], ids=str)
def test_chunk_order_is_the_same_function(key):
    c = B.lbs_case(*key)
    ref = B.lbs_reference(c)
    ch64 = B.lbs_backward(c, torch.float64, chunked=True)
    for name in ref:
        assert _same(ch64[name], ref[name][0]), name
    assert c["V"] > 2 * B.CHUNK and not torch.equal(ref["g_a"][1], ref["g_a"][2])      # three and more chunks: another fp32 order


@pytest.mark.parametrize("key", B.BLEND_CASES, ids=str)
def test_slice_order_is_the_same_function(key):
    bc = B.blend_case(*key)
    y64, y32, ysl = B.blend_reference(bc)
    assert _same(B.blend_backward(bc, torch.float64, sliced=True), y64)
    if bc["np"] > B.SLICE:
        assert not torch.equal(y32, ysl)


@pytest.mark.parametrize("n_rows,V", [(0, 5), (1, 1), (5, 128), (33, 129), (96, 385)])
def test_csr_transpose_round_trips(n_rows, V):
    C = B.regressor(torch.Generator().manual_seed(n_rows + V), n_rows, V)
    ptr, row, val = B.csr_transpose(C)
    assert ptr.dtype == torch.int32 and row.dtype == torch.int32 and val.dtype == torch.float32
    assert ptr.numel() == V + 1 and int(ptr[0]) == 0 and int(ptr[-1]) == row.numel() == val.numel() == int((C != 0).sum())
    assert torch.equal(B.csr_to_dense(ptr, row, val, n_rows), C)
    for v in range(V):                                                               # a vertex's entries in the order of C's rows
        r = row[int(ptr[v]):int(ptr[v + 1])]
        assert bool((r[1:] > r[:-1]).all())


def test_case_recipe():
    c = B.lbs_case(*B.LBS_CASES[4])                                                  # (17, 257, 22, 12, 66, ...)
    per_vertex = (c["csrt"][0][1:] - c["csrt"][0][:-1]).long()
    assert int(per_vertex[c["V"] - 1]) >= 1 and int(per_vertex.max()) == 6 and float((per_vertex == 0).float().mean()) > 0.6
    assert all(int((per_vertex == n).sum()) > 0 for n in (1, 2, 3))
    for key in B.LBS_CASES:
        c = B.lbs_case(*key)
        nnz = (c["w_val"] != 0).sum(1)
        assert int(nnz.min()) >= 1 and int(nnz.max()) <= min(c["K"], c["J"]) and int(nnz[0]) == 1 and int(nnz[-1]) == 1
        assert bool(((c["w_val"] != 0) | (c["w_idx"] == 0)).all()) and int(c["w_idx"].max()) < c["J"]
        assert float((c["w_val"].double().sum(1) - 1).abs().max()) <= 1e-6
        for v in range(c["V"]):
            live = c["w_idx"][v][c["w_val"][v] != 0]
            assert live.unique().numel() == live.numel()
        assert c["ld"] >= 3 * c["V"] and c["n_rows"] <= B.MAX_ROWS
    assert any(k[3] > k[2] for k in B.LBS_CASES)                                       # K > J at least once
    bc = B.blend_case(240, 640, 129, 36)
    assert not bc["bmat"][bc["rows"]:].any() and not bc["bmat"][:, bc["N"]:].any() and bc["N"] < bc["np"]
    assert bool(torch.isfinite(bc["g_vposed"][:, :640]).all()) and bool(torch.isnan(bc["g_vposed"][:, 640:]).all())
    for name in B.TREES:
        parents = B.tree(name)
        assert parents[0] == -1 and all(p < i for i, p in enumerate(parents))
    assert max(B.depth_of(B.tree("chain32"))) == 31 and max(B.depth_of(B.tree("star32"))) == 1 and len(B.tree("smpl")) == 24
    pc = B.pose_case("smpl", 10, 9, False, 66)
    assert pc["zero_mesh"] == 4 and not pc["glob"][4].any() and not pc["body"][4].any() and pc["kp"] == 224


def test_only_the_large_case_walks_two_mesh_groups_per_workgroup():
    """launch_lbs_backward, restated: the large case gives groups_per_block = 2 over a y extent of 3, so its last workgroup holds one
    group, and that group is ragged; every other case has one group per workgroup."""
    M, V = B.LBS_LARGE_CASE[:2]
    splits, gpb, y = B.lbs_launch_geometry(M, V)
    n_groups = -(-M // B.GROUP)
    assert (splits, gpb, y) == (4, 2, 3)
    assert n_groups - (y - 1) * gpb == 1 < gpb                                         # the last workgroup holds fewer groups
    assert M - (n_groups - 1) * B.GROUP == 5                                           # and its group is ragged
    for key in B.LBS_CASES:
        assert B.lbs_launch_geometry(key[0], key[1])[1] == 1, key
    assert B.lbs_launch_geometry(304, 6890)[1] == 1 and B.lbs_launch_geometry(305, 6890)[1] == 2      # (the SMPL mesh: M > 304)


LBS_DEFECTS = {
    "second_group_uses_first_groups_transforms": (B.LBS_LARGE_CASE, "g_vposed"),
    "drop_last_vertex_of_partial_chunk": (B.LBS_CASES[3], "g_a"),
    "drop_third_regressor_entry": (B.LBS_CASES[4], "g_vposed"),
    "transl_misses_one_ones_row": (B.LBS_CASES[7], "g_transl"),
    "kinematic_joints_missing_from_transl": (B.LBS_CASES[3], "g_transl"),
}
POSE_DEFECTS = {
    "star_root_misses_last_child": (("star32", 10, 9, False, 66), "g_glob"),
    "betas_without_joint_term": (("smpl", 10, 9, False, 66), "g_betas"),
    "rodrigues_without_epsilon": (("smpl", 10, 9, False, 66), "g_body"),
}


@pytest.mark.parametrize("defect", B.DEFECTS)
def test_the_rule_has_teeth(defect):
    """Each defect, applied to the float64 reference of a case of the GPU tables, fails check() against the clean references."""
    if defect in LBS_DEFECTS:
        key, name = LBS_DEFECTS[defect]
        assert key in LBS_ALL
        c = B.lbs_case(*key)
        clean = B.lbs_reference(c)[name]
        good, bad = clean[0], B.lbs_backward(c, torch.float64, defect=defect)[name]
    elif defect == "padding_columns_not_zeroed":
        c = B.lbs_case(*B.LBS_CASES[4])
        y64, y32, ych = B.lbs_reference(c)["g_vposed"]
        clean = tuple(B.vposed_rows(c, y, -777.25) for y in (y64, y32, ych))
        good, bad = clean[0], B.vposed_rows(c, y64, -777.25, defect=defect)
    elif defect in POSE_DEFECTS:
        key, name = POSE_DEFECTS[defect]
        assert key in B.POSE_CASES
        pc = B.pose_case(*key)
        clean = B.pose_reference(pc)[name]
        good, bad = clean[0], B.pose_prep_backward(pc, torch.float64, defect=defect)[name]
    else:
        bc = B.blend_case(240, 640, 129, 36)
        assert bc["key"][:4] in B.BLEND_CASES
        clean = B.blend_reference(bc)
        good, bad = clean[0], B.blend_backward(bc, torch.float64, defect=defect)
    B.check("no defect", good, *clean)
    assert not torch.equal(bad, good)
    with pytest.raises(AssertionError):
        B.check(defect, bad, *clean)
