"""The cases, references and rule of the SMPL mesh-kernel tests (tests/mesh_scenario.py) on the host: every reference of every GPU case
stays inside its bound, the pair-ordered reference is the same function as the float64 one, the layout helpers round-trip, the rule
fails the defects a mesh kernel can have -- and the row count SMPL.forward passes to the shared-shape kernel is even for every number of
shape coefficients."""
import pytest
import torch

import mesh_scenario as S
from hierarchicalprobabilistic3dhuman_amd import smpl_data
from hierarchicalprobabilistic3dhuman_amd.smpl_official import SMPL


def test_every_reference_of_every_gpu_case_is_inside_its_bound():
    seen = set()
    for name, c, R in S.all_cases():
        if (c["key"], R) in seen:
            continue
        seen.add((c["key"], R))
        ref = S.reference(c, R)
        for out in ("y", "vp"):
            y64 = ref[out + "64"]
            assert torch.isfinite(y64).all(), (name, c["key"])               # (the NaN padding columns of xt are not part of any mesh)
            unit = S.EPS32 * float(y64.abs().max())
            for fam in ("_cpu32", "_pair32"):
                e = float((ref[out + fam] - y64).abs().max())
                assert e <= S.bound(y64, ref[out + "_cpu32"], ref[out + "_pair32"]), (name, c["key"], out, fam)
                # the references are what the issue measured them to be: about one fp32 rounding of the largest coordinate, so the
                # bound is about four of them (a reference that drifted to many roundings would widen the rule unnoticed)
                assert e <= 2.0 * unit, (name, c["key"], out, fam, e / unit)
    for R, nb, V in S.V_SHAPED_CASES:
        vc = S.v_shaped_case(R, nb, V)
        for fam in ("y_cpu32", "y_seq32"):
            assert float((vc[fam] - vc["y64"]).abs().max()) <= 2.0 * S.EPS32 * float(vc["y64"].abs().max())


@pytest.mark.parametrize("key,R", [((65, 129, 214, 24, 4, False), None), ((52, 200, 26, 24, 4, True), None), ((40, 33, 16, 24, 4, False), 3),
                                   ((9, 257, 218, 24, 24, False), None), ((300, 33, 17, 24, 4, False), 1)])
def test_pair_order_is_the_same_function(key, R):
    c = S.case(*key)
    sh = None if R is None else S.shared(c, R)
    ref = S.reference(c, R)
    y_pair64, vp_pair64 = S.forward(c, torch.float64, pair=True, sh=sh)
    assert float((y_pair64 - ref["y64"]).abs().max()) <= 1e-12 * float(ref["y64"].abs().max())
    assert float((vp_pair64 - ref["vp64"]).abs().max()) <= 1e-12 * float(ref["vp64"].abs().max())
    if c["rows"] > 2:                                                        # (with one k-pair there is one order)
        assert not torch.equal(ref["y_pair32"], ref["y_cpu32"]) and not torch.equal(ref["vp_pair32"], ref["vp_cpu32"])


@pytest.mark.parametrize("V", [1, 33, 65, 200])
def test_layout_helpers_round_trip(V):
    c = S.case(3, V, 18)
    bp = S.panel_permuted(c["bmat"], V)
    assert bp.shape == (32, -(-V // 64) * 192)
    assert torch.equal(S.panel_unpermuted(bp, V), c["bmat"])
    for v, ch in ((0, 0), (V - 1, 2), (V // 2, 1)):                           # the formula of include/hps.h, entry by entry
        assert torch.equal(bp[:, (v // 64) * 192 + ch * 64 + v % 64], c["bmat"][:, 3 * v + ch])
    used = torch.zeros(bp.shape[1], dtype=torch.bool)
    used[S._panel_columns(V)] = True
    assert int(used.sum()) == 3 * V and not bp[:, ~used].any()                # a permutation; unused columns zero
    b128 = S.blend_matrix(c)
    assert b128.shape[1] % 128 == 0 and torch.equal(b128[:, :3 * V], c["bmat"]) and not b128[:, 3 * V:].any()
    assert not c["bmat"][18:].any() and not c["xt"][18:].any() and torch.isnan(c["xt"][:18, 3:]).all() and torch.isfinite(c["xt"][:, :3]).all()


def test_case_recipe():
    c = S.case(70, 200, 210, 24, 8, True)
    nnz = (c["w_val"] != 0).sum(1)
    assert int(nnz.min()) >= 1 and int(nnz.max()) == 8 and int(nnz[0]) == 1 and int(nnz[-1]) == 1
    assert float(c["w_val"][0, 0]) == 1.0 and float(c["w_val"][-1, 0]) == 1.0
    assert float((c["w_val"].double().sum(1) - 1).abs().max()) <= 1e-6
    assert bool(((c["w_val"] != 0) | (c["w_idx"] == 0)).all())                # padded with (0, 0.0f)
    for v in range(200):                                                      # distinct joints
        live = c["w_idx"][v][c["w_val"][v] != 0]
        assert live.unique().numel() == live.numel()
    R = c["a"].view(70, 24, 3, 4)[..., :3].double()
    assert float((R @ R.transpose(-1, -2) - torch.eye(3, dtype=torch.float64)).abs().max()) <= 1e-6
    sh = S.shared(S.case(200, 64, 16), 3)
    gr, mr = sh["group_rows"].view(-1, 3), sh["mesh_row"]
    assert {int(s) for s in gr[:, 2]} == {0, 1, 31, 32, -1} and int(gr[0, 2]) >= 0 > int(gr[1, 2])
    for gi in range(gr.shape[0]):                                             # the table says what the rows are
        a, b, split = (int(x) for x in gr[gi])
        r = mr[32 * gi:32 * gi + 32]
        if split >= 0:
            assert bool((r[:split] == a).all()) and bool((r[split:] == b).all()) and a != b
        else:
            assert int((r[1:] != r[:-1]).sum()) > 1
    assert int(mr.min()) >= 0 and int(mr.max()) < 3


@pytest.mark.parametrize("defect", S.DEFECTS)
def test_the_rule_has_teeth(defect):
    """Each defect, injected into the fp32 evaluation, fails check() -- on a ragged last panel, a ragged mesh tile, the SMPL row count."""
    c = S.case(70, 200, 218, 24, 4, True)
    sh = None
    if defect == "row_a_at_split":
        c = S.case(40, 33, 16)
        sh = S.shared(c, 3)
    ref = S.reference(c, None if sh is None else 3)
    good, _ = S.forward(c, torch.float32, sh=sh)
    S.check("no defect", good, ref["y64"], ref["y_cpu32"], ref["y_pair32"])
    bad, _ = S.forward(c, torch.float32, sh=sh, defect=defect)
    assert not torch.equal(bad, good)
    with pytest.raises(AssertionError):
        S.check(defect, bad, ref["y64"], ref["y_cpu32"], ref["y_pair32"])


def test_shared_shape_row_count_is_even_for_every_number_of_shape_coefficients():
    """SMPL.forward passes _kp_pose as kp of hps_smpl_mesh_fused_shared_shape (the library refuses an odd one: _k_used - num_betas was 207
    with 11 shape coefficients), on operands advanced by num_betas rows: it is even, covers the pose rows, and where the form is taken
    (_k_used == 218) the rows it multiplies lie inside the zero-padded allocation.  num_betas = 0 is refused by the constructor."""
    model = smpl_data.synthetic_smpl_model(3, num_betas=16)                   # (the constructor keeps the first num_betas directions)
    for nb in range(1, 17):
        smpl = SMPL(model, num_betas=nb)
        assert smpl.shapedirs.shape[-1] == nb
        assert smpl._kp_pose % 2 == 0 and smpl._n_pose <= smpl._kp_pose <= smpl._n_pose + 1, nb
        assert smpl._k_used % 2 == 0 and smpl._k_used <= smpl._kp and smpl._kp % 16 == 0, nb
        if smpl._k_used == 218:
            assert nb + smpl._kp_pose <= smpl._kp, nb
            assert not smpl._bmat_p[nb + smpl._n_pose:].any() and not smpl._bmat[nb + smpl._n_pose:].any(), nb
    for nb in (0, -1):
        with pytest.raises(ValueError, match="num_betas"):
            SMPL(model, num_betas=nb)
