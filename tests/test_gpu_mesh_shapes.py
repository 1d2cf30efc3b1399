"""GPU: the SMPL mesh kernels -- hps_smpl_mesh_fused, hps_smpl_mesh_fused_picks, hps_smpl_mesh_fused_shared_shape (csrc/mesh_fused.hip),
hps_smpl_split_bf16x3 + hps_smpl_mesh_fused_shared_shape_bf16x3 (csrc/mesh_split.hip), their shared epilogue (csrc/mesh_epilogue.h) and the
unfused definition hps_smpl_blend + hps_smpl_lbs -- against the float64 definition of include/hps.h at vertex counts, row counts, mesh
counts, joint counts and weight counts other than SMPL's (tests/mesh_scenario.py: cases, references, rule), through the C ABI.

Every output is allocated with one guard mesh behind it and pre-filled with a sentinel: after the call the guard and every element the
ABI says is not written hold the sentinel exactly, and the live outputs are finite (the padding columns of the mesh operand hold NaN).

The rule is mesh_scenario.bound: err <= 4 * max(e_cpu32, e_pair32, 2^-23 max|y64|).  Worst err / (2^-23 max|y64|) measured on an MI355X per
entry point over the cases below.  The references' own ratios lie between 0.2 and 1.1 -- 1.6 for v_posed of the one-vertex case, whose
largest coordinate is small -- so the bound is 4.0 throughout, 4.1 and 6.5 in two cases; every kernel sits as close to float64 as they do:

    hps_smpl_mesh_fused (K = 4, 8, 12; 25 cases)                        0.74
    hps_smpl_blend, v_posed (34 cases)                                  1.00   (1.60 of a bound of 6.50 at M = 130, V = 1, kp = 224)
    hps_smpl_lbs behind it (K = 4, 8, 12, 24; 34 cases)                 0.74
    hps_smpl_mesh_fused_picks (7 cases)                                 0.70
    hps_smpl_mesh_fused_shared_shape (6 cases)                          0.75
    hps_smpl_v_shaped (6 cases)                                         0.39
    hps_smpl_split_bf16x3 + hps_smpl_mesh_fused_shared_shape_bf16x3     0.78   (8 cases)
    SMPL.forward with 1..16 shape coefficients (smpl_grad_scenario.bound: 4 x the oracle's own fp32 error, which is up to 3.1 here)
        vertices 3.28 where the oracle's fp32 has 3.06 (bound 12.2); closest to its bound: 1.56 of 5.16
        joints   2.83 where the oracle's fp32 has 1.93 (bound 7.7);  closest to its bound: 2.16 of 5.04
    SMPL.forward, 11 coefficients, shared shapes, f32 and bf16x3 alike: vertices 2.11 of 10.0, joints 2.12 of 6.88
"""
import pytest
import torch

import mesh_scenario as S
import smpl_grad_scenario as G
from hierarchicalprobabilistic3dhuman_amd import _capi, configs, smpl_data
from oracle import ref_cpu as O

pytestmark = pytest.mark.gpu
SENT = -777.25
P, IP = _capi.ptr, _capi.iptr


class _Ops:
    """The operands of a case on the device, in the layouts of include/hps.h."""

    def __init__(self, c, dev):
        V = c["V"]
        self.xt = c["xt"].to(dev)
        self.bmat = S.blend_matrix(c).to(dev)
        self.bmat_p = S.panel_permuted(c["bmat"], V).to(dev)
        self.np128, self.npf = self.bmat.shape[1], self.bmat_p.shape[1]
        assert self.npf == _capi.load().hps_smpl_mesh_fused_np(V)
        self.vt = c["v_template"].reshape(-1).contiguous().to(dev)
        self.a, self.w_idx, self.w_val = c["a"].to(dev), c["w_idx"].to(dev), c["w_val"].to(dev)
        self.transl = None if c["transl"] is None else c["transl"].to(dev)


def _guarded(M, n, dev):
    return torch.full((M + 1, n, 3), SENT, device=dev)


def _live(out, M, what):
    """The guard mesh is untouched and the live meshes are finite -> the live part."""
    torch.cuda.synchronize()
    assert bool((out[M:] == SENT).all()), what + ": written behind the last mesh"
    assert bool(torch.isfinite(out[:M]).all()), what + ": not finite"
    return out[:M]


def _fused(c, o, dev, vt=None):
    verts = _guarded(c["M"], c["V"], dev)
    _capi.call("hps_smpl_mesh_fused", P(o.xt), P(o.bmat_p), P(o.vt if vt is None else vt), P(o.a), IP(o.w_idx), P(o.w_val), c["K"], c["J"],
               P(o.transl), P(verts), c["M"], c["V"], c["kp"], c["mp"], o.npf, _capi.stream())
    return _live(verts, c["M"], "hps_smpl_mesh_fused")


def _unfused(c, o, dev):
    """hps_smpl_blend + hps_smpl_lbs -> (verts, v_posed (M, V, 3)); v_posed rows have a pitch beyond 3 V, and the columns behind 3 V and
    the row behind M keep the sentinel."""
    M, V = c["M"], c["V"]
    ldv = o.np128 + 32
    v_posed = torch.full((M + 1, ldv), SENT, device=dev)
    _capi.call("hps_smpl_blend", P(o.xt), P(o.bmat), P(o.vt), P(v_posed), M, 3 * V, c["kp16"], c["mp"], o.np128, ldv, _capi.stream())
    torch.cuda.synchronize()
    assert bool((v_posed[M:] == SENT).all()) and bool((v_posed[:, 3 * V:] == SENT).all()), "hps_smpl_blend: written outside (M, 3 V)"
    assert bool(torch.isfinite(v_posed[:M, :3 * V]).all())
    verts = _guarded(M, V, dev)
    _capi.call("hps_smpl_lbs", P(v_posed), ldv, P(o.a), IP(o.w_idx), P(o.w_val), c["K"], c["J"], P(o.transl), P(verts), M, V, _capi.stream())
    return _live(verts, M, "hps_smpl_lbs"), v_posed[:M, :3 * V].reshape(M, V, 3)


def _pick_table(V, dev):
    """pick_slot (V,) and the vertex of every slot: vertex 0, vertex V - 1 and the vertices on both sides of every panel edge, in slots
    that are NOT in vertex order."""
    chosen = sorted({0, V - 1} | {v for e in range(64, V, 64) for v in (e - 1, e)})
    n = len(chosen)
    slots = [(5 * i + 2) % n for i in range(n)] if n % 5 else [(3 * i + 1) % n for i in range(n)]
    assert sorted(slots) == list(range(n))
    pick_slot = torch.full((V,), -1, dtype=torch.int32)
    vertex_of_slot = torch.zeros(n, dtype=torch.long)
    for v, s in zip(chosen, slots):
        pick_slot[v] = s
        vertex_of_slot[s] = v
    return pick_slot.to(dev), vertex_of_slot.to(dev), n


def _picks(c, o, dev):
    M, V = c["M"], c["V"]
    pick_slot, vertex_of_slot, n = _pick_table(V, dev)
    verts, picked = _guarded(M, V, dev), _guarded(M, n, dev)
    _capi.call("hps_smpl_mesh_fused_picks", P(o.xt), P(o.bmat_p), P(o.vt), P(o.a), IP(o.w_idx), P(o.w_val), c["K"], c["J"], P(o.transl),
               P(verts), M, V, c["kp"], c["mp"], o.npf, IP(pick_slot), P(picked), n, _capi.stream())
    verts, picked = _live(verts, M, "hps_smpl_mesh_fused_picks"), _live(picked, M, "hps_smpl_mesh_fused_picks: picked")
    assert torch.equal(picked, verts[:, vertex_of_slot])
    return verts, picked


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,V,kp,J,transl", S.FUSED_CASES)
def test_fused_kernel_at_other_shapes(M, V, kp, J, transl, dev):
    """(a) hps_smpl_mesh_fused with K = 4: the rule against float64, the bits of hps_smpl_blend + hps_smpl_lbs on the same operands (the
    promise of include/hps.h), and the blend's v_posed itself under the rule."""
    c = S.case(M, V, kp, J, 4, transl)
    o, ref = _Ops(c, dev), S.reference(c)
    fused = _fused(c, o, dev)
    unfused, v_posed = _unfused(c, o, dev)
    S.check_case("hps_smpl_mesh_fused %s" % (c["key"],), ref, y_dev=fused)
    S.check_case("hps_smpl_blend %s" % (c["key"],), ref, vp_dev=v_posed)
    S.check_case("hps_smpl_lbs %s" % (c["key"],), ref, y_dev=unfused)
    assert torch.equal(fused, unfused), float((fused - unfused).abs().max())


@pytest.mark.parametrize("M,V,kp,K,transl", S.FUSED_WIDE_CASES)
def test_fused_kernel_with_eight_and_twelve_weights(M, V, kp, K, transl, dev):
    """(b) K = 8 and 12 with 24 joints: the rule, and the bits of the unfused pair."""
    c = S.case(M, V, kp, 24, K, transl)
    o, ref = _Ops(c, dev), S.reference(c)
    fused = _fused(c, o, dev)
    unfused, v_posed = _unfused(c, o, dev)
    S.check_case("hps_smpl_mesh_fused K=%d %s" % (K, c["key"]), ref, y_dev=fused)
    S.check_case("hps_smpl_lbs K=%d %s" % (K, c["key"]), ref, y_dev=unfused, vp_dev=v_posed)
    assert torch.equal(fused, unfused), float((fused - unfused).abs().max())


@pytest.mark.parametrize("M,V,kp,K,transl", S.LBS_CASES)
def test_lbs_kernel_with_wide_weights_around_its_vertex_tile(M, V, kp, K, transl, dev):
    """(b) hps_smpl_lbs with K = 8, 12, 24 at V = 1, 200, 257, 300 (both sides of its 256-vertex tile) behind hps_smpl_blend: the rule; where
    the fused kernel exists (K = 8, 12) it gives the same bits."""
    c = S.case(M, V, kp, 24, K, transl)
    o, ref = _Ops(c, dev), S.reference(c)
    unfused, v_posed = _unfused(c, o, dev)
    S.check_case("hps_smpl_lbs K=%d %s" % (K, c["key"]), ref, y_dev=unfused, vp_dev=v_posed)
    if K != 24:
        assert torch.equal(_fused(c, o, dev), unfused)


@pytest.mark.parametrize("M,V,kp,transl", S.PICKS_CASES)
def test_side_output_at_other_shapes(M, V, kp, transl, dev):
    """(c) hps_smpl_mesh_fused_picks (the TAIL = 5 instantiations) with 1, 2 and 14 chunks in the four-stage K loop (M <= 128) and the
    two-stage one: picked == verts[:, chosen] bit for bit and untouched behind M, verts the bits of the plain entry point, the rule; and
    the dev library's two-stage switch gives the same bits as the four-stage loop at these short kp."""
    c = S.case(M, V, kp, 24, 4, transl)
    o, ref = _Ops(c, dev), S.reference(c)
    verts, picked = _picks(c, o, dev)
    S.check_case("hps_smpl_mesh_fused_picks %s" % (c["key"],), ref, y_dev=verts)
    assert torch.equal(verts, _fused(c, o, dev))
    with _capi.dev_library():
        try:
            _capi.call("hps_dev_mesh_stages", 2)
            verts2, picked2 = _picks(c, o, dev)
        finally:
            _capi.call("hps_dev_mesh_stages", 0)
    assert torch.equal(verts2, verts) and torch.equal(picked2, picked)


def _shared_shape(c, o, sh, group_rows, dev):
    M, V = c["M"], c["V"]
    pick_slot, vertex_of_slot, n = _pick_table(V, dev)
    verts, picked = _guarded(M, V, dev), _guarded(M, n, dev)
    v_shaped, mesh_row, group_rows = sh["v_shaped"].to(dev), sh["mesh_row"].to(dev), group_rows.to(dev)      # (named: they must outlive the call)
    _capi.call("hps_smpl_mesh_fused_shared_shape", P(o.xt), P(o.bmat_p), P(v_shaped), IP(mesh_row), IP(group_rows),
               P(o.a), IP(o.w_idx), P(o.w_val), 4, 24, P(verts), M, V, c["kp"], c["mp"], o.npf, IP(pick_slot), P(picked), n, _capi.stream())
    verts, picked = _live(verts, M, "hps_smpl_mesh_fused_shared_shape"), _live(picked, M, "hps_smpl_mesh_fused_shared_shape: picked")
    assert torch.equal(picked, verts[:, vertex_of_slot])
    return verts


@pytest.mark.parametrize("M,V,kp", S.SHARED_CASES)
def test_shared_shape_kernel_at_other_shapes(M, V, kp, dev):
    """(d) hps_smpl_mesh_fused_shared_shape (TAIL = 8) on three shaped templates and group tables with split = 0, 1, 31, 32 and -1 (a tile
    with a split < 0 group beside an ordinary one): the rule against float64 built from the shaped templates, and the same bits when
    every group says -1."""
    c = S.case(M, V, kp)
    o, sh, ref = _Ops(c, dev), S.shared(c), S.reference(c, S.SHARED_R)
    verts = _shared_shape(c, o, sh, sh["group_rows"], dev)
    S.check_case("hps_smpl_mesh_fused_shared_shape %s" % (c["key"],), ref, y_dev=verts)
    assert torch.equal(_shared_shape(c, o, sh, S.every_group_fetches_per_mesh(sh["group_rows"]), dev), verts)


@pytest.mark.parametrize("R,nb,V", S.V_SHAPED_CASES)
def test_v_shaped_with_other_coefficient_counts(R, nb, V, dev):
    """(d) hps_smpl_v_shaped at num_betas = 0, 1, 10, 16 (the range of the C ABI) and R = 1, 3 against float64 under the rule."""
    vc = S.v_shaped_case(R, nb, V)
    out = torch.full((R + 1, 3 * V), SENT, device=dev)
    betas = vc["betas"].to(dev) if nb else torch.zeros(1, device=dev)                 # (num_betas = 0: nothing is read, any pointer)
    rows = vc["shape_rows"].to(dev) if nb else torch.zeros(1, device=dev)
    vt = vc["v_template"].to(dev)
    _capi.call("hps_smpl_v_shaped", P(betas), nb, P(rows), vc["ld"], P(vt), P(out), R, V, _capi.stream())
    torch.cuda.synchronize()
    assert bool((out[R:] == SENT).all()) and bool(torch.isfinite(out[:R]).all())
    S.check("hps_smpl_v_shaped %s" % ((R, nb, V),), out[:R], vc["y64"], vc["y_cpu32"], vc["y_seq32"])
    if nb == 0:
        assert torch.equal(out[:R].cpu(), vc["v_template"][None].expand(R, -1))


def _split(src, rows, tile, dev):
    lib = _capi.load()
    n = lib.hps_smpl_split_bf16x3_bytes(rows, src.shape[1])
    dst = torch.full((n + 64,), 0x55, dtype=torch.uint8, device=dev)
    _capi.call("hps_smpl_split_bf16x3", P(src), rows, src.shape[1], src.shape[1], tile, _capi._P(dst.data_ptr()), _capi.stream())
    torch.cuda.synchronize()
    assert bool((dst[n:] == 0x55).all()), "hps_smpl_split_bf16x3: written behind its output"
    return dst


@pytest.mark.parametrize("M,V,rows,R", S.SPLIT_CASES)
def test_bf16x3_kernel_at_other_shapes(M, V, rows, R, dev):
    """(e) hps_smpl_split_bf16x3 + hps_smpl_mesh_fused_shared_shape_bf16x3 with 1, 2 and 14 chunks, whole and ragged: the same rule (hps.h
    claims fp32 accuracy), no further from float64 than the fp32-MFMA form of the same case (the 1.25 x max / 1.1 x mean comparison of
    test_split_bf16_form_of_the_mesh_kernel), and the NaN padding columns of the mesh operand do not leak."""
    c = S.case(M, V, rows)
    o, sh, ref = _Ops(c, dev), S.shared(c, R), S.reference(c, R)
    assert bool(torch.isnan(o.xt[:rows, M:]).all())
    xsplit = _split(o.xt, rows, _capi.load().hps_smpl_split_bf16x3_mesh_tile(), dev)
    bsplit = _split(o.bmat_p, rows, 192, dev)
    pick_slot, vertex_of_slot, n = _pick_table(V, dev)
    verts, picked = _guarded(M, V, dev), _guarded(M, n, dev)
    v_shaped, mesh_row, group_rows = sh["v_shaped"].to(dev), sh["mesh_row"].to(dev), sh["group_rows"].to(dev)
    _capi.call("hps_smpl_mesh_fused_shared_shape_bf16x3", _capi._P(xsplit.data_ptr()), _capi._P(bsplit.data_ptr()), P(v_shaped), IP(mesh_row),
               IP(group_rows), P(o.a), IP(o.w_idx), P(o.w_val), 4, 24, P(verts), M, V, rows, c["mp"], IP(pick_slot), P(picked), n,
               _capi.stream())
    verts, picked = _live(verts, M, "hps_smpl_mesh_fused_shared_shape_bf16x3"), _live(picked, M, "bf16x3: picked")
    assert torch.equal(picked, verts[:, vertex_of_slot])
    S.check_case("hps_smpl_mesh_fused_shared_shape_bf16x3 %s R=%d" % (c["key"], R), ref, y_dev=verts)
    if R == 1:
        f32 = _fused(c, o, dev, vt=v_shaped.reshape(-1))
    else:
        f32 = _shared_shape(c, o, sh, sh["group_rows"], dev)
    e_sp = (verts.cpu().double() - ref["y64"]).abs()
    e_f32 = (f32.cpu().double() - ref["y64"]).abs()
    print("bf16x3 / fp32-MFMA error against float64: max %.3e / %.3e  mean %.3e / %.3e" % (e_sp.max(), e_f32.max(), e_sp.mean(), e_f32.mean()))
    assert float(e_sp.max()) <= max(1.25 * float(e_f32.max()), 1e-6) and float(e_sp.mean()) <= 1.1 * float(e_f32.mean()) + 1e-9


# ---------------------------------------------------------------------------------------------------------------------------------
def _module_inputs(M, nb, pose2rot, with_t, seed):
    g = torch.Generator().manual_seed(seed)
    betas = torch.randn(M, nb, generator=g)
    aa = torch.randn(M, 24, 3, generator=g) * 0.5
    tr = torch.randn(M, 3, generator=g) if with_t else None
    if pose2rot:
        return dict(betas=betas, body_pose=aa[:, 1:].reshape(M, 69).contiguous(), global_orient=aa[:, 0].contiguous(), transl=tr, pose2rot=True)
    R = O.batch_rodrigues(aa.double().view(-1, 3)).view(M, 24, 3, 3).float()
    return dict(betas=betas, body_pose=R[:, 1:].contiguous(), global_orient=R[:, :1].contiguous(), transl=tr, pose2rot=False)


def _oracle(p, x):
    dt = p.dtype
    out = O.smpl_forward(p, **{k: (v.to(dt) if torch.is_tensor(v) else v) for k, v in x.items()})
    return out["vertices"].double(), out["joints"].double()


def _check_module(name, out, x, p64, p32):
    v64, j64 = _oracle(p64, x)
    v32, j32 = _oracle(p32, x)
    assert bool(torch.isfinite(out.vertices).all()) and bool(torch.isfinite(out.joints).all())
    G.check(name + " vertices", out.vertices, v64, v32)
    G.check(name + " joints", out.joints, j64, j32)


@pytest.mark.parametrize("nb", S.MODULE_NUM_BETAS)
def test_module_with_other_shape_coefficient_counts(nb, dev):
    """(f) SMPL with 1, 2, 5, 9, 11, 16 shape coefficients (kp = 208, 210, 212, 216, 218, 224 at V = 6890) on both input routes, with and
    without translation, against oracle.ref_cpu.smpl_forward in float64 and its fp32 twin under smpl_grad_scenario.bound, vertices and
    joints.  With 11 coefficients the shared-shape route (f32 and bf16x3) runs too: SMPL.forward used to pass it an odd row count."""
    from hierarchicalprobabilistic3dhuman_amd.smpl_official import SMPL
    model = smpl_data.synthetic_smpl_model(20 + nb, num_betas=nb)
    extra = smpl_data.load_extra_joint_regressors(None)
    p64 = O.SMPLParams(model, extra, configs.SMPLX_EXTRA_VERTEX_IDS, num_betas=nb, dtype=torch.float64)
    p32 = O.SMPLParams(model, extra, configs.SMPLX_EXTRA_VERTEX_IDS, num_betas=nb, dtype=torch.float32)
    smpl = SMPL(model, num_betas=nb).to(dev)
    on_dev = lambda x: {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in x.items()}
    for M, pose2rot, with_t in ((3, True, True), (3, False, False), (130, False, True), (130, True, False)):
        x = _module_inputs(M, nb, pose2rot, with_t, 1000 * nb + M + int(with_t))
        _check_module("SMPL nb=%d M=%d pose2rot=%d transl=%d" % (nb, M, pose2rot, with_t), smpl(**on_dev(x)), x, p64, p32)
    if nb == 11:
        B, N = 2, 20
        rows = list(range(B)) + list(range(B)) + [b for b in range(B) for _ in range(N)]
        x = _module_inputs(len(rows), nb, False, False, 77)
        loc = torch.randn(B, nb, generator=torch.Generator().manual_seed(78))
        x["betas"] = loc[torch.tensor(rows)]
        mesh_row, group_rows = smpl.shared_shape_tables(rows)
        plain, seen = smpl(**on_dev(x)), []
        for arith in ("f32", "bf16x3"):
            smpl.mesh_arith = arith
            try:
                out = smpl(_shared_shapes=(loc.to(dev), mesh_row, group_rows), **on_dev(x))
            finally:
                smpl.mesh_arith = "f32"
            assert not torch.equal(out.vertices, plain.vertices)                       # (the other kernel did run)
            assert all(not torch.equal(out.vertices, other) for other in seen)
            seen.append(out.vertices)
            _check_module("SMPL nb=11 shared shapes %s" % arith, out, x, p64, p32)

