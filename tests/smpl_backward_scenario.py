"""Seeded cases, CPU references and the accuracy rule of the SMPL backward-kernel tests (tests/test_smpl_backward_scenario_host.py,
tests/test_gpu_smpl_backward_shapes.py).  Nothing here touches a device.

The cases are built at the level of the C ABI (include/hps.h), so everything the SMPL class ties to its model is free: the vertex count V,
the joint count J, the weights per vertex K, the regressor rows, the row and column counts of the blend matrix, the kinematic tree.

hps_smpl_lbs_backward -- lbs_case(M, V, J, K, n_rows, use_gv, use_gj, ...):
    a           (M, J, 12)          [R | t], R = Rodrigues of N(0, 0.5) axis-angles, t = N(0, 0.5)
    w_idx/w_val (V, K)              1..min(K, J) non-zero weights per vertex on distinct joints, normalised to sum 1, padded with
                                    (0, 0.0f); vertex 0 and vertex V - 1 have one influence (mesh_scenario.case's recipe, K > J allowed)
    v_posed     (M, V, 3)           N(0, 0.4)
    g_verts     (M, V, 3)           N(0, 1) or None
    g_joints    (M, J + n_rows, 3)  N(0, 1) or None
    C           (n_rows, V)         sparse regressor: four vertices in five have no entry, the others 1, 2 or 3; one vertex has
                                    min(6, n_rows) and vertex V - 1 has at least one.  csr_transpose(C) is C^T in CSR form over the vertices,
                                    a vertex's entries in the order of C's rows (csrt_ptr, csrt_row, csrt_val of hps.h)
  truth (float64, the comment in hps.h):  gV' = g_verts + C^T g_joints[J:],  T_v = sum_k w A,  g_vposed_v = T_v.R^T gV'_v,
    g_a[j].R = sum_v W[v, j] gV'_v (x) v_posed_v,  g_a[j].t = sum_v W[v, j] gV'_v,  g_transl = sum_v gV'_v + sum_{j<J} g_joints[j]
  evaluated mesh group by mesh group (eight meshes), so the large case holds no (M, V, 12) float64 temporaries.

hps_smpl_blend_backward -- blend_case(kp, np, M, ld_extra):
    bmat        (kp, np)            N(0, 0.008) on the data rows (kp - 3) and the columns below 3 V (V = (np - 4) / 3), zero elsewhere
    g_vposed    (M, np + ld_extra)  N(0, 1) below 3 V, finite N(0, 1) in [3 V, np) (the ABI asks for finite values there), NaN in
                                    [np, ld_g): the kernel must never read them
  truth: g_xt[k, m] = sum_n bmat[k, n] g[m, n] in float64.

hps_smpl_pose_prep_backward -- pose_case(tree, nb, M, rotmat, n_rows):
    parents / depth of the tree, j_template (J, 3) N(0, 0.3), j_shapedirs (J, 3, nb) N(0, 0.05), betas (M, nb) N(0, 1), glob / body as
    axis-angle N(0, 0.4) (one mesh all zero where M > 1) or the rotation matrices of such vectors, cotangents g_a (M, J, 12), g_joints
    (M, J + n_rows, 3) and g_xt (kp, mp) N(0, 1)
  truth: torch float64 autograd of <g_a, a> + <g_joints[:, :J], j_posed> + <g_xt[:, :M], xt> through pose_prep(), the restatement of
  hps_smpl_pose_prep's outputs (oracle.ref_cpu.batch_rodrigues with its + 1e-8 and _rigid_transform); rotation-matrix input is
  differentiated with respect to its nine unconstrained entries.

The family of legitimate fp32 evaluations, per output tensor: the same definition in torch fp32, and where the kernel adds partial sums in
a fixed order one fp32 member in that order -- g_a and g_transl as per-128-vertex-chunk partial sums added in chunk order (g_transl: the
chunk sums added in float64 and rounded once, as hps.h states), g_xt as per-512-column-slice partial sums added in slice order.  The rule
is mesh_scenario.check, i.e. smpl_grad_scenario.bound over the family: err <= 4 * max(e_members..., 2^-23 max|y64|) per output tensor.

DEFECTS lists the wrong kernels these tests exist to catch; the reference functions take ``defect=`` and the host test shows that each
of them, applied to the float64 reference of a case of the GPU tables, fails the rule.

References are computed once per case and shared: callers must not modify them.
"""
import functools

import torch

import head_forward_scenario as HF
import mesh_scenario as MS
from mesh_scenario import EPS32, bound, check  # noqa: F401  (the accuracy rule, imported and not copied)
from oracle import ref_cpu as O

CHUNK, GROUP, MAX_ROWS = 128, 8, 96          # csrc/smpl_backward.hip: LB_CH, LB_G, LB_MAXR
SLICE, ROW_TILE = 512, 224                   # BB_SL, BB_ROWS
LD_TIGHT, LD_PLUS_ONE, LD_WIDE = "3V", "3V+1", "np+32"

# ---- the GPU cases (tests/test_gpu_smpl_backward_shapes.py); the host test holds every reference of every one of them to the rule ----
# (a) hps_smpl_lbs_backward: (M, V, J, K, n_rows, g_verts, g_joints, g_transl wanted, ld_vposed).  V: one vertex, one short of / exactly /
# one over a 128-vertex chunk, three chunks with a one-vertex tail, ragged third and fourth chunks; J: 31, 30, 25, 16, 10, 8 and one
# "ones row" behind the joints (J = 1, 2, 7, 16, 22, 24, 31); every K, twice wider than J; M on both sides of the 8-mesh group and of a wave's mesh pair; n_rows 0 (g_joints non-null) to 96
LBS_CASES = [
    (1, 1, 1, 4, 0, True, True, True, LD_TIGHT), (3, 127, 2, 8, 1, True, True, True, LD_PLUS_ONE),
    (8, 128, 7, 4, 5, False, True, False, LD_WIDE), (9, 129, 16, 12, 33, True, True, True, LD_TIGHT),
    (17, 257, 22, 12, 66, True, True, True, LD_WIDE), (70, 300, 24, 24, 96, True, True, False, LD_PLUS_ONE),
    (130, 385, 31, 4, 5, True, True, True, LD_TIGHT), (3, 300, 24, 8, 66, True, False, True, LD_WIDE),
    (9, 385, 31, 24, 96, False, True, True, LD_PLUS_ONE), (130, 129, 7, 4, 66, False, True, True, LD_TIGHT),
    (8, 257, 16, 8, 33, True, False, False, LD_TIGHT),
]
# the one case in which a workgroup walks two mesh groups (lbs_launch_geometry; the host test proves it, and that no other case does)
LBS_LARGE_CASE = (37, 66000, 24, 4, 66, True, True, True, LD_WIDE)
# (b) hps_smpl_blend_backward: (kp, np, M, ld_g - np)
BLEND_CASES = [(16, 128, 1, 0), (208, 384, 127, 36), (224, 512, 128, 0), (240, 640, 129, 36), (304, 1152, 300, 0), (448, 640, 1, 36),
               (464, 1152, 129, 36), (16, 1152, 300, 36), (224, 128, 129, 0)]
# (c) hps_smpl_pose_prep_backward: (tree, num_betas, M, rotation matrices, n_rows)
TREES = dict(smpl=None, chain7=HF.TREES["chain7"], mixed12=HF.TREES["mixed12"], chain32=(-1,) + tuple(range(31)), star32=(-1,) + (0,) * 31,
             one=(-1,))
# (a gradient of one element has nothing to be small against: max|y64| is the element itself, which cancellation makes as small as it
# likes.  So num_betas = 1 goes with rotation-matrix input, where no mesh is run alone under the rule, and M = 1 with num_betas = 0)
POSE_CASES = [("smpl", 10, 9, False, 66), ("chain32", 16, 8, True, 0), ("star32", 1, 70, True, 5), ("chain7", 0, 1, False, 0),
              ("mixed12", 16, 9, False, 5), ("one", 10, 8, False, 5), ("one", 0, 1, True, 0), ("star32", 10, 9, False, 66),
              ("chain32", 10, 70, False, 5), ("mixed12", 1, 9, True, 0), ("chain7", 16, 70, True, 5)]
# (d) the chained test: mixed 12-joint tree, V = 300, K = 8, 16 shape coefficients, M = 9, five regressor rows
CHAINED = dict(tree="mixed12", V=300, K=8, nb=16, M=9, n_rows=5)

DEFECTS = ("second_group_uses_first_groups_transforms", "drop_last_vertex_of_partial_chunk", "drop_third_regressor_entry",
           "transl_misses_one_ones_row", "kinematic_joints_missing_from_transl", "padding_columns_not_zeroed", "drop_last_slice",
           "drop_rows_behind_224", "star_root_misses_last_child", "betas_without_joint_term", "rodrigues_without_epsilon")


def _round_up(x, m):
    return (x + m - 1) // m * m


def _ceil_div(a, b):
    return (a + b - 1) // b


def lbs_launch_geometry(M, V):
    """launch_lbs_backward of csrc/smpl_backward.hip restated: (splits, groups_per_block, y extent of the grid)."""
    n_chunks, n_groups = _ceil_div(V, CHUNK), _ceil_div(M, GROUP)
    splits = min(_ceil_div(2048, n_chunks), n_groups, 65535)
    gpb = _ceil_div(n_groups, splits)
    return splits, gpb, _ceil_div(n_groups, gpb)


# ---- hps_smpl_lbs_backward ----
def skinning_weights(g, V, J, K):
    """mesh_scenario.case's recipe with K > J allowed: 1..min(K, J) non-zero weights on distinct joints, padded with (0, 0.0f)."""
    k_live = min(K, J)
    nnz = torch.randint(1, k_live + 1, (V,), generator=g)
    nnz[0] = nnz[V - 1] = 1
    joints = torch.zeros(V, K, dtype=torch.long)
    joints[:, :k_live] = torch.argsort(torch.rand(V, J, generator=g), dim=1)[:, :k_live]
    live = torch.arange(K)[None] < nnz[:, None]
    w = (torch.rand(V, K, generator=g, dtype=torch.float64) * 0.9 + 0.1) * live
    w_val = (w / w.sum(1, keepdim=True)).float().contiguous()
    w_idx = torch.where(live, joints, torch.zeros_like(joints)).to(torch.int32).contiguous()
    return w_idx, w_val


def regressor(g, n_rows, V):
    """Dense C (n_rows, V), see the module docstring."""
    C = torch.zeros(n_rows, V)
    if n_rows == 0:
        return C
    cnt = torch.randint(1, 4, (V,), generator=g) * (torch.rand(V, generator=g) < 0.2)
    cnt[V - 1] = max(int(cnt[V - 1]), 1)
    cnt[V // 2] = 6
    cnt = cnt.clamp(max=n_rows)
    order = torch.argsort(torch.rand(V, n_rows, generator=g), dim=1)                   # distinct rows per vertex
    val = torch.rand(V, n_rows, generator=g) * 0.9 + 0.1
    for v in torch.nonzero(cnt).flatten().tolist():
        rows = order[v, :int(cnt[v])]
        C[rows, v] = val[v, :int(cnt[v])]
    return C


def csr_transpose(C):
    """C^T in CSR form over the vertices: (csrt_ptr (V + 1,) int32, csrt_row int32, csrt_val fp32), each vertex's entries in the order
    of C's rows."""
    vr = torch.nonzero(C.t())                                                          # (vertex, row), sorted by vertex, then by row
    ptr = torch.zeros(C.shape[1] + 1, dtype=torch.int64)
    ptr[1:] = torch.cumsum(torch.bincount(vr[:, 0], minlength=C.shape[1]), 0)
    return ptr.to(torch.int32), vr[:, 1].to(torch.int32).contiguous(), C.t()[vr[:, 0], vr[:, 1]].contiguous()


def csr_to_dense(ptr, row, val, n_rows):
    V = ptr.numel() - 1
    C = torch.zeros(n_rows, V, dtype=val.dtype)
    for v in range(V):
        for e in range(int(ptr[v]), int(ptr[v + 1])):
            C[int(row[e]), v] = val[e]
    return C


def ld_of(V, ld):
    return {LD_TIGHT: 3 * V, LD_PLUS_ONE: 3 * V + 1, LD_WIDE: _round_up(3 * V, 128) + 32}[ld]


@functools.lru_cache(maxsize=None)
def lbs_case(M, V, J, K, n_rows, use_gv=True, use_gj=True, want_transl=True, ld=LD_TIGHT, seed=0):
    """fp32 CPU operands of one hps_smpl_lbs_backward call (see the module docstring)."""
    assert use_gv or use_gj
    g = torch.Generator().manual_seed(200003 * seed + 7919 * M + 104729 * V + 1009 * J + 13 * K + 31 * n_rows + 2 * int(use_gv) + int(use_gj))
    aa = torch.randn(M * J, 3, generator=g, dtype=torch.float64) * 0.5
    R = O.batch_rodrigues(aa).view(M, J, 3, 3).float()
    a = torch.cat([R, torch.randn(M, J, 3, 1, generator=g) * 0.5], dim=3).reshape(M, J, 12).contiguous()
    w_idx, w_val = skinning_weights(g, V, J, K)
    C = regressor(g, n_rows, V)
    return dict(key=(M, V, J, K, n_rows, bool(use_gv), bool(use_gj), bool(want_transl), ld, seed), M=M, V=V, J=J, K=K, n_rows=n_rows,
                want_transl=bool(want_transl), ld=ld_of(V, ld), a=a, w_idx=w_idx, w_val=w_val, C=C, csrt=csr_transpose(C),
                v_posed=torch.randn(M, V, 3, generator=g) * 0.4,
                g_verts=torch.randn(M, V, 3, generator=g) if use_gv else None,
                g_joints=torch.randn(M, J + n_rows, 3, generator=g) if use_gj else None)


def one_mesh(c, m):
    """The M = 1 case of mesh m: the same model, that mesh's operands."""
    out = dict(c, M=1, key=c["key"] + ("mesh", m))
    for k in ("a", "v_posed", "g_verts", "g_joints"):
        out[k] = None if c[k] is None else c[k][m:m + 1].contiguous()
    return out


def dense_weights(c, dtype):
    W = torch.zeros(c["V"], c["J"], dtype=dtype)
    W.scatter_add_(1, c["w_idx"].long(), c["w_val"].to(dtype))
    return W


def lbs_backward(c, dtype, chunked=False, defect=None):
    """dict(g_vposed (M, V, 3), g_a (M, J, 12), g_transl (M, 3)) of the definition, as float64 tensors.  chunked: g_a and g_transl as
    per-128-vertex partial sums added in chunk order (g_transl: the chunk sums added in float64 and rounded once)."""
    M, V, J, K = c["M"], c["V"], c["J"], c["K"]
    W = dense_weights(c, dtype)
    Ct = c["C"].to(dtype).t().contiguous()                                             # (V, n_rows)
    if defect == "drop_third_regressor_entry":
        ptr, row, _ = c["csrt"]
        for v in torch.nonzero(ptr[1:] - ptr[:-1] >= 3).flatten().tolist():
            Ct[v, int(row[int(ptr[v]) + 2])] = 0
    a_all = c["a"].to(dtype)
    if defect == "second_group_uses_first_groups_transforms":
        gpb = lbs_launch_geometry(M, V)[1]
        a_all = a_all.clone()
        for m in range(M):
            if (m // GROUP) % gpb == 1:
                a_all[m] = c["a"][m - GROUP].to(dtype)
    idx = c["w_idx"].long()
    w = c["w_val"].to(dtype)
    n_chunks = _ceil_div(V, CHUNK)
    out = dict(g_vposed=torch.zeros(M, V, 3, dtype=torch.float64), g_a=torch.zeros(M, J, 12, dtype=torch.float64),
               g_transl=torch.zeros(M, 3, dtype=torch.float64))
    for m0 in range(0, M, GROUP):
        sl = slice(m0, min(M, m0 + GROUP))
        n = sl.stop - sl.start
        gv = torch.zeros(n, V, 3, dtype=dtype) if c["g_verts"] is None else c["g_verts"][sl].to(dtype)
        gj = None if c["g_joints"] is None else c["g_joints"][sl].to(dtype)
        if gj is not None and c["n_rows"]:
            gv = gv + torch.einsum("vr,mrc->mvc", Ct, gj[:, J:])
        T = torch.zeros(n, V, 12, dtype=dtype)
        for k in range(K):
            T = T + w[None, :, k, None] * a_all[sl][:, idx[:, k]]
        Rt = T.view(n, V, 3, 4)[..., :3].transpose(-1, -2)
        out["g_vposed"][sl] = (Rt @ gv[..., None])[..., 0].double()
        del T, Rt
        vp1 = torch.cat([c["v_posed"][sl].to(dtype), torch.ones(n, V, 1, dtype=dtype)], dim=2)
        outer = (gv[..., :, None] * vp1[..., None, :]).reshape(n, V, 12)
        Wa = W
        if defect == "drop_last_vertex_of_partial_chunk" and V % CHUNK:
            Wa = W.clone()
            Wa[V - 1] = 0
        gt = gv
        if defect == "transl_misses_one_ones_row":
            s = (torch.arange(V) % CHUNK) // 2
            gt = gv * (s % (32 - J) != 32 - J - 1).to(dtype)[None, :, None]
        if chunked:
            g_a = torch.zeros(n, J, 12, dtype=dtype)
            g_t = torch.zeros(n, 3, dtype=torch.float64)
            for ch in range(n_chunks):
                cs = slice(ch * CHUNK, min(V, (ch + 1) * CHUNK))
                g_a = g_a + torch.einsum("vj,mve->mje", Wa[cs], outer[:, cs])
                g_t = g_t + gt[:, cs].sum(1).double()
        else:
            g_a = torch.einsum("vj,mve->mje", Wa, outer)
            g_t = gt.sum(1).double()
        if gj is not None and defect != "kinematic_joints_missing_from_transl":
            g_t = g_t + (gj[:, :J].double().sum(1) if chunked else gj[:, :J].sum(1).double())
        out["g_a"][sl] = g_a.double()
        out["g_transl"][sl] = g_t.to(dtype).double()
    return out


def vposed_rows(c, g_vposed, before, defect=None):
    """The (M, ld) image of v_posed after the call: g_vposed, then zeros in [3 V, ld); ``before``: what lay in the padding."""
    rows = torch.full((c["M"], c["ld"]), 0.0 if defect != "padding_columns_not_zeroed" else float(before), dtype=torch.float64)
    rows[:, :3 * c["V"]] = g_vposed.reshape(c["M"], -1)
    return rows


@functools.lru_cache(maxsize=None)
def _lbs_reference(key):
    c = lbs_case(*key)
    r64, r32, rch = lbs_backward(c, torch.float64), lbs_backward(c, torch.float32), lbs_backward(c, torch.float32, chunked=True)
    return {k: (r64[k], r32[k], rch[k]) for k in r64}


def lbs_reference(c):
    """{g_vposed, g_a, g_transl: (y64, y_cpu32, y_chunk32)}, float64 tensors."""
    return _lbs_reference(c["key"])


def lbs_autograd(c):
    """The same three tensors by torch float64 autograd through mesh_scenario.skin plus the joint regression and the translation."""
    M, V, J = c["M"], c["V"], c["J"]
    a = c["a"].double().requires_grad_(True)
    vp = c["v_posed"].double().requires_grad_(True)
    tr = torch.zeros(M, 3, dtype=torch.float64, requires_grad=True)
    mc = dict(M=M, V=V, K=c["K"], a=a, w_val=c["w_val"], w_idx=c["w_idx"], transl=tr)
    verts = MS.skin(mc, vp, torch.float64)
    loss = 0.0
    if c["g_verts"] is not None:
        loss = loss + (c["g_verts"].double() * verts).sum()
    if c["g_joints"] is not None:
        # (the kinematic joints reach the translation only: their dependence on a belongs to hps_smpl_pose_prep_backward)
        joints = torch.cat([tr[:, None].expand(M, J, 3), torch.einsum("rv,mvc->mrc", c["C"].double(), verts)], dim=1)
        loss = loss + (c["g_joints"].double() * joints).sum()
    loss.backward()
    return dict(g_vposed=vp.grad, g_a=a.grad, g_transl=tr.grad)


# ---- hps_smpl_blend_backward ----
@functools.lru_cache(maxsize=None)
def blend_case(kp, np_, M, ld_extra, seed=0):
    g = torch.Generator().manual_seed(300007 * seed + 17 * kp + 1013 * np_ + 7 * M + ld_extra)
    rows, N = kp - 3, (np_ - 4) // 3 * 3
    bmat = torch.zeros(kp, np_)
    bmat[:rows, :N] = torch.randn(rows, N, generator=g) * 0.008
    gvp = torch.full((M, np_ + ld_extra), float("nan"))
    gvp[:, :np_] = torch.randn(M, np_, generator=g)
    return dict(key=(kp, np_, M, ld_extra, seed), kp=kp, np=np_, M=M, ld_g=np_ + ld_extra, rows=rows, N=N, mp=MS.padded_mesh_count(M),
                bmat=bmat, g_vposed=gvp)


def blend_backward(bc, dtype, sliced=False, defect=None):
    """g_xt[:, :M] (kp, M) as a float64 tensor; sliced: per-512-column partial sums added in slice order."""
    b, g = bc["bmat"].to(dtype), bc["g_vposed"][:, :bc["np"]].to(dtype)
    n_slices = _ceil_div(bc["np"], SLICE)
    if defect == "drop_last_slice" or sliced:
        out = torch.zeros(bc["kp"], bc["M"], dtype=dtype)
        for s in range(n_slices - (1 if defect == "drop_last_slice" else 0)):
            out = out + b[:, s * SLICE:(s + 1) * SLICE] @ g[:, s * SLICE:(s + 1) * SLICE].t()
    else:
        out = b @ g.t()
    if defect == "drop_rows_behind_224":
        out = out.clone()
        out[ROW_TILE:] = 0
    return out.double()


@functools.lru_cache(maxsize=None)
def _blend_reference(key):
    bc = blend_case(*key)
    return blend_backward(bc, torch.float64), blend_backward(bc, torch.float32), blend_backward(bc, torch.float32, sliced=True)


def blend_reference(bc):
    """(y64, y_cpu32, y_slice32) of g_xt[:, :M]."""
    return _blend_reference(bc["key"])


# ---- hps_smpl_pose_prep_backward ----
def tree(name):
    return tuple(HF.tree("smpl")) if name == "smpl" else TREES[name]


def depth_of(parents):
    d = []
    for i, p in enumerate(parents):
        assert p < i
        d.append(0 if p < 0 else d[p] + 1)
    return d


def _rotation_vectors(g, M, J, zero_mesh):
    aa = torch.randn(M, J, 3, generator=g, dtype=torch.float64) * 0.4
    if zero_mesh is not None:
        aa[zero_mesh] = 0.0
    return aa


@functools.lru_cache(maxsize=None)
def pose_case(tree_name, nb, M, rotmat, n_rows, seed=0):
    parents = tree(tree_name)
    J = len(parents)
    g = torch.Generator().manual_seed(400009 * seed + 131 * J + 17 * nb + 1013 * M + 2 * int(rotmat) + 7 * n_rows + sum(parents))
    zero_mesh = M // 2 if (M > 1 and not rotmat) else None
    aa = _rotation_vectors(g, M, J, zero_mesh)
    if rotmat:
        R = O.batch_rodrigues(aa.reshape(-1, 3)).view(M, J, 9).float()
        glob, body = R[:, 0].contiguous(), R[:, 1:].reshape(M, 9 * (J - 1)).contiguous()
    else:
        glob, body = aa[:, 0].float().contiguous(), aa[:, 1:].reshape(M, 3 * (J - 1)).float().contiguous()
    rows = nb + 9 * (J - 1)
    kp, mp = max(16, _round_up(rows, 16)), MS.padded_mesh_count(M)
    return dict(key=(tree_name, nb, M, bool(rotmat), n_rows, seed), tree=tree_name, parents=parents, depth=depth_of(parents), J=J, nb=nb, M=M,
                rotmat=bool(rotmat), n_rows=n_rows, rows=rows, kp=kp, mp=mp, zero_mesh=zero_mesh, glob=glob, body=body,
                betas=torch.randn(M, nb, generator=g), j_template=torch.randn(J, 3, generator=g) * 0.3,
                j_shapedirs=(torch.randn(J, 3, nb, generator=g) * 0.05).contiguous(), g_a=torch.randn(M, J, 12, generator=g),
                g_joints=torch.randn(M, J + n_rows, 3, generator=g), g_xt=torch.randn(kp, mp, generator=g))


def one_pose(pc, m):
    """The M = 1 case of mesh m (g_xt keeps its pitch: column 0 is the mesh's)."""
    out = dict(pc, M=1, key=pc["key"] + ("mesh", m), zero_mesh=0 if pc["zero_mesh"] == m else None)
    for k in ("glob", "body", "betas", "g_a", "g_joints"):
        out[k] = pc[k][m:m + 1].contiguous()
    g_xt = torch.zeros(pc["kp"], MS.padded_mesh_count(1))
    g_xt[:, 0] = pc["g_xt"][:, m]
    out.update(g_xt=g_xt, mp=g_xt.shape[1])
    return out


def _rodrigues_of(d, angle):
    """batch_rodrigues from the direction and the angle (the defect's route: angle = ||r||, without the + 1e-8)."""
    n = d.shape[0]
    rx, ry, rz = torch.split(d, 1, dim=1)
    z = torch.zeros((n, 1), dtype=d.dtype)
    K = torch.cat([z, -rz, ry, rz, z, -rx, -ry, rx, z], dim=1).view(n, 3, 3)
    return torch.eye(3, dtype=d.dtype)[None] + torch.sin(angle)[..., None] * K + (1 - torch.cos(angle))[..., None] * torch.bmm(K, K)


def _rigid_transform_with_cut(R, joints, parents, cut):
    """oracle.ref_cpu._rigid_transform with the world transform of ``cut``'s parent detached on the way to ``cut``."""
    M, J = joints.shape[:2]
    rel = joints.clone()
    rel[:, 1:] = rel[:, 1:] - joints[:, list(parents[1:])]
    L = torch.cat([R, rel[..., None]], dim=3)                                           # (M, J, 3, 4)
    bottom = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=R.dtype).expand(M, J, 1, 4)
    L = torch.cat([L, bottom], dim=2)
    chain = [L[:, 0]]
    for i in range(1, J):
        P = chain[parents[i]]
        chain.append(torch.matmul(P.detach() if i == cut else P, L[:, i]))
    G = torch.stack(chain, dim=1)
    posed = G[:, :, :3, 3]
    A = G.clone()
    A[:, :, :3, 3] = G[:, :, :3, 3] - (G[:, :, :3, :3] @ joints[..., None])[..., 0]
    return posed, A


def pose_prep(pc, dtype, glob, body, betas, defect=None):
    """hps_smpl_pose_prep's outputs restated: (xt (rows, M), a (M, J, 12), j_posed (M, J, 3))."""
    M, J, nb, parents = pc["M"], pc["J"], pc["nb"], pc["parents"]
    if pc["rotmat"]:
        R = torch.cat([glob.view(M, 1, 3, 3), body.view(M, J - 1, 3, 3)], dim=1) if J > 1 else glob.view(M, 1, 3, 3)
    else:
        aa = torch.cat([glob.view(M, 1, 3), body.view(M, J - 1, 3)], dim=1) if J > 1 else glob.view(M, 1, 3)
        if defect == "rodrigues_without_epsilon":
            angle = torch.norm(aa.reshape(-1, 3), dim=1, keepdim=True)
            R = _rodrigues_of(aa.reshape(-1, 3) / angle, angle).view(M, J, 3, 3)
        else:
            R = O.batch_rodrigues(aa.reshape(-1, 3)).view(M, J, 3, 3)
    shaped = torch.einsum("jcl,ml->mjc", pc["j_shapedirs"].to(dtype), betas)
    joints = pc["j_template"].to(dtype)[None] + (shaped.detach() if defect == "betas_without_joint_term" else shaped)
    if defect == "star_root_misses_last_child":
        posed, A = _rigid_transform_with_cut(R, joints, parents, J - 1)
    else:
        posed, A = O._rigid_transform(R, joints, torch.tensor(parents, dtype=torch.long))
    a = A[:, :, :3, :].reshape(M, J, 12)
    feat = (R[:, 1:] - torch.eye(3, dtype=dtype)).reshape(M, 9 * (J - 1))
    return torch.cat([betas, feat], dim=1).t(), a, posed


def pose_leaves(pc, dtype):
    return {k: pc[k].detach().clone().to(dtype).requires_grad_(True) for k in ("glob", "body", "betas")}


def pose_prep_backward(pc, dtype, use_gj=True, use_gxt=True, defect=None):
    """dict(g_glob, g_body, g_betas) shaped like the inputs, float64 tensors: autograd of the loss of the module docstring."""
    x = pose_leaves(pc, dtype)
    xt, a, posed = pose_prep(pc, dtype, x["glob"], x["body"], x["betas"], defect)
    loss = (pc["g_a"].to(dtype) * a).sum()
    if use_gj:
        loss = loss + (pc["g_joints"][:, :pc["J"]].to(dtype) * posed).sum()
    if use_gxt:
        loss = loss + (pc["g_xt"][:pc["rows"], :pc["M"]].to(dtype) * xt).sum()
    loss.backward()
    return {"g_" + k: (torch.zeros_like(v) if v.grad is None else v.grad).double() for k, v in x.items()}


@functools.lru_cache(maxsize=None)
def _pose_reference(key, use_gj, use_gxt):
    pc = pose_case(*key[:6])
    if len(key) > 6:
        pc = one_pose(pc, key[7])
    r64, r32 = pose_prep_backward(pc, torch.float64, use_gj, use_gxt), pose_prep_backward(pc, torch.float32, use_gj, use_gxt)
    return {k: (r64[k], r32[k]) for k in r64}


def pose_reference(pc, use_gj=True, use_gxt=True):
    """{g_glob, g_body, g_betas: (y64, y_cpu32)}, float64 tensors (g_body of a single joint and g_betas without coefficients are empty)."""
    return _pose_reference(pc["key"], bool(use_gj), bool(use_gxt))


# ---- the chained case ----
@functools.lru_cache(maxsize=None)
def chained_case():
    """Operands of hps_smpl_pose_prep -> hps_smpl_blend -> the three backward calls as SMPL._backward strings them, on CHAINED's shape."""
    k = CHAINED
    pc = pose_case(k["tree"], k["nb"], k["M"], False, k["n_rows"], seed=1)
    M, V, J = k["M"], k["V"], pc["J"]
    g = torch.Generator().manual_seed(9176)
    w_idx, w_val = skinning_weights(g, V, J, k["K"])
    C = regressor(g, k["n_rows"], V)
    bmat = torch.zeros(pc["kp"], _round_up(3 * V, 128))
    bmat[:pc["rows"], :3 * V] = torch.randn(pc["rows"], 3 * V, generator=g) * 0.008
    return dict(pose=pc, M=M, V=V, J=J, K=k["K"], n_rows=k["n_rows"], w_idx=w_idx, w_val=w_val, C=C, csrt=csr_transpose(C), bmat=bmat,
                np=bmat.shape[1], v_template=torch.randn(V, 3, generator=g) * 0.4, transl=torch.randn(M, 3, generator=g),
                g_verts=torch.randn(M, V, 3, generator=g), g_joints=torch.randn(M, J + k["n_rows"], 3, generator=g))


def chained_forward(cc, dtype, glob, body, betas, transl):
    """(vertices (M, V, 3), joints (M, J + n_rows, 3)) of the composite."""
    pc, M, V = cc["pose"], cc["M"], cc["V"]
    xt, a, posed = pose_prep(pc, dtype, glob, body, betas)
    v_posed = cc["v_template"].to(dtype)[None] + (xt.t() @ cc["bmat"][:pc["rows"], :3 * V].to(dtype)).view(M, V, 3)
    mc = dict(M=M, V=V, K=cc["K"], a=a, w_val=cc["w_val"], w_idx=cc["w_idx"], transl=transl)
    verts = MS.skin(mc, v_posed, dtype)
    joints = torch.cat([posed + transl[:, None], torch.einsum("rv,mvc->mrc", cc["C"].to(dtype), verts)], dim=1)
    return verts, joints


@functools.lru_cache(maxsize=None)
def chained_reference():
    """{glob, body, betas, transl: (g64, g_cpu32)} of <g_verts, vertices> + <g_joints, joints>."""
    cc, out = chained_case(), {}
    for dtype in (torch.float64, torch.float32):
        x = pose_leaves(cc["pose"], dtype)
        x["transl"] = cc["transl"].to(dtype).requires_grad_(True)
        verts, joints = chained_forward(cc, dtype, x["glob"], x["body"], x["betas"], x["transl"])
        ((cc["g_verts"].to(dtype) * verts).sum() + (cc["g_joints"].to(dtype) * joints).sum()).backward()
        for k, v in x.items():
            out.setdefault(k, []).append(v.grad.double())
    return {k: tuple(v) for k, v in out.items()}
