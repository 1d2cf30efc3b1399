"""Seeded cases, CPU references and the accuracy rule of the SMPL mesh-kernel tests (tests/test_mesh_scenario_host.py,
tests/test_gpu_mesh_shapes.py).  Nothing here touches a device.

A case is built at the level of the C ABI (include/hps.h), so the vertex count V, the number of data rows of the blend operands, the
joint count J and the number of skinning weights per vertex K are free (the SMPL class ties V to its 6890-column joint regressors):

    xt          (kp16, mp)   rows [0, min(10, rows)) N(0, 1) ("betas"), the other data rows N(0, 0.3) ("pose feature"), the rows behind
                             ``rows`` zero; kp16 = rows rounded up to 16, mp = HPS_WS_SMPL_MP(M).  The padding columns m >= M hold NaN
                             on the data rows: hps_smpl_pose_prep writes the columns below M only and SMPL.forward allocates the
                             operand with torch.empty, so anything may lie there -- and a mesh is a ROW of the MFMA result, so no live
                             mesh may see it.
    bmat        (kp16, 3 V)  N(0, 0.008), rows behind ``rows`` zero; its two device layouts are blend_matrix() (the 128-padded one of
                             hps_smpl_blend) and panel_permuted() (bmat_p of hps_smpl_mesh_fused)
    v_template  (V, 3)       N(0, 0.4)
    a           (M, J, 12)   [R | t], R = Rodrigues of N(0, 0.5) axis-angles, t = N(0, 0.5)
    w_idx/w_val (V, K)       1..K non-zero weights per vertex on distinct joints, normalised to sum 1, padded with (0, 0.0f); vertex 0
                             and vertex V - 1 have a single influence of weight 1
    transl      (M, 3)       N(0, 1), or None

shared(c, R) adds what the shared-shape entry points take: R shaped templates (R, V, 3) and the mesh_row / group_rows tables, whose
groups of 32 meshes cycle through split = 31, -1, 1, 32 | 0, 31, 1, 32 -- so the first tile (64 meshes, or 128 in the bf16x3 kernel)
holds a split < 0 group beside ordinary ones and takes the per-mesh fetch, and the second 128 meshes take the two-row select.

The truth is y64, the definition of include/hps.h in float64 (einsum, skinning, translation).  The family of legitimate fp32
evaluations it is compared with:

    y_cpu32    the same in torch fp32
    y_pair32   fp32 with the products of the blend accumulated k-pair by k-pair, ascending, from zero, the template added last: the
               order of the kernels' MFMA chain

and likewise v_posed (vp64, vp_cpu32, vp_pair32) for the blend alone.  The accuracy rule is smpl_grad_scenario.bound with the family
widened as in conv_scenario (the factor 4 is the project's margin for a summation order other than the reference's), per output tensor:

    bound = 4 * max(e_cpu32, e_pair32, 2**-23 * max|y64|)        e_* = max|y_* - y64|

References are computed once per case and shared: callers must not modify them.
"""
import functools

import torch

from hierarchicalprobabilistic3dhuman_amd import _capi
from oracle import ref_cpu as O

EPS32 = 2.0 ** -23
PANEL = 64                # vertices per panel of bmat_p
SPLITS = (31, -1, 1, 32, 0, 31, 1, 32)

# ---- the GPU cases (tests/test_gpu_mesh_shapes.py); the host test holds every reference of every one of them to the rule ----
# (a) hps_smpl_mesh_fused, K = 4: (M, V, kp, J, transl).  V: one vertex, less than / exactly / just over one 32-vertex wave group and
# one 64-vertex panel, ragged second and third panels; kp: every tail 1..8 of the last 16-row chunk with 1, 2 and 14 chunks; M: ragged
# tiles, and nine tiles (520), where the XCD-aware grid has seven padding blocks; a compile-time (24) and a run-time (7, 22) joint count.
FUSED_CASES = [
    (1, 1, 2, 24, False), (64, 31, 14, 24, True), (65, 32, 16, 24, False), (130, 33, 18, 24, True), (65, 63, 32, 7, False),
    (64, 64, 208, 24, False), (130, 65, 210, 24, True), (1, 127, 212, 22, True), (65, 129, 214, 24, False), (130, 200, 216, 24, True),
    (65, 200, 218, 24, False), (130, 65, 218, 24, True), (64, 33, 220, 7, True), (130, 64, 222, 24, False), (65, 129, 224, 22, False),
    (520, 65, 218, 24, False), (520, 33, 16, 24, True), (1, 64, 18, 24, True), (130, 1, 224, 24, False), (64, 127, 2, 22, False),
    (520, 200, 212, 7, True),
]
# (b) K = 8 and 12 with 24 joints, fused: (M, V, kp, K, transl)
FUSED_WIDE_CASES = [(65, 65, 218, 8, False), (130, 200, 210, 12, True), (64, 200, 16, 8, True), (1, 65, 224, 12, False)]
# (b) hps_smpl_blend + hps_smpl_lbs with K = 8, 12, 24 on both sides of the 256-vertex tile of the LBS kernel: (M, V, kp, K, transl)
LBS_CASES = [(9, 1, 16, 8, False), (70, 200, 32, 12, True), (9, 257, 218, 24, False), (70, 300, 16, 8, True), (9, 300, 32, 12, False),
             (70, 1, 16, 24, True), (9, 200, 16, 24, False), (70, 257, 224, 8, True), (9, 257, 16, 12, True)]
# (c) hps_smpl_mesh_fused_picks (TAIL = 5): (M, V, kp, transl); M <= 128: the four-stage K loop (1, 2 and 14 chunks), 130: two stages
PICKS_CASES = [(1, 65, 10, False), (52, 200, 26, True), (128, 65, 218, False), (130, 200, 218, True), (128, 200, 10, True),
               (130, 65, 26, False), (52, 65, 218, False)]
# (d) hps_smpl_mesh_fused_shared_shape (TAIL = 8): (M, V, kp); M <= 128: four stages
SHARED_CASES = [(40, 33, 16), (128, 64, 32), (200, 200, 208), (40, 200, 208), (128, 33, 208), (200, 64, 16)]
SHARED_R = 3
# hps_smpl_v_shaped: (R, num_betas, V)
V_SHAPED_CASES = [(1, 0, 33), (3, 1, 64), (1, 10, 200), (3, 16, 257), (3, 0, 1), (1, 16, 65)]
# (e) hps_smpl_split_bf16x3 + hps_smpl_mesh_fused_shared_shape_bf16x3: (M, V, rows, R).  R = 3: the shared-shape tables (the fp32-MFMA
# form of the case is hps_smpl_mesh_fused_shared_shape, which exists where kp is a multiple of 16); R = 1: one template row for all
# meshes, "what SMPL.forward does" without shared shapes (the fp32-MFMA form is hps_smpl_mesh_fused)
SPLIT_CASES = [(1, 33, 1, 1), (128, 64, 15, 3), (129, 200, 16, 3), (300, 33, 17, 1), (129, 64, 207, 3), (300, 200, 217, 1), (128, 200, 207, 3),
               (1, 64, 217, 1)]
# (f) module level
MODULE_NUM_BETAS = (1, 2, 5, 9, 11, 16)


def _round_up(x, m):
    return (x + m - 1) // m * m


def padded_mesh_count(M):
    """mp of the blend operand: HPS_WS_SMPL_MP."""
    return _capi.query_workspace(_capi.WS_SMPL_MP, M)


@functools.lru_cache(maxsize=None)
def case(M, V, rows, J=24, K=4, transl=False, seed=0):
    """fp32 CPU operands of one call (see the module docstring)."""
    assert 1 <= K <= J
    g = torch.Generator().manual_seed(100003 * seed + 7919 * M + 104729 * V + 31 * rows + 1009 * J + 13 * K + int(transl))
    kp16, mp = _round_up(rows, 16), padded_mesh_count(M)
    nb = min(10, rows)
    xt = torch.zeros(kp16, mp)
    xt[:nb, :M] = torch.randn(nb, M, generator=g)
    xt[nb:rows, :M] = torch.randn(rows - nb, M, generator=g) * 0.3
    xt[:rows, M:] = float("nan")
    bmat = torch.zeros(kp16, 3 * V)
    bmat[:rows] = torch.randn(rows, 3 * V, generator=g) * 0.008
    v_template = torch.randn(V, 3, generator=g) * 0.4
    aa = torch.randn(M * J, 3, generator=g, dtype=torch.float64) * 0.5
    R = O.batch_rodrigues(aa).view(M, J, 3, 3).float()
    t = torch.randn(M, J, 3, 1, generator=g) * 0.5
    a = torch.cat([R, t], dim=3).reshape(M, J, 12).contiguous()
    nnz = torch.randint(1, K + 1, (V,), generator=g)
    nnz[0] = nnz[V - 1] = 1
    joints = torch.argsort(torch.rand(V, J, generator=g), dim=1)[:, :K]               # K distinct joints per vertex
    live = torch.arange(K)[None] < nnz[:, None]
    w = (torch.rand(V, K, generator=g, dtype=torch.float64) * 0.9 + 0.1) * live
    w_val = (w / w.sum(1, keepdim=True)).float().contiguous()
    w_idx = torch.where(live, joints, torch.zeros_like(joints)).to(torch.int32).contiguous()
    tr = torch.randn(M, 3, generator=g) if transl else None
    return dict(key=(M, V, rows, J, K, bool(transl), seed), M=M, V=V, rows=rows, J=J, K=K, kp=_round_up(rows, 2), kp16=kp16, mp=mp, xt=xt,
                bmat=bmat, v_template=v_template, a=a, w_idx=w_idx, w_val=w_val, transl=tr)


# ---- device layouts of the blend matrix ----
def blend_matrix(c):
    """bmat of hps_smpl_blend: (kp16, np), np = 3 V rounded up to 128, zero padded."""
    out = torch.zeros(c["kp16"], _round_up(3 * c["V"], 128))
    out[:, :3 * c["V"]] = c["bmat"]
    return out


def _panel_columns(V):
    v = torch.arange(V)
    return torch.stack([(v // PANEL) * 3 * PANEL + ch * PANEL + v % PANEL for ch in range(3)], dim=1).reshape(-1)      # column of n = 3 v + ch


def panel_permuted(bmat, V):
    """bmat_p of include/hps.h: col(v, c) = (v / 64) * 192 + c * 64 + v % 64, unused columns zero."""
    out = torch.zeros(bmat.shape[0], -(-V // PANEL) * 3 * PANEL, dtype=bmat.dtype)
    out[:, _panel_columns(V)] = bmat[:, :3 * V]
    return out


def panel_unpermuted(bmat_p, V):
    return bmat_p[:, _panel_columns(V)]


# ---- shared shapes ----
@functools.lru_cache(maxsize=None)
def _shared(key, R):
    c = case(*key)
    M, V, mp = c["M"], c["V"], c["mp"]
    g = torch.Generator().manual_seed(977 + 31 * M + V + 1000 * R)
    v_shaped = (c["v_template"][None] + torch.randn(R, V, 3, generator=g) * 0.05).contiguous()
    mesh_row = torch.zeros(mp, dtype=torch.int32)
    groups = torch.zeros(mp // 32, 3, dtype=torch.int32)
    for gi in range(mp // 32):
        split = SPLITS[gi % len(SPLITS)] if R > 1 else 32
        ra = gi % R
        rb = (ra + 1) % R
        if split < 0:
            rows = torch.randint(0, R, (32,), generator=g, dtype=torch.int32)
            rows[:4] = torch.tensor([ra, rb, ra, rb], dtype=torch.int32)              # (more than one change, whatever the draw)
        else:
            rows = torch.full((32,), rb, dtype=torch.int32)
            rows[:split] = ra
        mesh_row[32 * gi:32 * gi + 32] = rows
        groups[gi] = torch.tensor([ra, rb, split], dtype=torch.int32)
    return dict(R=R, v_shaped=v_shaped, mesh_row=mesh_row, group_rows=groups.reshape(-1).contiguous())


def shared(c, R=SHARED_R):
    """R shaped templates and the mesh_row (mp,) / group_rows (mp / 32 * 3,) tables of the shared-shape entry points."""
    return _shared(c["key"], R)


def every_group_fetches_per_mesh(group_rows):
    """The same table with split = -1 in every group (hps.h: mesh_row is authoritative, so any group may say -1)."""
    gr = group_rows.view(-1, 3).clone()
    gr[:, 2] = -1
    return gr.reshape(-1).contiguous()


# ---- the definition, in any dtype and either order ----
DEFECTS = ("drop_last_pair", "neighbour_weights", "previous_mesh_transforms", "swap_yz", "no_translation_on_last", "row_a_at_split")


def blend(c, dtype, pair=False, sh=None, defect=None):
    """v_posed (M, V, 3) = template + sum_k xt[k, m] bmat[k, 3 v + c]; pair: accumulated k-pair by k-pair, ascending, from zero."""
    M, V, rows = c["M"], c["V"], c["rows"]
    x, b = c["xt"][:rows, :M].to(dtype), c["bmat"][:rows].to(dtype)
    if defect == "drop_last_pair":
        x = x.clone()
        x[2 * ((rows - 1) // 2):, M // 2] = 0
    if pair:
        acc = torch.zeros(M, 3 * V, dtype=dtype)
        for k in range(0, rows, 2):
            acc = acc + x[k:k + 2].T @ b[k:k + 2]
    else:
        acc = torch.einsum("km,kn->mn", x, b)
    if sh is None:
        base = c["v_template"].to(dtype)[None]
    else:
        rows_of = sh["mesh_row"][:M].long().clone()
        if defect == "row_a_at_split":
            gr = sh["group_rows"].view(-1, 3)
            gi = next(i for i in range(gr.shape[0]) if 0 < int(gr[i, 2]) < 32 and 32 * i + int(gr[i, 2]) < M)
            rows_of[32 * gi + int(gr[gi, 2])] = int(gr[gi, 0])
        base = sh["v_shaped"].to(dtype)[rows_of]
    return base + acc.view(M, V, 3)


def skin(c, v_posed, dtype, defect=None):
    """verts[m, v] = (sum_k w[v, k] A[m, idx[v, k]]) [v_posed[m, v]; 1] (+ transl[m])"""
    M, V, K = c["M"], c["V"], c["K"]
    a, w, idx = c["a"].to(dtype), c["w_val"].to(dtype), c["w_idx"].long()
    if defect == "neighbour_weights":
        w, idx = w.clone(), idx.clone()
        w[V - 1], idx[V - 1] = w[V - 2], idx[V - 2]
    if defect == "previous_mesh_transforms":
        a = a.clone()
        a[M - 1] = a[M - 2]
    T = torch.zeros(M, V, 12, dtype=dtype)
    for k in range(K):
        T = T + w[None, :, k, None] * a[:, idx[:, k]]
    T = T.view(M, V, 3, 4)
    out = (T[..., :3] @ v_posed.to(dtype)[..., None])[..., 0] + T[..., 3]
    if c["transl"] is not None:
        tr = c["transl"].to(dtype).clone()
        if defect == "no_translation_on_last":
            tr[M - 1] = 0
        out = out + tr[:, None]
    if defect == "swap_yz":
        out = out.clone()
        m, v = M // 2, V // 2
        out[m, v, 1], out[m, v, 2] = out[m, v, 2].clone(), out[m, v, 1].clone()
    return out


def forward(c, dtype, pair=False, sh=None, defect=None):
    """(verts, v_posed) of the definition as float64 tensors."""
    vp = blend(c, dtype, pair, sh, defect)
    return skin(c, vp, dtype, defect).double(), vp.double()


@functools.lru_cache(maxsize=None)
def _reference(key, R):
    c = case(*key)
    sh = None if R is None else shared(c, R)
    out = {}
    for name, dtype, pair in (("64", torch.float64, False), ("_cpu32", torch.float32, False), ("_pair32", torch.float32, True)):
        out["y" + name], out["vp" + name] = forward(c, dtype, pair, sh)
    return out


def reference(c, R=None):
    """dict(y64, y_cpu32, y_pair32, vp64, vp_cpu32, vp_pair32), float64 tensors (M, V, 3); R: with the case's R shaped templates."""
    return _reference(c["key"], R)


# ---- the rule ----
def bound(y64, *family):
    return 4.0 * max([float((y - y64).abs().max()) for y in family] + [EPS32 * float(y64.abs().max())])


def check(name, y_dev, y64, *family):
    """Prints the figures, then asserts the accuracy rule for one output tensor; returns err / (2^-23 max|y64|)."""
    err = float((y_dev.detach().cpu().double().reshape(y64.shape) - y64).abs().max())
    unit = EPS32 * float(y64.abs().max())
    b = bound(y64, *family)
    print("%-34s max|dev - f64| = %.3e  max|y64| = %.3e  dev/(2^-23 max|y64|) = %.2f  references/(..) = %s  bound/(..) = %.2f"
          % (name, err, unit / EPS32, err / unit, " ".join("%.2f" % (float((y - y64).abs().max()) / unit) for y in family), b / unit))
    assert err <= b, (name, err, b)
    return err / unit


def check_case(name, ref, y_dev=None, vp_dev=None):
    """check() of the vertices and / or of v_posed against the three references of a case."""
    out = []
    if y_dev is not None:
        out.append(check(name + " verts", y_dev, ref["y64"], ref["y_cpu32"], ref["y_pair32"]))
    if vp_dev is not None:
        out.append(check(name + " v_posed", vp_dev, ref["vp64"], ref["vp_cpu32"], ref["vp_pair32"]))
    return max(out)


# ---- hps_smpl_v_shaped ----
@functools.lru_cache(maxsize=None)
def v_shaped_case(R, nb, V):
    """betas (R, nb) N(0, 1), shape_rows (nb, ld) N(0, 0.012) with ld = 3 V rounded up to 128, v_template (3 V,) N(0, 0.4) and the three
    references of v_shaped[r, n] = v_template[n] + sum_l betas[r, l] shape_rows[l, n] (float64; fp32 einsum; fp32 chain over l, ascending)."""
    g = torch.Generator().manual_seed(5 + 100 * R + 10 * nb + 1000 * V)
    ld = _round_up(3 * V, 128)
    betas = torch.randn(R, nb, generator=g)
    shape_rows = torch.randn(nb, ld, generator=g) * 0.012
    vt = torch.randn(3 * V, generator=g) * 0.4
    s = shape_rows[:, :3 * V]
    y64 = vt.double()[None] + betas.double() @ s.double()
    y_cpu32 = (vt[None] + betas @ s).double()
    acc = torch.zeros(R, 3 * V)
    for l in range(nb):
        acc = acc + betas[:, l, None] * s[l][None]
    y_seq32 = (vt[None] + acc).double()
    return dict(R=R, nb=nb, V=V, ld=ld, betas=betas, shape_rows=shape_rows, v_template=vt, y64=y64, y_cpu32=y_cpu32, y_seq32=y_seq32)


def all_cases():
    """(name, case, R) of every GPU case whose references the host test holds to the rule."""
    out = []
    for M, V, kp, J, tr in FUSED_CASES:
        out.append(("fused", case(M, V, kp, J, 4, tr), None))
    for M, V, kp, K, tr in FUSED_WIDE_CASES:
        out.append(("fused_wide", case(M, V, kp, 24, K, tr), None))
    for M, V, kp, K, tr in LBS_CASES:
        out.append(("lbs", case(M, V, kp, 24, K, tr), None))
    for M, V, kp, tr in PICKS_CASES:
        out.append(("picks", case(M, V, kp, 24, 4, tr), None))
    for M, V, kp in SHARED_CASES:
        out.append(("shared", case(M, V, kp, 24, 4, False), SHARED_R))
    for M, V, rows, R in SPLIT_CASES:
        out.append(("bf16x3", case(M, V, rows, 24, 4, False), R))
    return out
