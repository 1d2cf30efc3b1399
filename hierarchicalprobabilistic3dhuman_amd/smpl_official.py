"""``SMPL`` with the call surface of the reference's models/smpl_official.py (a thin subclass of
smplx.SMPL that appends 9 + 19 + 17 regressed joints -> 90), executed by hand-written gfx950 kernels.

    smpl = SMPL(model_path, batch_size=1, gender='neutral', num_betas=10).to(device)
    out = smpl(body_pose=(M,23,3,3), global_orient=(M,1,3,3), betas=(M,10), pose2rot=False)
    out.vertices (M,6890,3), out.joints (M,90,3)

Kernel sequence per call (all on the current HIP stream, no host synchronisation):
  hps_smpl_pose_prep  Rodrigues, rest joints, forward kinematics, blend-GEMM operand
  hps_smpl_mesh_fused v_template + [betas | pose feature] @ [shapedirs ; posedirs] (fp32 MFMA) skinned in the GEMM
                      epilogue: v_posed never exists in HBM.  ``fused_mesh = False`` selects the unfused pair
                      hps_smpl_blend + hps_smpl_lbs (bit-identical vertices; the definition SURVEY 8(d)'s LBS bytes use)
  hps_smpl_joints     24 kinematic joints + 21 vertex picks + 45 regressed joints

Under autograd (grad mode on and betas / body_pose / global_orient / transl requiring grad) the same kernels run inside a
torch.autograd.Function whose backward is three more (hps_smpl_lbs_backward, hps_smpl_blend_backward,
hps_smpl_pose_prep_backward): see ``SMPL.forward``.
"""
from collections import namedtuple

import numpy as np
import torch
from torch import nn

from . import _capi
from .device_state import DeviceStateModule
from .configs import SMPLX_EXTRA_VERTEX_IDS
from .smpl_data import resolve_smpl_model, load_extra_joint_regressors, parents_from_kintree

SMPLOutput = namedtuple("SMPLOutput", ["vertices", "joints", "full_pose", "betas", "global_orient", "body_pose"])
SMPLOutput.__new__.__defaults__ = (None,) * 6

_LBS_K_CHOICES = (4, 8, 12, 24)


def _round_up(x, m):
    return (x + m - 1) // m * m


class _SMPLFunction(torch.autograd.Function):
    """SMPL.forward for autograd: forward = the module's own kernel sequence (K = 217 forms), backward = the three device backward
    stages on what hps_smpl_pose_prep + hps_smpl_blend recompute from the saved INPUTS (nothing else is kept: 83 KB of transient
    v_posed per mesh in the backward instead of 83 KB per mesh held from forward to backward)."""

    @staticmethod
    def forward(ctx, smpl, pose2rot, g, b, be, tr):
        out = smpl.forward(betas=be, body_pose=b, global_orient=g, transl=tr, pose2rot=pose2rot, _k217=True)
        ctx.smpl, ctx.pose2rot = smpl, pose2rot
        ctx.save_for_backward(g, b, be)
        ctx.set_materialize_grads(False)
        return out.vertices, out.joints

    @staticmethod
    def backward(ctx, g_verts, g_joints):
        g, b, be = ctx.saved_tensors
        grads = ctx.smpl._backward(g, b, be, ctx.pose2rot, g_verts, g_joints, ctx.needs_input_grad[2:6])
        return (None, None) + grads


class SMPL(DeviceStateModule):
    """models/smpl_official.py:12-41.  ``model_path``: directory holding SMPL_<GENDER>.pkl, a pkl path,
    or a dict of arrays (e.g. ``smpl_data.synthetic_smpl_model()``).  ``model_files_dir`` may point at the
    reference's model_files/ (extra joint regressors); the packaged copies are used otherwise."""

    SWITCHES = ("fused_mesh", "picked_joints", "shared_shape", "mesh_arith", "pad_v_posed")
    NUM_JOINTS = 24
    NUM_BODY_JOINTS = 23

    def __init__(self, model_path, batch_size=1, gender="neutral", num_betas=10, model_files_dir=None,
                 dtype=torch.float32, **kwargs):
        super().__init__()
        if dtype != torch.float32:
            raise ValueError("the gfx950 kernels compute in fp32 (the reference never changes dtype)")
        if int(num_betas) < 1:
            # include/hps.h documents 0..16 rows of betas at the C ABI; a module with NO shape coefficients would hand the library the
            # null pointer of its empty (M, 0) betas tensor, which every entry point refuses -- say so here instead
            raise ValueError("num_betas must be at least 1, got %r: this module has no form without shape coefficients (its empty betas "
                             "tensor has no device pointer to give the library); pass zero betas instead" % (num_betas,))
        model = resolve_smpl_model(model_path, gender=gender, num_betas=num_betas)
        self.gender = gender
        self.batch_size = batch_size
        self.num_betas = num_betas
        self.dtype = dtype
        self.keep_intermediates = False
        self.lbs_events = None
        self.pad_v_posed = True
        self.fused_mesh = True
        # meshes that share their shape (infer(use_mean_shape=True): every mesh of an image has the image's betas) take the K = 207 form of
        # the fused kernel (hps_smpl_mesh_fused_shared_shape: the shape blend once per image, not once per mesh).  False: the K = 217 form
        # for every call (the bit-level partner of the unfused pair).
        self.shared_shape = True
        # arithmetic of the shared-shape form's pose blend GEMM.  "f32": v_mfma_f32_32x32x2_f32, the reference's own arithmetic type in every
        # instruction (default).  "bf16x3": every fp32 operand as three bf16 pieces, six exact piece products per product on the bf16 matrix
        # pipe, fp32 accumulation -- fp32 accuracy (as close to the float64 twin as "f32"), not the same bits (include/hps.h:
        # hps_smpl_mesh_fused_shared_shape_bf16x3).  Applies where the shared-shape form applies; every other call is "f32".
        self.mesh_arith = "f32"

        f32 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32)
        v_template = np.asarray(model["v_template"], np.float64)
        shapedirs = np.asarray(model["shapedirs"], np.float64)[:, :, :num_betas]
        posedirs_v3k = np.asarray(model["posedirs"], np.float64)                  # (V,3,207)
        J_regressor = np.asarray(model["J_regressor"], np.float64)
        weights = np.asarray(model["weights"], np.float64)
        parents = parents_from_kintree(model["kintree_table"])
        V, J = v_template.shape[0], J_regressor.shape[0]
        self.num_verts = V

        # ---- buffers with smplx's names / layouts (what a user of the reference can inspect) ----
        self.register_buffer("v_template", f32(v_template))
        self.register_buffer("shapedirs", f32(shapedirs))
        self.register_buffer("posedirs", f32(posedirs_v3k.reshape(-1, posedirs_v3k.shape[-1]).T))   # (207,3V)
        self.register_buffer("J_regressor", f32(J_regressor))
        self.register_buffer("lbs_weights", f32(weights))
        self.register_buffer("parents", torch.tensor(parents, dtype=torch.long))
        extra, cocoplus, h36m = load_extra_joint_regressors(model_files_dir)      # smpl_official.py:17-25
        self.register_buffer("J_regressor_extra", f32(extra))
        self.register_buffer("J_regressor_cocoplus", f32(cocoplus))
        self.register_buffer("J_regressor_h36m", f32(h36m))
        # zero-initialised module parameters of `batch_size` rows, the defaults smplx falls back to
        self.betas = nn.Parameter(torch.zeros(batch_size, num_betas), requires_grad=False)
        self.global_orient = nn.Parameter(torch.zeros(batch_size, 3), requires_grad=False)
        self.body_pose = nn.Parameter(torch.zeros(batch_size, 69), requires_grad=False)

        # ---- kernel-side constants (derived in float64, stored fp32; not part of the state dict) ----
        nb = num_betas
        n_pose = posedirs_v3k.shape[-1]
        self._N = 3 * V
        self._n_pose = n_pose
        self._kp = _round_up(nb + n_pose, 16)
        self._k_used = _round_up(nb + n_pose, 2)          # rows the fused kernel multiplies (the rest of the 16-row padding is zero)
        # rows the shared-shape form multiplies: the pose rows alone, rounded up to even ON THEIR OWN (207 -> 208) -- not _k_used - nb,
        # which is odd for an odd nb (nb = 11: 218 - 11 = 207, refused by the library).  Row nb + 207 of the operands is a zero row of
        # the 16-row padding whenever the form is taken (_k_used == 218: nb + 208 <= 219 < _kp = 224).
        self._kp_pose = _round_up(n_pose, 2)
        self._np = _round_up(self._N, 128)
        bmat = np.zeros((self._kp, self._np), np.float64)
        bmat[:nb, :self._N] = shapedirs.reshape(self._N, nb).T                    # row l: d v[n] / d beta_l
        bmat[nb:nb + n_pose, :self._N] = posedirs_v3k.reshape(self._N, n_pose).T
        self.register_buffer("_bmat", f32(bmat), persistent=False)
        # the same matrix with panel-permuted columns for the fused kernel (include/hps.h: hps_smpl_mesh_fused):
        # col(v, c) = (v // 64) * 192 + c * 64 + v % 64
        self._np_fused = -(-V // 64) * 192
        vi = np.arange(V)
        bmat_p = np.zeros((self._kp, self._np_fused), np.float64)
        for c in range(3):
            bmat_p[:, (vi // 64) * 192 + c * 64 + vi % 64] = bmat[:, 3 * vi + c]
        self.register_buffer("_bmat_p", f32(bmat_p), persistent=False)
        self.register_buffer("_v_template_flat", f32(v_template.reshape(-1)), persistent=False)
        # joint regression folded through the linear shape blend: J = J_reg (v_t + S beta)
        self.register_buffer("_j_template", f32(J_regressor @ v_template), persistent=False)                 # (J,3)
        self.register_buffer("_j_shapedirs", f32(np.einsum("jv,vcl->jcl", J_regressor, shapedirs)), persistent=False)
        depth = np.zeros(J, np.int32)
        for j in range(1, J):
            depth[j] = depth[parents[j]] + 1
        self.register_buffer("_parents_i32", torch.tensor(parents, dtype=torch.int32), persistent=False)
        self.register_buffer("_depth_i32", torch.tensor(depth, dtype=torch.int32), persistent=False)
        # compressed skinning weights: K entries per vertex, exact when K >= max non-zeros per row
        nnz = int((weights != 0).sum(1).max())
        K = next(k for k in _LBS_K_CHOICES if k >= nnz)
        order = np.argsort(-(weights != 0).astype(np.int8), axis=1, kind="stable")[:, :K]   # non-zeros first, index order
        w_val = np.take_along_axis(weights, order, axis=1)
        w_idx = np.where(w_val != 0, order, 0)
        self._lbs_k = K
        # the fused mesh kernel exists for K = 4 (any joint count) and K = 8, 12 (24 joints): include/hps.h hps_smpl_mesh_fused;
        # denser skinning weights take the unfused pair (same bits)
        self._fused_ok = K == 4 or (K in (8, 12) and J == 24)
        self.register_buffer("_w_idx", torch.tensor(w_idx, dtype=torch.int32).contiguous(), persistent=False)
        self.register_buffer("_w_val", f32(w_val).contiguous(), persistent=False)
        # joint rows after the 24 kinematic joints: 21 vertex picks (smplx VertexJointSelector), then the
        # extra / cocoplus / h36m regressors (smpl_official.py:30-34) -- one CSR matrix over the vertices
        picks = np.zeros((len(SMPLX_EXTRA_VERTEX_IDS), V))
        picks[np.arange(len(SMPLX_EXTRA_VERTEX_IDS)), SMPLX_EXTRA_VERTEX_IDS] = 1.0
        rows = [picks, extra, cocoplus, h36m]
        dense = np.concatenate(rows, axis=0)
        ptr_, col_, val_ = [0], [], []
        for r in range(dense.shape[0]):
            nz = np.nonzero(dense[r])[0]
            col_.extend(nz.tolist())
            val_.extend(dense[r, nz].tolist())
            ptr_.append(len(col_))
        self._n_joint_rows = dense.shape[0]
        # the distinct vertices those rows read (SMPL: 198 of 6 890) get a slot in a compact array the fused mesh kernel fills beside
        # the vertices (hps_smpl_mesh_fused_picks); the joint kernel then reads that array through the entries' slots
        uniq = sorted(set(col_))
        slot_of = {v: i for i, v in enumerate(uniq)}
        pick_slot = np.full(V, -1, np.int32)
        pick_slot[uniq] = np.arange(len(uniq), dtype=np.int32)
        self._n_picked = len(uniq)
        self.register_buffer("_pick_slot", torch.tensor(pick_slot, dtype=torch.int32), persistent=False)
        self.register_buffer("_csr_slot", torch.tensor([slot_of[v] for v in col_], dtype=torch.int32), persistent=False)
        self.picked_joints = True       # False: gather the regressor vertices from the mesh (the round-4 route; same bits)
        self.register_buffer("_csr_ptr", torch.tensor(ptr_, dtype=torch.int32), persistent=False)
        self.register_buffer("_csr_col", torch.tensor(col_, dtype=torch.int32), persistent=False)
        self.register_buffer("_csr_val", torch.tensor(val_, dtype=torch.float32), persistent=False)
        # backward: the same matrix transposed (CSR over the vertices, a vertex's entries in row order) -- over all vertices for the
        # dense route, over the picked vertices' slots for the joints-only route, which runs the backward kernels on the picked
        # vertices alone (their columns of the blend matrix, their skinning weights: _picked_tables)
        row_of = np.repeat(np.arange(dense.shape[0]), np.diff(ptr_))
        def transposed(cols, n):
            order = np.argsort(np.asarray(cols, np.int64), kind="stable")
            tptr = np.concatenate([[0], np.cumsum(np.bincount(np.asarray(cols, np.int64), minlength=n))])
            return (torch.tensor(tptr, dtype=torch.int32), torch.tensor(row_of[order], dtype=torch.int32),
                    torch.tensor(np.asarray(val_, np.float64)[order], dtype=torch.float32))
        for name, t in zip(("_csrt_ptr", "_csrt_row", "_csrt_val"), transposed(col_, V)):
            self.register_buffer(name, t, persistent=False)
        for name, t in zip(("_pk_csrt_ptr", "_pk_csrt_row", "_pk_csrt_val"), transposed([slot_of[v] for v in col_], len(uniq))):
            self.register_buffer(name, t, persistent=False)
        self.register_buffer("_pk_verts", torch.tensor(uniq, dtype=torch.long), persistent=False)
        self._last_backward = None

    def shared_shape_tables(self, mesh_rows):
        """The (mesh_row, group_rows) tables of hps_smpl_mesh_fused_shared_shape for meshes whose shapes are rows of a small table:
        ``mesh_rows`` (M,) host integers, mesh m has shape row mesh_rows[m].  Device int32 tensors, padded to the kernel's mesh count."""
        rows = np.asarray(mesh_rows, np.int32).reshape(-1)
        M = rows.shape[0]
        mp = _capi.query_workspace(_capi.WS_SMPL_MP, M)
        full = np.concatenate([rows, np.full(mp - M, rows[-1] if M else 0, np.int32)])
        groups = np.zeros((mp // 32, 3), np.int32)
        for g in range(mp // 32):
            r = full[32 * g:32 * g + 32]
            change = np.nonzero(r[1:] != r[:-1])[0]
            if change.size == 0:
                groups[g] = (r[0], r[0], 32)
            elif change.size == 1:
                groups[g] = (r[0], r[-1], change[0] + 1)
            else:
                groups[g] = (r[0], r[0], -1)
        dev = self.v_template.device
        return torch.from_numpy(full).to(dev), torch.from_numpy(groups.reshape(-1)).to(dev)

    def layout_tables(self, layout, mesh_rows):
        """shared_shape_tables(mesh_rows()) kept in the device state for a few ``layout`` keys (infer(): (B, N))."""
        return self._derived("layouts", layout, lambda: self.shared_shape_tables(mesh_rows()))

    def _blend_matrix_split(self, with_shape_rows=False):
        """The panel-permuted blend matrix as bf16 piece planes in MFMA fragment order (once per device state): the 207 pose rows
        (shared shapes) or, ``with_shape_rows``, all num_betas + 207 rows (the shape blend inside the GEMM)."""
        def build():
            first, rows = (0, self.num_betas + self._n_pose) if with_shape_rows else (self.num_betas, self._n_pose)
            n = _capi.load(dev=_capi._use_dev).hps_smpl_split_bf16x3_bytes(rows, self._np_fused)
            buf = torch.empty(n, dtype=torch.uint8, device=self._bmat_p.device)
            _capi.call("hps_smpl_split_bf16x3", _capi._P(self._bmat_p.data_ptr() + 4 * first * self._np_fused), rows, self._np_fused,
                       self._np_fused, 192, _capi._P(buf.data_ptr()), _capi.stream())
            return buf
        return self._derived("bsplit", with_shape_rows, build)

    def _one_shape_tables(self, mp):
        """(mesh_row, group_rows) of the bf16x3 kernel for a call whose meshes do NOT share shapes: one template row (v_template) for all."""
        dev = self.v_template.device
        return self._derived("one_shape", mp, lambda: (torch.zeros(mp, dtype=torch.int32, device=dev),
                                                        torch.tensor([0, 0, 32], dtype=torch.int32).repeat(mp // 32).to(dev)))

    def _picked_tables(self):
        """Constants of the joints-only backward (once per device state): the picked vertices' columns of the blend matrix padded to
        the kernels' multiple, their template entries and skinning weights."""
        def build():
            n = self._n_picked
            cols = (3 * self._pk_verts.unsqueeze(1) + torch.arange(3, device=self._pk_verts.device)).reshape(-1)
            np_ = _round_up(3 * n, 128)
            bmat = torch.zeros(self._kp, np_, dtype=torch.float32, device=cols.device)
            bmat[:, :3 * n] = self._bmat.index_select(1, cols)
            return dict(V=n, N=3 * n, np=np_, bmat=bmat, v_template=self._v_template_flat.index_select(0, cols).contiguous(),
                        w_idx=self._w_idx.index_select(0, self._pk_verts).contiguous(),
                        w_val=self._w_val.index_select(0, self._pk_verts).contiguous(),
                        csrt=(self._pk_csrt_ptr, self._pk_csrt_row, self._pk_csrt_val))
        return self._derived("picked_bwd", 0, build)

    def _backward(self, g, b, be, pose2rot, g_verts, g_joints, needs):
        """Gradients of (global_orient, body_pose, betas, transl), fp32 (M, -1) like the Function's inputs; ``needs``: which of
        them are wanted.  g_verts / g_joints: cotangents of vertices / joints or None."""
        if (g_verts is None and g_joints is None) or not any(needs):
            return (None, None, None, None)
        dev, J, M = g.device, self.NUM_JOINTS, g.shape[0]
        f32 = dict(device=dev, dtype=torch.float32)
        P, IP, s = _capi.ptr, _capi.iptr, _capi.stream()
        g_verts = None if g_verts is None else _capi.f32c(g_verts)
        g_joints = None if g_joints is None else _capi.f32c(g_joints)
        is_rotmat = 0 if pose2rot else 1
        picked = g_verts is None and self._n_picked > 0
        if picked:
            t = self._picked_tables()
        else:
            t = dict(V=self.num_verts, N=self._N, np=self._np, bmat=self._bmat, v_template=self._v_template_flat, w_idx=self._w_idx,
                     w_val=self._w_val, csrt=(self._csrt_ptr, self._csrt_row, self._csrt_val))
        mp = _capi.query_workspace(_capi.WS_SMPL_MP, M)
        xt = torch.empty(self._kp, mp, **f32)
        a = torch.empty(M, J, 12, **f32)
        j_posed = torch.empty(M, J, 3, **f32)
        fwd_args = (P(g), P(b), is_rotmat, P(be), self.num_betas, P(self._j_template), P(self._j_shapedirs),
                    IP(self._parents_i32), IP(self._depth_i32), J)
        _capi.call("hps_smpl_pose_prep", *fwd_args, P(xt), self._kp, mp, P(a), P(j_posed), None, M, s)
        ld = t["np"]
        v_posed = torch.empty(M, ld, **f32)          # becomes g_vposed in place
        _capi.call("hps_smpl_blend", P(xt), P(t["bmat"]), P(t["v_template"]), P(v_posed), M, t["N"], self._kp, mp, t["np"], ld, s)
        g_a = torch.empty(M, J, 12, **f32)
        g_tr = torch.empty(M, 3, **f32) if needs[3] else None
        ws = torch.empty(_capi.query_workspace(_capi.WS_SMPL_LBS_BWD, M, t["V"], J) // 4, **f32)
        csrt = t["csrt"] if g_joints is not None else (None, None, None)
        _capi.call("hps_smpl_lbs_backward", P(v_posed), ld, P(a), IP(t["w_idx"]), P(t["w_val"]), self._lbs_k, J, P(g_verts),
                   P(g_joints), self._n_joint_rows, IP(csrt[0]), IP(csrt[1]), P(csrt[2]), P(g_a), P(g_tr), P(ws), M, t["V"], s)
        g_g = g_b = g_be = g_xt = None
        if any(needs[:3]):
            g_xt = torch.empty(self._kp, mp, **f32)
            ws2 = torch.empty(_capi.query_workspace(_capi.WS_SMPL_BLEND_BWD, M, self._kp, t["np"]) // 4, **f32)
            _capi.call("hps_smpl_blend_backward", P(t["bmat"]), P(v_posed), P(g_xt), P(ws2), M, self._kp, mp, t["np"], ld, s)
            g_g = torch.empty_like(g) if needs[0] else None
            g_b = torch.empty_like(b) if needs[1] else None
            g_be = torch.empty_like(be) if needs[2] else None
            _capi.call("hps_smpl_pose_prep_backward", *fwd_args, P(g_a), P(g_joints), self._n_joint_rows, P(g_xt), mp, P(g_g),
                       P(g_b), P(g_be), M, s)
        if self.keep_intermediates:                                         # tests / profiling only
            self._last_backward = dict(route="picked" if picked else "dense", M=M, g_a=g_a, g_xt=g_xt, g_vposed=v_posed)
        return (g_g, g_b, g_be, g_tr)

    # ------------------------------------------------------------------------------------------
    def forward(self, betas=None, body_pose=None, global_orient=None, transl=None, pose2rot=True,
                return_verts=True, return_full_pose=False, **kwargs):
        """smplx SMPL.forward semantics as used by the reference (models/smpl_official.py:27-41):
        omitted arguments default to the zero module parameters; betas with fewer rows than the pose
        are expanded; ``pose2rot=False`` takes rotation matrices, otherwise axis-angle.

        Differentiable: with grad mode on and any of betas / body_pose / global_orient / transl (the module's own parameters
        included) requiring grad, the call goes through a torch.autograd.Function.  Its forward launches the kernels of a no_grad
        call in their K = 217 forms (hps_smpl_mesh_fused[_picks], or blend + lbs with ``fused_mesh = False``, then hps_smpl_joints) and
        returns the same bits; ``mesh_arith = "bf16x3"`` and ``shared_shape`` do not apply on this route.  The backward saves the
        inputs only, recomputes xt / a / v_posed and runs hps_smpl_lbs_backward, hps_smpl_blend_backward and
        hps_smpl_pose_prep_backward; when only ``joints`` received a cotangent it runs them on the regressor vertices alone
        (``_last_backward["route"] == "picked"`` under ``keep_intermediates``).  For ``pose2rot=False`` the pose gradients are those of
        the unconstrained matrix entries.  No host synchronisation either way.  The private hooks of the inference pipeline
        (``_shared_shapes``, ``_before_mesh``, ``_after_mesh``, ``_defer_joints``) cannot be combined with it: ValueError."""
        dev = self.v_template.device
        _capi.require_device(self.v_template, "SMPL buffers (call .to('cuda'))")
        J = self.NUM_JOINTS
        global_orient = self.global_orient if global_orient is None else global_orient
        body_pose = self.body_pose if body_pose is None else body_pose
        betas = self.betas if betas is None else betas
        for name, t in (("betas", betas), ("body_pose", body_pose), ("global_orient", global_orient)):
            _capi.require_device(t, name)
        M = max(betas.shape[0], global_orient.shape[0], body_pose.shape[0])
        if betas.shape[0] != M:
            betas = betas.expand(int(M / betas.shape[0]), -1) if betas.shape[0] == 1 else betas.repeat(int(M / betas.shape[0]), 1)
        if global_orient.shape[0] != M or body_pose.shape[0] != M:
            raise ValueError("global_orient / body_pose must have the same number of rows")

        g = _capi.f32c(global_orient).reshape(M, -1)
        b = _capi.f32c(body_pose).reshape(M, -1)
        is_rotmat = 0 if pose2rot else 1
        exp_g, exp_b = (9, 9 * (J - 1)) if is_rotmat else (3, 3 * (J - 1))
        if g.shape[1] != exp_g or b.shape[1] != exp_b:
            raise ValueError("pose2rot=%s expects global_orient with %d and body_pose with %d values per mesh, got %d / %d"
                             % (pose2rot, exp_g, exp_b, g.shape[1], b.shape[1]))
        be = _capi.f32c(betas)
        if be.shape[1] != self.num_betas:
            raise ValueError("betas must have %d columns" % self.num_betas)
        tr = None if transl is None else _capi.f32c(transl).reshape(M, 3)
        if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (g, b, be, tr)):
            hooks = [h for h in ("_shared_shapes", "_before_mesh", "_after_mesh", "_defer_joints") if kwargs.get(h) is not None]
            if hooks:
                raise ValueError("SMPL.forward: %s cannot be combined with inputs that require grad (the hooks belong to the "
                                 "inference pipeline, which has no backward)" % ", ".join(hooks))
            # (betas were expanded and every input brought to fp32 (M, -1) above, OUTSIDE the Function: autograd sums / casts back)
            verts, joints = _SMPLFunction.apply(self, bool(pose2rot), g, b, be, tr)
            return SMPLOutput(vertices=verts if return_verts else None, joints=joints,
                              full_pose=torch.cat([g, b], dim=1) if return_full_pose else None,
                              betas=betas, global_orient=global_orient, body_pose=body_pose)

        V, N = self.num_verts, self._N
        mp = _capi.query_workspace(_capi.WS_SMPL_MP, M)                  # padded mesh count of the blend operand
        f32 = dict(device=dev, dtype=torch.float32)
        xt = torch.empty(self._kp, mp, **f32)
        a = torch.empty(M, J, 12, **f32)
        j_posed = torch.empty(M, J, 3, **f32)
        s = _capi.stream()
        P = _capi.ptr
        verts = torch.empty(M, V, 3, **f32)
        joints = torch.empty(M, J + self._n_joint_rows, 3, **f32)
        # the SMPL configuration also gets the regressor vertices as a compact side output of the mesh kernel
        use_picks = (self.fused_mesh and self._fused_ok and self.picked_joints and self._lbs_k == 4 and J == 24 and self._k_used == 218
                     and self._n_picked > 0)
        picked = torch.empty(M, self._n_picked, 3, **f32) if use_picks else None
        # ``_shared_shapes = (shape_betas (R, num_betas), mesh_row, group_rows)``: betas[m] == shape_betas[mesh_row[m]] (the caller's
        # promise -- infer(use_mean_shape=True)): the shape blend once per distinct shape, the GEMM over the pose rows only
        shared = kwargs.get("_shared_shapes") if (self.shared_shape and use_picks and tr is None) else None
        v_shaped = None
        if self.mesh_arith not in ("f32", "bf16x3"):
            raise ValueError("mesh_arith must be 'f32' or 'bf16x3', got %r" % (self.mesh_arith,))
        # bf16x3: the shared-shape form (207 pose rows), or -- no shared shapes, SMPL configuration, no translation -- the same kernel over
        # all 217 rows with v_template as the one "shaped template" (the shape blend inside the GEMM, as in the fp32 K = 217 form)
        split = self.mesh_arith == "bf16x3" and use_picks and tr is None and self.fused_mesh and not kwargs.get("_k217")
        split_rows = (self.num_betas, self._n_pose) if shared is not None else (0, self.num_betas + self._n_pose)      # (first row, rows)
        xsplit = bsplit = None
        if shared is not None:
            sb = _capi.f32c(shared[0])
            v_shaped = torch.empty(sb.shape[0], V, 3, **f32)
            _capi.call("hps_smpl_v_shaped", P(sb), self.num_betas, P(self._bmat), self._np, P(self._v_template_flat), P(v_shaped),
                       sb.shape[0], V, s)
        _capi.call("hps_smpl_pose_prep", P(g), P(b), is_rotmat, P(be), self.num_betas, P(self._j_template),
                   P(self._j_shapedirs), _capi.iptr(self._parents_i32), _capi.iptr(self._depth_i32), J, P(xt),
                   self._kp, mp, P(a), P(j_posed), None, M, s)
        if split:
            lib = _capi.load(dev=_capi._use_dev)
            bsplit = self._blend_matrix_split(with_shape_rows=shared is None)
            xsplit = torch.empty(lib.hps_smpl_split_bf16x3_bytes(split_rows[1], mp), dtype=torch.uint8, device=dev)
            _capi.call("hps_smpl_split_bf16x3", _capi._P(xt.data_ptr() + 4 * split_rows[0] * mp), split_rows[1], mp, mp,
                       lib.hps_smpl_split_bf16x3_mesh_tile(), _capi._P(xsplit.data_ptr()), s)
        # InferencePipeline: only the chip-filling mesh kernel(s) run alone; pose prep (before) and the joint regression (after)
        # may share the GPU with the neighbouring batches' encoders
        if kwargs.get("_before_mesh") is not None:
            entry_stream = torch.cuda.current_stream()
            ordered = kwargs["_before_mesh"]()
            now = torch.cuda.current_stream()
            if now != entry_stream:              # the hook moved the mesh kernel to another stream (InferencePipeline.inline_mesh)
                s = _capi.stream()
                # The operands were allocated on the entry stream.  A hook that returns "ordered" promises that its _after_mesh
                # partner makes the entry stream wait for the mesh kernel before anything else is queued there: the allocator hands
                # these blocks back to the entry stream's pool only, so every reuse is ordered behind the kernel.  Without the promise
                # the tensors are registered with the other stream -- which costs an event record ON THAT STREAM for each of them
                # when they are freed (seven markers of ~6 us in front of the next encoder, measured: profiles/r05_experiments.txt).
                if ordered != "ordered":
                    for t in (xt, a, verts, picked, be, g, b, v_shaped, xsplit):
                        if t is not None:
                            t.record_stream(now)
        ev = None
        if self.lbs_events is not None:      # bench.py: HIP events around the mesh kernel launch, on its own stream
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        trp = P(tr) if tr is not None else None
        v_posed = None
        if self.fused_mesh and self._fused_ok:
            if ev is not None:
                ev[0].record()
            if split:
                rows_t, groups_t = (shared[1], shared[2]) if shared is not None else self._one_shape_tables(mp)
                _capi.call("hps_smpl_mesh_fused_shared_shape_bf16x3", _capi._P(xsplit.data_ptr()), _capi._P(bsplit.data_ptr()),
                           P(v_shaped) if shared is not None else P(self._v_template_flat), _capi.iptr(rows_t), _capi.iptr(groups_t), P(a),
                           _capi.iptr(self._w_idx), P(self._w_val), self._lbs_k, J, P(verts), M, V, split_rows[1], mp,
                           _capi.iptr(self._pick_slot), P(picked), self._n_picked, s)
            elif shared is not None:
                nb = self.num_betas
                _capi.call("hps_smpl_mesh_fused_shared_shape", _capi._P(xt.data_ptr() + 4 * nb * mp), _capi._P(self._bmat_p.data_ptr() + 4 * nb * self._np_fused),
                           P(v_shaped), _capi.iptr(shared[1]), _capi.iptr(shared[2]), P(a), _capi.iptr(self._w_idx), P(self._w_val), self._lbs_k, J,
                           P(verts), M, V, self._kp_pose, mp, self._np_fused, _capi.iptr(self._pick_slot), P(picked), self._n_picked, s)
            elif use_picks:
                _capi.call("hps_smpl_mesh_fused_picks", P(xt), P(self._bmat_p), P(self._v_template_flat), P(a),
                           _capi.iptr(self._w_idx), P(self._w_val), self._lbs_k, J, trp, P(verts), M, V, self._k_used, mp,
                           self._np_fused, _capi.iptr(self._pick_slot), P(picked), self._n_picked, s)
            else:
                _capi.call("hps_smpl_mesh_fused", P(xt), P(self._bmat_p), P(self._v_template_flat), P(a),
                           _capi.iptr(self._w_idx), P(self._w_val), self._lbs_k, J, trp, P(verts), M, V, self._k_used, mp,
                           self._np_fused, s)
        else:
            ldv = self._np if self.pad_v_posed else N          # row pitch of v_posed in floats (128-byte aligned rows)
            v_posed = torch.empty(M, ldv, **f32)
            _capi.call("hps_smpl_blend", P(xt), P(self._bmat), P(self._v_template_flat), P(v_posed), M, N, self._kp,
                       mp, self._np, ldv, s)
            if ev is not None:
                ev[0].record()
            _capi.call("hps_smpl_lbs", P(v_posed), ldv, P(a), _capi.iptr(self._w_idx), P(self._w_val), self._lbs_k, J,
                       trp, P(verts), M, V, s)
        if ev is not None:
            ev[1].record()
            self.lbs_events.append((M, ev[0], ev[1]))
        if kwargs.get("_after_mesh") is not None:
            # (an event already recorded right behind the mesh kernel -- bench.py's timing event -- is handed to the hook, which may wait
            # on it instead of recording one of its own: an event record costs the queue ~8 us)
            kwargs["_after_mesh"](ev[1] if ev is not None else None)
            s = _capi.stream()                   # (the hook may have switched back to the caller's stream)
        if picked is not None and kwargs.get("_defer_joints") is not None:
            # infer(): the joint regression rides in the launch of the uncertainty pass (hps_joints_and_uncertainty); the caller gets the
            # launch's joint arguments and fills ``joints`` itself
            kwargs["_defer_joints"](dict(picked=picked, j_posed=j_posed, csr_ptr=self._csr_ptr, csr_slot=self._csr_slot, csr_val=self._csr_val,
                                         n_rows=self._n_joint_rows, J=J, transl=tr, joints=joints, M=M, n_picked=self._n_picked))
        elif picked is not None:      # the regressor vertices lie side by side: same rows, same values, same sums
            _capi.call("hps_smpl_joints", P(picked), P(j_posed), _capi.iptr(self._csr_ptr), _capi.iptr(self._csr_slot),
                       P(self._csr_val), self._n_joint_rows, J, P(tr) if tr is not None else None, P(joints), M, self._n_picked, s)
        else:
            _capi.call("hps_smpl_joints", P(verts), P(j_posed), _capi.iptr(self._csr_ptr), _capi.iptr(self._csr_col),
                       P(self._csr_val), self._n_joint_rows, J, P(tr) if tr is not None else None, P(joints), M, V, s)
        full_pose = torch.cat([g, b], dim=1) if return_full_pose else None
        if self.keep_intermediates:                                         # tests / profiling only
            self._last = dict(xt=xt, a=a, j_posed=j_posed)
            if v_posed is not None:
                self._last.update(v_posed=v_posed[:, :N].reshape(M, V, 3), v_posed_raw=v_posed, ldv=ldv)
        return SMPLOutput(vertices=verts if return_verts else None, joints=joints, full_pose=full_pose,
                          betas=betas, global_orient=global_orient, body_pose=body_pose)
