"""Times of the SMPL backward on one MI355X: every kernel of both routes (dense: cotangent on the vertices; picked: on the joints
only) by HIP events, and the whole backward against the whole forward through SMPL.forward under autograd.

    python tests/dev/smpl_backward_time.py [M ...]        # default 64 and 6528 meshes

Each kernel: 5 warm-up launches, then the median over 20 windows of 5 back-to-back launches (events around a window).  Rates use the
operations / bytes the algorithm needs: blend GEMMs 2 * 217 * 3 V FLOP per mesh against the sustained fp32 MFMA rate of
DESIGN.md section 4 (153.7 TF/s); LBS backward 3 * 12 V bytes per mesh (v_posed and gV read, g_vposed written)."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from hierarchicalprobabilistic3dhuman_amd import _capi, smpl_data  # noqa: E402
from hierarchicalprobabilistic3dhuman_amd.smpl_official import SMPL  # noqa: E402

MFMA_F32_SUSTAINED = 153.7e12
WARMUP, WINDOWS, PER_WINDOW = 5, 20, 5


def timed(fn):
    """Median microseconds per call."""
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(WINDOWS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(PER_WINDOW):
            fn()
        e1.record()
        torch.cuda.synchronize()
        t.append(e0.elapsed_time(e1) * 1e3 / PER_WINDOW)
    t.sort()
    return t[len(t) // 2]


def kernels(smpl, M, picked, dev):
    """{kernel: us} of one route's backward (and the forward blend at the same operands as the yardstick)."""
    P, IP, s = _capi.ptr, _capi.iptr, _capi.stream
    J, kp, nb = smpl.NUM_JOINTS, smpl._kp, smpl.num_betas
    g = torch.Generator().manual_seed(0)
    R = torch.linalg.qr(torch.randn(M, J, 3, 3, generator=g))[0].contiguous().to(dev)
    glob, body = R[:, :1].contiguous(), R[:, 1:].contiguous()
    betas = torch.randn(M, nb, generator=g).to(dev)
    if picked:
        t = smpl._picked_tables()
    else:
        t = dict(V=smpl.num_verts, N=smpl._N, np=smpl._np, bmat=smpl._bmat, v_template=smpl._v_template_flat, w_idx=smpl._w_idx,
                 w_val=smpl._w_val, csrt=(smpl._csrt_ptr, smpl._csrt_row, smpl._csrt_val))
    V, ld = t["V"], t["np"]
    mp = _capi.query_workspace(_capi.WS_SMPL_MP, M)
    f32 = dict(device=dev, dtype=torch.float32)
    xt, a, jp = torch.empty(kp, mp, **f32), torch.empty(M, J, 12, **f32), torch.empty(M, J, 3, **f32)
    v_posed = torch.empty(M, ld, **f32)
    gV = None if picked else torch.randn(M, V, 3, **f32)
    gJ = torch.randn(M, J + smpl._n_joint_rows, 3, **f32)
    g_a, g_tr, g_xt = torch.empty(M, J, 12, **f32), torch.empty(M, 3, **f32), torch.empty(kp, mp, **f32)
    ws1 = torch.empty(_capi.query_workspace(_capi.WS_SMPL_LBS_BWD, M, V, J) // 4, **f32)
    ws2 = torch.empty(_capi.query_workspace(_capi.WS_SMPL_BLEND_BWD, M, kp, t["np"]) // 4, **f32)
    g_g, g_b, g_be = torch.empty_like(glob), torch.empty_like(body), torch.empty_like(betas)
    fwd = (P(glob), P(body), 1, P(betas), nb, P(smpl._j_template), P(smpl._j_shapedirs), IP(smpl._parents_i32), IP(smpl._depth_i32), J)

    calls = {
        "hps_smpl_pose_prep": lambda: _capi.call("hps_smpl_pose_prep", *fwd, P(xt), kp, mp, P(a), P(jp), None, M, s()),
        "hps_smpl_blend": lambda: _capi.call("hps_smpl_blend", P(xt), P(t["bmat"]), P(t["v_template"]), P(v_posed), M, t["N"], kp, mp,
                                             t["np"], ld, s()),
        "hps_smpl_lbs_backward": lambda: _capi.call(
            "hps_smpl_lbs_backward", P(v_posed), ld, P(a), IP(t["w_idx"]), P(t["w_val"]), smpl._lbs_k, J, P(gV), P(gJ),
            smpl._n_joint_rows, IP(t["csrt"][0]), IP(t["csrt"][1]), P(t["csrt"][2]), P(g_a), P(g_tr), P(ws1), M, V, s()),
        "hps_smpl_blend_backward": lambda: _capi.call("hps_smpl_blend_backward", P(t["bmat"]), P(v_posed), P(g_xt), P(ws2), M, kp, mp,
                                                      t["np"], ld, s()),
        "hps_smpl_pose_prep_backward": lambda: _capi.call("hps_smpl_pose_prep_backward", *fwd, P(g_a), P(gJ), smpl._n_joint_rows,
                                                          P(g_xt), mp, P(g_g), P(g_b), P(g_be), M, s()),
    }
    return {k: timed(fn) for k, fn in calls.items()}, V       # (in this order: every kernel runs on what the one before it wrote)


def whole(smpl, M, picked, dev):
    """(forward us, backward us) of SMPL.forward under autograd, host work of the calls included."""
    g = torch.Generator().manual_seed(1)
    R = torch.linalg.qr(torch.randn(M, 24, 3, 3, generator=g))[0].contiguous().to(dev)
    x = [R[:, :1].contiguous().requires_grad_(True), R[:, 1:].contiguous().requires_grad_(True),
         torch.randn(M, smpl.num_betas, generator=g).to(dev).requires_grad_(True)]
    gV, gJ = torch.randn(M, smpl.num_verts, 3, device=dev), torch.randn(M, 90, 3, device=dev)
    tf, tb = [], []
    for it in range(WARMUP + WINDOWS):
        for t in x:
            t.grad = None
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        out = smpl(global_orient=x[0], body_pose=x[1], betas=x[2], pose2rot=False)
        e[1].record()
        if picked:
            torch.autograd.backward([out.joints], [gJ])
        else:
            torch.autograd.backward([out.vertices, out.joints], [gV, gJ])
        e[2].record()
        torch.cuda.synchronize()
        if it >= WARMUP:
            tf.append(e[0].elapsed_time(e[1]) * 1e3)
            tb.append(e[1].elapsed_time(e[2]) * 1e3)
    tf.sort(); tb.sort()
    return tf[len(tf) // 2], tb[len(tb) // 2]


def main():
    Ms = [int(a) for a in sys.argv[1:]] or [64, 6528]
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    smpl = SMPL(smpl_data.synthetic_smpl_model(0)).to(dev)
    for M in Ms:
        for picked in (False, True):
            k, V = kernels(smpl, M, picked, dev)
            fwd, bwd = whole(smpl, M, picked, dev)
            flop = 2.0 * 217 * 3 * V * M
            frac = lambda us: flop / (us * 1e-6) / MFMA_F32_SUSTAINED
            lbs_bytes = 3.0 * 12 * V * M
            route = "picked" if picked else "dense"
            print("M = %d, route %s (%d vertices)" % (M, route, V))
            for name, us in k.items():
                print("  %-30s %9.1f us" % (name, us))
            print("  blend backward: %.1f TF/s = %.3f of the sustained fp32 MFMA rate; forward hps_smpl_blend: %.1f TF/s = %.3f"
                  % (flop / k["hps_smpl_blend_backward"] / 1e6, frac(k["hps_smpl_blend_backward"]),
                     flop / k["hps_smpl_blend"] / 1e6, frac(k["hps_smpl_blend"])))
            print("  LBS backward: %.1f MB algorithmic -> %.2f TB/s" % (lbs_bytes / 1e6, lbs_bytes / k["hps_smpl_lbs_backward"] / 1e6))
            print("  SMPL.forward under autograd %.1f us, backward %.1f us = %.2f x the forward" % (fwd, bwd, bwd / fwd))
            print(json.dumps(dict(M=M, route=route, V=V, kernels_us={n: round(v, 2) for n, v in k.items()},
                                  blend_backward_frac=round(frac(k["hps_smpl_blend_backward"]), 4),
                                  blend_forward_frac=round(frac(k["hps_smpl_blend"]), 4),
                                  lbs_backward_TBps=round(lbs_bytes / k["hps_smpl_lbs_backward"] / 1e6, 3),
                                  forward_us=round(fwd, 1), backward_us=round(bwd, 1), backward_over_forward=round(bwd / fwd, 3))))


if __name__ == "__main__":
    main()
