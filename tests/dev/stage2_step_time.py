"""Times of the stage-2 training step (train/train_poseMF_shapeGaussian_net.py:292-320) on one MI355X: the sampler's forward on the
differentiable route beside the no_grad one, hps_mf_sample_backward with the bytes it moves, and one whole stage-2 forward + backward
from cached features beside the stage-1 one in the same run, with every library call of one stage-2 step.

    python tests/dev/stage2_step_time.py [--out profiles/stage2_step_time.txt]

Single calls and whole steps: 3 warm-up rounds, then the median of 10 rounds (HIP events around the call, host work included).  Call
list: one more round with an event pair around every call into the library.  Bytes of the backward kernel: 52 per sample and joint
(4 quaternion + 9 g_R floats) plus 21 floats read and 21 written per (image, joint); rates as a fraction of the 8 TB/s HBM peak."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from hierarchicalprobabilistic3dhuman_amd import _capi, configs, smpl_data, sampling_utils as su  # noqa: E402
from hierarchicalprobabilistic3dhuman_amd.matrix_fisher_loss import PoseMFShapeGaussianLoss  # noqa: E402
from hierarchicalprobabilistic3dhuman_amd.smpl_official import SMPL  # noqa: E402
import head_grad_scenario as HS  # noqa: E402
import test_gpu_stage2 as T  # noqa: E402

HBM_PEAK = 8.0e12
WARMUP, ROUNDS = 3, 10
med = lambda v: sorted(v)[len(v) // 2]


def timed(fn):
    for _ in range(WARMUP):
        fn()
    out = []
    for _ in range(ROUNDS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return med(out)


def sampler_rows(net, dev, B, N):
    g = torch.Generator().manual_seed(B)
    with torch.no_grad():
        out = T.outputs(net(None, input_feats=torch.rand(B, 512, generator=g).to(dev)))
    U, S, V = (out[k].detach() for k in ("pose_U", "pose_S", "pose_V"))
    leaves = [t.clone().requires_grad_(True) for t in (U, S, V)]

    def plain():
        with torch.no_grad():
            su.pose_matrix_fisher_sampling_torch(U, S, V, N, seed=1)

    t_plain = timed(plain)
    t_diff = timed(lambda: su.pose_matrix_fisher_sampling_torch(*leaves, N, seed=1))
    R = su.pose_matrix_fisher_sampling_torch(*leaves, N, seed=1)
    quat = R.grad_fn.saved_tensors[3]
    g_R = torch.randn(B, N, 23, 3, 3, generator=g).to(dev)
    outs = [torch.empty_like(t) for t in (U, S, V)]
    P = _capi.ptr
    t_bwd = timed(lambda: _capi.call("hps_mf_sample_backward", P(U), P(S), P(V), None, None, None, P(quat), P(g_R), B * 23, 23, N, 1.5, P(outs[0]), P(outs[1]),
                                     P(outs[2]), _capi.stream()))
    su.check_sampling()
    nbytes = B * 23 * (52.0 * N + 2 * 21 * 4)
    return ["B = %d, N = %d (%d calls of %d samples):" % (B, N, B * 23, N),
            "  sampler forward, no_grad route            %9.3f ms" % t_plain,
            "  sampler forward, differentiable route     %9.3f ms   (the same launch + the quaternions, autograd bookkeeping)" % t_diff,
            "  hps_mf_sample_backward                    %9.3f ms   %8.3f MB  %6.3f TB/s = %.4f of 8 TB/s"
            % (t_bwd, nbytes / 1e6, nbytes / (t_bwd * 1e-3) / 1e12, nbytes / (t_bwd * 1e-3) / HBM_PEAK)]


def stage1_loss(net, smpl, out, target, criterion):
    from torch.distributions import Normal
    from hierarchicalprobabilistic3dhuman_amd import cam_utils, rigid_transform_utils as rtu
    glob_rotmats = rtu.rot6d_to_rotmat(out["glob"])
    mode_out = smpl(body_pose=out["mode"], global_orient=glob_rotmats.unsqueeze(1), betas=out["loc"], pose2rot=False)
    j2d = cam_utils.orthographic_project_torch(cam_utils.flip_about_x(mode_out.joints[:, T.ALL_JOINTS_TO_COCO_MAP]), out["cam"])
    pred = {"pose_params_F": out["pose_F"], "pose_params_U": out["pose_U"], "pose_params_S": out["pose_S"],
            "pose_params_V": out["pose_V"], "shape_params": Normal(out["loc"], out["scale"], validate_args=False),
            "joints2D": j2d[:, None], "glob_rotmats": glob_rotmats, "verts": mode_out.vertices, "joints3D": mode_out.joints[:, T.J14]}
    return criterion(target, pred)


def step(net, smpl, feats, target, criterion, stage2):
    net.zero_grad(set_to_none=True)
    f = feats.detach().requires_grad_(True)
    out = T.outputs(net(None, input_feats=f))
    if stage2:
        loss = T.stage2_loss(net, smpl, out, target, criterion, False, 17, 23, pin_shape_noise=False)[0]
    else:
        loss = stage1_loss(net, smpl, out, target, criterion)
    loss.backward()


def call_list(fn):
    log, real = [], _capi.call

    def timed_call(name, *args):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        real(name, *args)
        e1.record()
        log.append((name, e0, e1))

    _capi.call = timed_call
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        _capi.call = real
    return [(n, e0.elapsed_time(e1)) for n, e0, e1 in log]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stage2_step_time.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    net = HS.make_net("spread").to(dev)
    net.set_differentiable_factors(True)
    smpl = SMPL(smpl_data.synthetic_smpl_model(0)).to(dev)
    lines = ["The stage-2 training step on one MI355X (gfx950), default kernels, head of head_grad_scenario's spread recipe.",
             "tests/dev/stage2_step_time.py: HIP events; median of %d rounds after %d warm-up rounds; the call list is one further round with"
             % (ROUNDS, WARMUP), "an event pair around every call into the library.", ""]
    for B, N in ((72, 8), (64, 100)):
        lines += sampler_rows(net, dev, B, N) + [""]
    B = 72
    cfg = configs.get_cfg_defaults().LOSS
    feats = torch.rand(B, 512, generator=torch.Generator().manual_seed(1)).to(dev)
    target = T.stage2_targets(B, dev)
    c1, c2 = PoseMFShapeGaussianLoss(cfg.STAGE1, 256), PoseMFShapeGaussianLoss(cfg.STAGE2, 256)
    t1 = timed(lambda: step(net, smpl, feats, target, c1, False))
    t2 = timed(lambda: step(net, smpl, feats, target, c2, True))
    su.check_sampling()
    lines += ["one forward + backward from cached features (B = %d; stage 2: N = %d samples, 'means+samples'):" % (B, T.NS),
              "  stage 1 (mode mesh only)                  %9.3f ms" % t1,
              "  stage 2 (mode mesh + %d sample meshes)     %9.3f ms = %.2f x stage 1" % (T.NS, t2, t2 / t1), ""]
    calls = call_list(lambda: step(net, smpl, feats, target, c2, True))
    lines.append("every library call of one stage-2 forward + backward, in order:")
    total, by_name = 0.0, {}
    for name, ms in calls:
        lines.append("  %-40s %9.3f ms" % (name, ms))
        total += ms
        n0, t0 = by_name.get(name, (0, 0.0))
        by_name[name] = (n0 + 1, t0 + ms)
    lines += ["", "by entry point:"]
    for name, (n, ms) in sorted(by_name.items(), key=lambda kv: -kv[1][1]):
        lines.append("  %-40s %3d calls %9.3f ms  %5.1f %%" % (name, n, ms, 100.0 * ms / total))
    lines.append("  %-40s           %9.3f ms" % ("all library calls", total))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
