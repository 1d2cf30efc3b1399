"""What a training step costs on one MI355X under four optimiser routes, in the same process:

    (a) torch.optim.Adam, torch's defaults          (b) torch.optim.Adam(fused=True), if this torch build accepts it
    (c) DeviceAdam, not registered: hps_adam_step, but the modules still drop and rebuild their device state behind every step
    (d) DeviceAdam(refresh=(net,)): hps_adam_step + hps_weights_refresh, the device state survives

    python tests/dev/train_step_time.py [--batch 72] [--size 256] [--out profiles/train_step_time.txt]

Default kernels, set_batchnorm_training(True) under .train(), stage-1 loss (PoseMFShapeGaussianLoss, LOSS.STAGE1) through SMPL, the head
and the encoder.  A step = zero_grad, forward + loss, backward, optimiser call; what the step does to the NEXT forward (the rebuild of
routes a-c) is inside the next step's forward, so steady-state steps carry it.  Every route has its own net and optimiser, all built
first; the routes are then ALTERNATED: one step of each per round, 3 warm-up rounds, then 10 rounds, so drift of the machine falls on
all routes alike.  A step is timed by the host clock between device synchronisations (the rebuild is partly host work: the stem's
Winograd filters are computed on the CPU), the median reported with the fastest and slowest; the three segments of a step the same
way, the backward also by HIP events.  Route (e) is a diagnostic, not a candidate: route (d) with the device left idle for 6 ms
before each step (not counted) -- the host-bound rebuild of routes (a) and (c) leaves such a gap in front of their kernels.  The rebuild of a route is its
forward segment minus route (d)'s.  Launch counts: kernels and copies torch's profiler sees inside one optimiser call.  Per route the
number of steps whose forward found the device state dropped is listed: torch's fused Adam does not move version counters.
hps_adam_step: HIP events around the library call, bytes = 28 per element (p, g, m, v read, p, m, v written)."""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from hierarchicalprobabilistic3dhuman_amd import _capi, configs, rigid_transform_utils as rtu, smpl_data  # noqa: E402
from hierarchicalprobabilistic3dhuman_amd.device_optim import DeviceAdam  # noqa: E402
from hierarchicalprobabilistic3dhuman_amd.matrix_fisher_loss import PoseMFShapeGaussianLoss  # noqa: E402
from hierarchicalprobabilistic3dhuman_amd.smpl_official import SMPL  # noqa: E402
import encoder_grad_scenario as ES  # noqa: E402
import head_grad_scenario as HS  # noqa: E402

HBM_PEAK = 8.0e12
WARMUP, ROUNDS = 3, 10
med = lambda v: sorted(v)[len(v) // 2]


def make_net(dev):
    net = HS.make_net("spread")
    ES.randomize_bn(net.image_encoder)
    net = net.to(dev)
    net.set_batchnorm_training(True)
    return net.train()


def targets(B, dev):
    g = torch.Generator().manual_seed(21)
    return {"pose_params_rotmats": rtu.batch_rodrigues((torch.randn(B * 23, 3, generator=g) * 0.3).to(dev)).view(B, 23, 3, 3),
            "shape_params": torch.randn(B, 10, generator=g).to(dev), "joints2D": (torch.rand(B, 17, 2, generator=g) * 256).to(dev),
            "joints2D_vis": torch.ones(B, 17, dtype=torch.bool, device=dev),
            "glob_rotmats": rtu.batch_rodrigues((torch.randn(B, 3, generator=g) * 0.3).to(dev)),
            "verts": torch.randn(B, 6890, 3, generator=g).to(dev), "joints3D": torch.randn(B, 14, 3, generator=g).to(dev)}


def stage1_loss(net, smpl, criterion, x, target):
    """tests/test_gpu_encoder_backward.chain_loss with the targets made once."""
    from torch.distributions import Normal
    pose_F, pose_U, pose_S, pose_V, mode, shape_dist, glob, cam = net(x)
    glob_rotmats = rtu.rot6d_to_rotmat(glob)
    out = smpl(body_pose=mode, global_orient=glob_rotmats.unsqueeze(1), betas=shape_dist.loc, pose2rot=False)
    joints2D = (out.joints[:, :17, :2] * cam[:, None, :1] + cam[:, None, 1:]).unsqueeze(1)
    pred = {"pose_params_F": pose_F, "pose_params_U": pose_U, "pose_params_S": pose_S, "pose_params_V": pose_V,
            "shape_params": Normal(shape_dist.loc, shape_dist.scale, validate_args=False), "joints2D": joints2D,
            "glob_rotmats": glob_rotmats, "verts": out.vertices, "joints3D": out.joints[:, :14]}
    return criterion(target, pred)


def one_step(net, smpl, criterion, x, target, opt, idle=0.0):
    """(whole step, forward + loss, backward, optimiser call, backward by HIP events) in ms, memory_allocated before and after."""
    sync, now = torch.cuda.synchronize, time.perf_counter
    sync()
    if idle:
        time.sleep(idle)
    mem0 = torch.cuda.memory_allocated()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    prep = net.image_encoder._prepared
    t0 = now()
    net.zero_grad(set_to_none=True)
    loss = stage1_loss(net, smpl, criterion, x, target)
    sync()
    t1 = now()
    rebuilt = prep is not None and net.image_encoder._prepared is not prep      # the forward dropped the state the last step left
    e0.record()
    loss.backward()
    e1.record()
    sync()
    t2 = now()
    opt.step()
    sync()
    t3 = now()
    return [1e3 * (t3 - t0), 1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (t3 - t2), e0.elapsed_time(e1), rebuilt], mem0, torch.cuda.memory_allocated()


def count_launches(opt):
    """(kernels, copies) the profiler sees on the device inside one optimiser call; None where it is not available."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            opt.step()
            torch.cuda.synchronize()
        dev_events = [e for e in prof.events() if str(e.device_type).endswith("CUDA")]
        copies = [e for e in dev_events if "memcpy" in e.name.lower() or "copy" in e.name.lower() and "kernel" not in e.name.lower()]
        return len(dev_events) - len(copies), len(copies)
    except Exception as e:                                    # the profiler is optional here
        print("profiler unavailable: %s" % e)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=72)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_step_time.txt"))
    ap.add_argument("--no-profiler", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    B, S = args.batch, args.size
    x = torch.rand(B, 18, S, S, generator=torch.Generator().manual_seed(0)).to(dev)
    smpl = SMPL(smpl_data.synthetic_smpl_model(0)).to(dev)
    criterion = PoseMFShapeGaussianLoss(loss_config=configs.get_cfg_defaults().LOSS.STAGE1, img_wh=256)
    target = targets(B, dev)
    routes = [("(a) torch.optim.Adam", lambda net: torch.optim.Adam(net.parameters(), lr=1e-4), 0.0),
              ("(b) torch.optim.Adam(fused=True)", lambda net: torch.optim.Adam(net.parameters(), lr=1e-4, fused=True), 0.0),
              ("(c) DeviceAdam, not registered", lambda net: DeviceAdam(net.parameters(), lr=1e-4), 0.0),
              ("(d) DeviceAdam, registered", lambda net: DeviceAdam(net.parameters(), lr=1e-4, refresh=(net,)), 0.0),
              ("(e) = (d) after 6 ms of idle device", lambda net: DeviceAdam(net.parameters(), lr=1e-4, refresh=(net,)), 0.006)]
    head = ["A training step on one MI355X (gfx950) under four optimiser routes: ResNet-18 encoder + head, input %d x 18 x %d x %d," % (B, S, S),
            "default kernels, training-mode BatchNorm, stage-1 loss.  tests/dev/train_step_time.py: the routes alternated (one step of each",
            "per round), host clock between device synchronisations, median (fastest .. slowest) of %d rounds after %d warm-up rounds, ms." % (ROUNDS, WARMUP), ""]
    results, adam_ms, n_elems, notes = {}, [], 0, []
    real_call = _capi.call
    timing = [False]

    def timed_call(name, *a):
        if name != "hps_adam_step" or not timing[0]:
            return real_call(name, *a)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        real_call(name, *a)
        e1.record()
        adam_ms.append((e0, e1))

    live = []
    for label, make_opt, idle in routes:
        net = make_net(dev)
        try:
            opt = make_opt(net)
        except (RuntimeError, ValueError, TypeError) as e:
            notes.append("%s: this torch build refuses it (%s)" % (label, e))
            continue
        n_elems = sum(p.numel() for p in net.parameters())
        live.append((label, net, opt, idle))
        results[label] = dict(rows=[], refresh=None, opt=opt, launches=None)
    _capi.call = timed_call
    try:
        for r in range(WARMUP + ROUNDS):
            for label, net, opt, idle in live:
                timing[0] = label.startswith("(d)") and r >= WARMUP
                row = one_step(net, smpl, criterion, x, target, opt, idle)
                if r >= WARMUP:
                    results[label]["rows"].append(row)
    finally:
        _capi.call = real_call
    for label, net, opt, idle in live:
        if label.startswith("(d)"):
            ts = []
            for _ in range(ROUNDS):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                net.refresh_weights()
                torch.cuda.synchronize()
                ts.append(1e3 * (time.perf_counter() - t0))
            results[label]["refresh"] = ts

    def report():
        lines = list(head)
        fmt = lambda v: "%9.3f (%9.3f .. %9.3f)" % (med(v), min(v), max(v))
        ref_fwd = med([r[0][1] for r in results[routes[3][0]]["rows"]]) if routes[3][0] in results else None
        lines.append("%-36s %-35s %-35s %-35s %-35s %-35s" % ("route", "whole step", "forward + loss", "backward", "optimiser call", "backward (HIP events)"))
        for label, _, _ in routes:
            if label not in results:
                continue
            rows = results[label]["rows"]
            lines.append("%-36s %s %s %s %s %s" % ((label,) + tuple(fmt([r[0][k] for r in rows]) for k in range(5))))
        lines.append("")
        for label, _, _ in routes:
            if label not in results:
                continue
            r = results[label]
            rows = r["rows"]
            fwd = med([q[0][1] for q in rows])
            if r["refresh"] is not None:
                what = "refresh (hps_weights_refresh, inside the optimiser call) %s" % fmt(r["refresh"])
            else:
                what = "rebuild (forward segment minus route (d)'s) %9.3f" % (fwd - ref_fwd) if ref_fwd is not None else "rebuild n/a"
            launches = "launches in the optimiser call: %s" % ("%d kernels, %d copies" % r["launches"] if r["launches"] else "not counted")
            lines.append("%-36s %s;  %s" % (label, what, launches))
            lines.append("%-36s the forward found the device state dropped (version counters moved) in %d of %d steps"
                         % ("", sum(bool(q[0][5]) for q in rows), len(rows)))
            lines.append("%-36s memory_allocated before / after a step: %s" % ("", ", ".join("%.1f / %.1f MB" % (a / 1e6, b / 1e6) for _, a, b in rows[-3:])))
        if adam_ms:
            ms = [a.elapsed_time(b) for a, b in adam_ms]
            nbytes = 28.0 * n_elems
            lines += ["", "hps_adam_step (HIP events around the call, %d steps): %s ms; %d elements, %.1f MB moved, %.2f TB/s = %.3f of the 8 TB/s HBM peak"
                      % (len(ms), fmt(ms), n_elems, nbytes / 1e6, nbytes / (med(ms) * 1e-3) / 1e12, nbytes / (med(ms) * 1e-3) / HBM_PEAK)]
        lines += ["", "torch.optim.Adam(fused=True) changes the parameters without moving their version counters (torch._fused_adam_): the modules do not",
                  "see its steps, keep their device state and run the next forward on the kernel-side weights of BEFORE the step -- route (b) is",
                  "timed as it runs, and what it runs is not a training loop of this package unless the caller invalidates by hand."] + notes
        text = "\n".join(lines) + "\n"
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
        return text

    report()                                                  # the times are on disk before the profiler is tried
    if not args.no_profiler:
        for label, _, _ in routes[:4]:
            if label in results and results[label]["opt"] is not None:
                results[label]["launches"] = count_launches(results[label]["opt"])
    print(report())


if __name__ == "__main__":
    main()
