"""Times the head (PoseMFShapeGaussianNet.forward on cached features) at B = 1 and at B = 72 (the reference's training batch) with HIP
events, median over --iters after --warmup:
  no_grad_forward_ms    the head under torch.no_grad()
  autograd_forward_ms   the same call under grad mode (torch.autograd.Function around the same launches)
  backward_ms           torch.autograd.backward of the seven differentiable outputs with standard-normal cotangents, gradients reset
                        to None first (as after optimiser.zero_grad())
then runs itself once under `rocprofv3 --kernel-trace --stats` (--trace: one no_grad forward, one grad-mode forward, one backward at
B = 72, separated by a one-element torch kernel as a marker) and writes everything to profiles/head_backward_time.txt.

    python tools/head_backward_time.py [--iters 200] [--warmup 20] [--no-trace]
"""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import head_grad_scenario as HS  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "head_backward_time.txt")
TRACE_B = 72


def median_ms(fn, warmup, iters, before=None):
    times = []
    for i in range(warmup + iters):
        if before is not None:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= warmup:
            times.append(a.elapsed_time(b))
    return statistics.median(times)


class Case:
    def __init__(self, net, B, dev):
        self.net = net
        g = torch.Generator().manual_seed(B)
        self.feats = torch.rand(B, 512, generator=g).to(dev)
        self.cot = [HS.cotangents(B)[k].to(dev) for k in HS.OUTPUTS]
        self.params = [p for k, p in net.named_parameters() if k.startswith(HS.HEAD_PREFIXES)]
        self.outs = None

    def no_grad_forward(self):
        with torch.no_grad():
            self.net(None, input_feats=self.feats)

    def autograd_forward(self):
        pose_F, _, pose_S, _, mode, dist, glob, cam = self.net(None, input_feats=self.feats)
        self.outs = [pose_F, pose_S, mode, dist.loc, dist.scale, glob, cam]

    def reset(self):
        for p in self.params:
            p.grad = None
        self.autograd_forward()

    def backward(self):
        torch.autograd.backward(self.outs, self.cot)


def trace_run(dev):
    """One no_grad forward | one grad-mode forward | one backward at B = TRACE_B, a marker kernel before, between and after."""
    c = Case(HS.make_net("default").to(dev), TRACE_B, dev)
    marker = torch.zeros(1, device=dev)
    for _ in range(3):
        c.no_grad_forward()
        c.reset()
        c.backward()
    for p in c.params:
        p.grad = None
    torch.cuda.synchronize()
    for step in (c.no_grad_forward, c.autograd_forward, c.backward):
        marker.add_(1.0)
        step()
    marker.add_(1.0)
    torch.cuda.synchronize()


def read_trace(directory):
    """The kernels of the three traced segments: [(name, microseconds), ...] per segment, split at the last four marker kernels."""
    paths = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    if not paths:
        raise RuntimeError("rocprofv3 wrote no kernel trace under %s" % directory)
    rows = []
    for path in paths:
        with open(path) as f:
            for r in csv.DictReader(f):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    marks = [i for i, r in enumerate(rows) if "hps::" not in r[2] and "elementwise" in r[2]]
    if len(marks) < 4:
        raise RuntimeError("the kernel trace holds %d marker kernels, expected at least 4" % len(marks))
    m = marks[-4:]
    return [[(name.split("(")[0], (e - s) / 1000.0) for s, e, name in rows[m[i] + 1:m[i + 1]]] for i in range(3)]


def summarise(segment):
    order, total, count = [], {}, {}
    for name, us in segment:
        if name not in total:
            order.append(name)
        total[name] = total.get(name, 0.0) + us
        count[name] = count.get(name, 0) + 1
    return ["    %-72s x%-3d %8.1f us" % (n[:72], count[n], total[n]) for n in order] + [
        "    total: %d launches, %.1f us of kernel time" % (len(segment), sum(us for _, us in segment))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--trace", action="store_true", help="the traced run itself (started by this tool under rocprofv3)")
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 pass")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    if args.trace:
        trace_run(dev)
        return
    net = HS.make_net("default").to(dev)
    lines = ["Head forward and backward on one %s (PoseMFShapeGaussianNet on cached features, seed-0 default weights)." % torch.cuda.get_device_name(0),
             "tools/head_backward_time.py: HIP events around each call, median of %d after %d warm-up calls; the backward starts from" % (args.iters, args.warmup),
             "gradients reset to None and standard-normal cotangents on the seven differentiable outputs.  Times include the Python /",
             "autograd host work of each call; the GPU time alone is the kernel list below.", ""]
    for B in (1, TRACE_B):
        c = Case(net, B, dev)
        res = {"B": B, "no_grad_forward_ms": median_ms(c.no_grad_forward, args.warmup, args.iters),
               "autograd_forward_ms": median_ms(c.autograd_forward, args.warmup, args.iters),
               "backward_ms": median_ms(c.backward, args.warmup, args.iters, before=c.reset), "iters": args.iters, "warmup": args.warmup}
        print(json.dumps(res), flush=True)
        lines.append(json.dumps(res))
    if not args.no_trace:
        rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
        tmp = tempfile.mkdtemp(prefix="head_backward_trace_")
        try:
            cmd = [rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "hb", "--", sys.executable,
                   os.path.abspath(__file__), "--trace"]
            subprocess.run(cmd, check=True, timeout=600, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            fwd, fwd_grad, bwd = read_trace(tmp)
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
        same = [n for n, _ in fwd] == [n for n, _ in fwd_grad]
        only_hps = all(n.startswith("hps::") or " hps::" in n for n, _ in bwd)
        lines += ["", "rocprofv3 --kernel-trace --stats -- python tools/head_backward_time.py --trace   (B = %d, after three warm-up rounds)" % TRACE_B,
                  "  no_grad forward:"] + summarise(fwd) + ["  grad-mode forward:"] + summarise(fwd_grad) + ["  backward:"] + summarise(bwd) + [
                  "  grad-mode forward launches the no_grad kernel list: %s" % same, "  backward launches only hps:: kernels: %s" % only_hps]
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
