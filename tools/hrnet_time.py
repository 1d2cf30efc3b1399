"""W48 forward at (1, 3, 384, 288) and (16, 3, 384, 288): the device module against the same network as plain torch calls in fp32
on the same card.

The stock network is built ONCE before any timing (StockNet below): the structure of tests/hrnet_scenario.forward64 resolved into
lists of prepared layers -- BatchNorm folded into filter and bias in float64, so that a layer is one F.conv2d and one in-place
F.relu -- with no string work, dictionary probing or folding left in a call.  Device events around whole calls, three warm-up calls
of each route, then the routes alternated; medians and quartiles.  Beside the device time of a call, the host time its enqueue takes
(host clock around the call, no synchronise): a route whose enqueue time equals its event time is host-bound.  

    python tools/hrnet_time.py
"""
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))

import hrnet_scenario as S  # noqa: E402
from hierarchicalprobabilistic3dhuman_amd.pose2D_hrnet import PoseHighResolutionNet  # noqa: E402


class StockNet:
    """HRNet from a state dict as prepared torch.nn.functional calls; everything a call needs is resolved here."""

    def __init__(self, sd, cfg, dev):
        self.sd, self.dev = sd, dev
        extra = cfg["MODEL"]["EXTRA"]
        L, has = self.layer, lambda k: k in sd
        self.stem = [L("conv1", "bn1", 2, True), L("conv2", "bn2", 2, True)]
        self.layer1 = [self.block("layer1.%d" % i, "BOTTLENECK") for i in range(4)]
        self.stages = []
        for n in (2, 3, 4):
            st = extra["STAGE%d" % n]
            nb = st["NUM_BRANCHES"]
            trans = []
            for i in range(nb):
                p = "transition%d.%d" % (n - 1, i)
                if has(p + ".0.weight"):
                    trans.append([L(p + ".0", p + ".1", 1, True)])
                elif has(p + ".0.0.weight"):
                    k, steps = 0, []
                    while has("%s.%d.0.weight" % (p, k)):
                        steps.append(L("%s.%d.0" % (p, k), "%s.%d.1" % (p, k), 2, True))
                        k += 1
                    trans.append(steps)
                else:
                    trans.append(None)
            modules = []
            for m in range(st["NUM_MODULES"]):
                mp = "stage%d.%d" % (n, m)
                branches = [[self.block("%s.branches.%d.%d" % (mp, i, b), st["BLOCK"]) for b in range(st["NUM_BLOCKS"][i])] for i in range(nb)]
                rows = []
                for i in range(nb):
                    if nb == 1 or not any(k.startswith("%s.fuse_layers.%d." % (mp, i)) for k in sd):
                        continue
                    row = []
                    for j in range(nb):
                        p = "%s.fuse_layers.%d.%d" % (mp, i, j)
                        if j == i:
                            row.append(None)
                        elif j > i:
                            row.append(([L(p + ".0", p + ".1", 1, False)], 2 ** (j - i)))
                        else:
                            row.append(([L("%s.%d.0" % (p, k), "%s.%d.1" % (p, k), 2, k != i - j - 1) for k in range(i - j)], 0))
                    rows.append(row)
                modules.append((branches, rows))
            self.stages.append((trans, modules))
        w = sd["final_layer.weight"]
        self.final = (w.to(dev), sd["final_layer.bias"].to(dev), 1, w.shape[-1] // 2, False)

    def layer(self, conv, bn, stride, relu):
        sd = self.sd
        w = sd[conv + ".weight"]
        scale = sd[bn + ".weight"].double() / torch.sqrt(sd[bn + ".running_var"].double() + S.BN_EPS)
        shift = sd[bn + ".bias"].double() - sd[bn + ".running_mean"].double() * scale
        return ((w.double() * scale.view(-1, 1, 1, 1)).float().to(self.dev), shift.float().to(self.dev), stride, w.shape[-1] // 2, relu)

    def block(self, p, kind):
        names = ("1", "2") if kind == "BASIC" else ("1", "2", "3")
        main = [self.layer("%s.conv%s" % (p, n), "%s.bn%s" % (p, n), 1, n != names[-1]) for n in names]
        down = self.layer(p + ".downsample.0", p + ".downsample.1", 1, False) if p + ".downsample.0.weight" in self.sd else None
        return main, down

    @staticmethod
    def run(layers, t):
        for w, b, stride, pad, relu in layers:
            t = F.conv2d(t, w, b, stride, pad)
            if relu:
                t = F.relu_(t)
        return t

    def __call__(self, x):
        run = self.run

        def blocks(stack, t):
            for main, down in stack:
                t = F.relu_(run(main, t) + (t if down is None else run([down], t)))
            return t

        ys = [blocks(self.layer1, run(self.stem, x))]
        for trans, modules in self.stages:
            xs = [ys[i] if t is None else run(t, ys[-1]) for i, t in enumerate(trans)]
            for branches, rows in modules:
                xs = [blocks(br, t) for br, t in zip(branches, xs)]
                if not rows:
                    continue
                out = []
                for i, row in enumerate(rows):
                    total = None
                    for j, cell in enumerate(row):
                        if cell is None:
                            term = xs[j]
                        else:
                            term = run(cell[0], xs[j])
                            if cell[1]:
                                term = F.interpolate(term, scale_factor=cell[1], mode="nearest")
                        total = term if total is None else total + term
                    out.append(F.relu_(total))
                xs = out
            ys = xs
        return run([self.final], ys[0])


def main():
    dev = torch.device("cuda:0")
    keys = json.load(open(os.path.join(ROOT, "tests", "golden", "hrnet_w48_keys.json")))
    sd = S.seeded_state_dict({k: (tuple(s), d) for k, s, d in keys}, S.W48_SEED)
    cfg = S.config("W48")
    net = PoseHighResolutionNet(cfg).eval()
    net.load_state_dict(sd, strict=True)
    net = net.to(dev)
    stock = StockNet(sd, cfg, dev)
    out = {}
    with torch.no_grad():
        xc = S.seeded_input((1, 3, 384, 288), 0)
        y64 = S.forward64(sd, cfg, xc.double())
        e_stock = float((stock(xc.to(dev)).cpu().double() - y64).abs().max())
        e_ours = float((net(xc.to(dev)).cpu().double() - y64).abs().max())
        print("against float64 at B = 1: max|ours - f64| = %.3e  max|stock - f64| = %.3e  max|y64| = %.3e" % (e_ours, e_stock, float(y64.abs().max())), flush=True)
        assert e_stock < 1e-4 * float(y64.abs().max()), "the stock network does not compute the network"
        for B, iters in ((1, 60), (16, 24)):
            x = S.seeded_input((B, 3, 384, 288), 0).to(dev)
            routes = (("ours", lambda: net(x)), ("stock", lambda: stock(x)))
            for _ in range(3):
                for _, fn in routes:
                    fn()
            torch.cuda.synchronize()
            dev_ms, host_ms = {"ours": [], "stock": []}, {"ours": [], "stock": []}
            for _ in range(iters):
                for name, fn in routes:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0 = time.perf_counter()
                    e0.record()
                    fn()
                    e1.record()
                    host_ms[name].append((time.perf_counter() - t0) * 1e3)
                    e1.synchronize()
                    dev_ms[name].append(e0.elapsed_time(e1))
            res = {"launches": net.launches_per_forward(B, 384, 288, dev)}
            for name in ("ours", "stock"):
                q = statistics.quantiles(dev_ms[name], n=4)
                res[name + "_ms"], res[name + "_q"] = statistics.median(dev_ms[name]), (q[0], q[2])
                res[name + "_enqueue_ms"] = statistics.median(host_ms[name])
            out["B%d" % B] = res
            print("B=%d" % B, res, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
