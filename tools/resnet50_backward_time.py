"""The backward of the ResNet-50 encoder at the training shape, B = 72 x 18 x 256 x 256, on one MI355X.

1. Per distinct 1x1 layer shape of ResNet-50 (tests/resnet50_grad_scenario.resnet50_1x1_layers): hps_conv_dgrad / hps_conv_wgrad
   against hps_conv1x1_dgrad / hps_conv1x1_wgrad through the C ABI on the same frames (halo 1, as the encoder's), HIP events around
   every call, 3 warm-up rounds, then 15 timed rounds with the four kernels alternated; median and quartiles.  ``routed``: the new
   kernel's upper quartile lies below the old kernel's lower quartile -- the condition of ResNet._gemm_dgrad / _gemm_wgrad
   (DESIGN.md section 4).  The data gradients are compared bit for bit on the way.
2. The whole encoder, forward + backward of <cot, features> with respect to the input and every parameter, eval-mode BatchNorm:
   the device module with gemm_backward on and off against the same network as BatchNorm-folded torch.nn.functional calls under torch
   autograd in fp32 on the same card; host clock from the call to the end of a device synchronise, 2 warm-up rounds, 10 timed rounds,
   routes alternated; ``device_train_bn``: the device module with every BatchNorm on batch statistics (no torch route beside it: the
   folded network has no BatchNorm left).  The ResNet-18 encoder's line from the same run beside it.  

    python tools/resnet50_backward_time.py [--batch 72] [--skip-encoder]
"""
import argparse
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

import resnet50_grad_scenario as GS  # noqa: E402
import resnet50_scenario as S  # noqa: E402
from hierarchicalprobabilistic3dhuman_amd import _capi  # noqa: E402
from hierarchicalprobabilistic3dhuman_amd.resnet import resnet18  # noqa: E402


def quartiles(v):
    q = statistics.quantiles(v, n=4)
    return {"median_ms": round(statistics.median(v), 4), "q1_ms": round(q[0], 4), "q3_ms": round(q[2], 4)}


def layer_table(B, dev, warm=3, rounds=15):
    lib, P, s = _capi.load(), _capi.ptr, _capi.stream()
    rows = []
    for cin, cout, stride, hw in GS.resnet50_1x1_layers():
        ho = (hw - 1) // stride + 1
        gen = torch.Generator(device=dev).manual_seed(cin + cout + hw)
        xf = torch.randn(B, hw + 2, hw + 2, cin, device=dev, generator=gen)
        gf = torch.randn(B, ho + 2, ho + 2, cout, device=dev, generator=gen)
        wt = torch.randn(cout, cin, device=dev, generator=gen) / cout ** 0.5
        dx = [torch.zeros_like(xf), torch.zeros_like(xf)]
        G = [torch.empty(cout, cin, device=dev), torch.empty(cout, cin, device=dev)]
        ws = [torch.empty(int(lib.hps_conv_wgrad_workspace(B, hw, hw, cin, cout, 1, 1, stride, 0)) // 4, device=dev),
              torch.empty(int(lib.hps_conv1x1_wgrad_workspace(B, hw, hw, cin, cout, stride)) // 4, device=dev)]
        calls = {
            "dgrad_old": lambda: _capi.call("hps_conv_dgrad", P(gf), P(wt), None, P(dx[0]), B, hw, hw, cin, cout, 1, 1, stride, 0, 1, 1, cin, s),
            "dgrad_new": lambda: _capi.call("hps_conv1x1_dgrad", P(gf), P(wt), None, P(dx[1]), B, hw, hw, cin, cout, stride, 1, 1, cin, s),
            "wgrad_old": lambda: _capi.call("hps_conv_wgrad", P(xf), P(gf), P(G[0]), P(ws[0]), B, hw, hw, 1, cin, cin, cout, 1, 1, stride, 0, 1, s),
            "wgrad_new": lambda: _capi.call("hps_conv1x1_wgrad", P(xf), P(gf), P(G[1]), P(ws[1]), B, hw, hw, 1, cin, cin, cout, stride, 1, s),
        }
        ms = {k: [] for k in calls}
        for r in range(warm + rounds):
            for k, fn in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if r >= warm:
                    ms[k].append(e0.elapsed_time(e1))
        assert torch.equal(dx[0], dx[1]), "hps_conv1x1_dgrad lost the bits of hps_conv_dgrad"
        rel = float((G[0] - G[1]).abs().max()) / float(G[0].abs().max())
        row = {"cin": cin, "cout": cout, "stride": stride, "map": hw, "gflop": round(2e-9 * B * ho * ho * cin * cout, 3),
               "wgrad_rel_diff": rel, "workspace_mb": [round(w.numel() * 4 / 2 ** 20, 2) for w in ws]}
        for k in calls:
            row[k] = quartiles(ms[k])
        for kind in ("dgrad", "wgrad"):
            row[kind + "_routed"] = row[kind + "_new"]["q3_ms"] < row[kind + "_old"]["q1_ms"]
        rows.append(row)
        print("%4d -> %4d / %d  %2d x %2d  %7.3f GFLOP | dgrad old %7.3f [%7.3f, %7.3f]  new %7.3f [%7.3f, %7.3f] %s | wgrad old %7.3f [%7.3f, %7.3f]"
              "  new %7.3f [%7.3f, %7.3f] %s  (ws %s MB)"
              % (cin, cout, stride, hw, hw, row["gflop"],
                 row["dgrad_old"]["median_ms"], row["dgrad_old"]["q1_ms"], row["dgrad_old"]["q3_ms"],
                 row["dgrad_new"]["median_ms"], row["dgrad_new"]["q1_ms"], row["dgrad_new"]["q3_ms"], "new" if row["dgrad_routed"] else "old",
                 row["wgrad_old"]["median_ms"], row["wgrad_old"]["q1_ms"], row["wgrad_old"]["q3_ms"],
                 row["wgrad_new"]["median_ms"], row["wgrad_new"]["q1_ms"], row["wgrad_new"]["q3_ms"], "new" if row["wgrad_routed"] else "old",
                 row["workspace_mb"]), flush=True)
        del xf, gf, dx, ws
        torch.cuda.empty_cache()
    return rows


class TorchNet:
    """An encoder of this package as prepared torch calls under autograd: BatchNorm folded into filter and bias in float64 (leaves that
    require grad), one F.conv2d per layer."""

    def __init__(self, enc, dev):
        def layer(conv, bn):
            scale = bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps)
            shift = bn.bias.detach().double() - bn.running_mean.double() * scale
            w = (conv.weight.detach().double() * scale.view(-1, 1, 1, 1)).float().to(dev).requires_grad_(True)
            return w, shift.float().to(dev).requires_grad_(True), conv.stride[0], conv.padding[0]

        self.stem = layer(enc.conv1, enc.bn1)
        self.blocks = []
        for stage in (enc.layer1, enc.layer2, enc.layer3, enc.layer4):
            for blk in stage:
                n = 3 if hasattr(blk, "conv3") else 2
                convs = [layer(getattr(blk, "conv%d" % i), getattr(blk, "bn%d" % i)) for i in range(1, n + 1)]
                self.blocks.append((convs, layer(blk.downsample[0], blk.downsample[1]) if blk.downsample is not None else None))
        self.leaves = [t for l in [self.stem] + [c for convs, d in self.blocks for c in convs + ([d] if d else [])] for t in l[:2]]

    def __call__(self, x):
        y = F.max_pool2d(F.relu(F.conv2d(x, *self.stem)), 3, 2, 1)
        for convs, down in self.blocks:
            t = y
            for c in convs[:-1]:
                t = F.relu(F.conv2d(t, *c))
            y = F.relu(F.conv2d(t, *convs[-1]) + (y if down is None else F.conv2d(y, *down)))
        return y.mean(dim=(2, 3))


def step_times(B, dev, warm=2, rounds=10):
    out = {}
    x = S.seeded_input((B, 18, 256, 256), 3).to(dev)
    for label in ("resnet50", "resnet18"):
        if label == "resnet50":
            enc = S.build_encoder(S.FULL_LAYERS, S.case("production")[0])
            enc.set_differentiable(True)
        else:
            torch.manual_seed(0)
            enc = resnet18(18).eval()
        stock = TorchNet(enc, dev)
        enc = enc.to(dev)
        width = 512 * enc.block.expansion
        cot = torch.randn(B, width, device=dev, generator=torch.Generator(device=dev).manual_seed(5))

        def device_step(train=False, gemm=True):
            enc.gemm_backward = gemm
            enc.train(train)
            enc.zero_grad(set_to_none=True)
            xd = x.detach().requires_grad_(True)
            (cot * enc(xd)).sum().backward()

        def torch_step():
            xd = x.detach().requires_grad_(True)
            torch.autograd.grad((cot * stock(xd)).sum(), [xd] + stock.leaves)

        enc.set_batchnorm_training(True)               # (with no BatchNorm in training mode the eval launches are issued)
        routes = [("device", device_step), ("device_gemm_off", lambda: device_step(gemm=False)),
                  ("device_train_bn", lambda: device_step(train=True)), ("torch", torch_step)]
        ms = {n: [] for n, _ in routes}
        for r in range(warm + rounds):
            for n, fn in routes:
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if r >= warm:
                    ms[n].append((time.perf_counter() - t0) * 1e3)
        out[label] = {n: quartiles(v) for n, v in ms.items()}
        print(label, "forward + backward at B = %d:" % B, json.dumps(out[label]), flush=True)
        enc.train(False)
        del enc, stock
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=72)
    ap.add_argument("--skip-encoder", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"batch": args.batch, "layers": layer_table(args.batch, dev)}
    if not args.skip_encoder:
        out["steps"] = step_times(args.batch, dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
