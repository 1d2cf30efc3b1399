"""ResNet-50 encoder forward on (B, 18, 256, 256), B = 1, 16, 64, on one MI355X: the routes of the device module against each other
and against the same network as BatchNorm-folded torch.nn.functional calls in fp32 on the same card.

Routes: ``fold`` (the default: Winograd 3x3 layers, entry blocks through hps_bottleneck_expand_down), ``two_launch``
(fold_downsample off), ``direct`` (set_winograd(False)), at B = 1 also ``latency`` (set_latency_mode), and ``torch``.  Every route has
a module of its own (a switch rebuilds the device state), the weights are tests/resnet50_scenario.py's seeded "production" case.
Method: host clock from the call to the end of a device synchronise, 3 warm-up rounds, then 20 timed rounds with the routes
alternated; median and quartiles.  Then, at B = 64, every launch of the default plan on its own (``composite = False``'s entry points,
HIP events around 10 repetitions after 3 warm-up ones), grouped by layer shape: time, algorithmic GFLOP (2 x multiply-adds) and TF/s
against the 153.7 TF/s fp32 matrix ceiling.  Printed too: multiply-adds per image, launches per forward, bytes of one frame set.


    python tools/resnet50_time.py
"""
import collections
import copy
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

import resnet50_scenario as S  # noqa: E402
from hierarchicalprobabilistic3dhuman_amd import _capi  # noqa: E402

PEAK_TFLOPS = 153.7
KIND_NAMES = {_capi.ENC_CONV: "direct", _capi.ENC_CONV_WINOGRAD: "winograd", _capi.ENC_EXPAND_DOWN: "expand+down",
              _capi.ENC_STEM_WINOGRAD_POOLED_NCHW: "stem+pool", _capi.ENC_AVGPOOL: "avgpool"}


class TorchNet:
    """The encoder from a state dict as prepared torch calls: BatchNorm folded into filter and bias in float64, one F.conv2d per layer."""

    def __init__(self, sd, dev):
        def layer(conv, bn, stride, pad):
            w = sd[conv + ".weight"]
            scale = sd[bn + ".weight"].double() / torch.sqrt(sd[bn + ".running_var"].double() + S.BN_EPS)
            shift = sd[bn + ".bias"].double() - sd[bn + ".running_mean"].double() * scale
            return (w.double() * scale.view(-1, 1, 1, 1)).float().to(dev), shift.float().to(dev), stride, pad

        self.stem = layer("conv1", "bn1", 2, 3)
        self.blocks = []
        for li, blocks in enumerate(S.layers_of(sd), 1):
            for bi in range(blocks):
                p = "layer%d.%d." % (li, bi)
                s = 2 if li > 1 and bi == 0 else 1
                down = layer(p + "downsample.0", p + "downsample.1", s, 0) if p + "downsample.0.weight" in sd else None
                self.blocks.append((layer(p + "conv1", p + "bn1", 1, 0), layer(p + "conv2", p + "bn2", s, 1), layer(p + "conv3", p + "bn3", 1, 0), down))

    def __call__(self, x):
        y = F.max_pool2d(F.relu_(F.conv2d(x, *self.stem)), 3, 2, 1)
        for c1, c2, c3, down in self.blocks:
            t = F.conv2d(F.relu_(F.conv2d(F.relu_(F.conv2d(y, *c1)), *c2)), *c3)
            y = F.relu_(t + (y if down is None else F.conv2d(y, *down)))
        return y.mean(dim=(2, 3))


def macs_per_image(enc, H, W):
    maps = enc._layer_maps(H, W)
    return sum(maps[name][0] * maps[name][1] * conv.out_channels * conv.in_channels * conv.kernel_size[0] * conv.kernel_size[1]
               for name, conv, _ in enc._enc_layers())


def frame_set_bytes(fs):
    seen, total = set(), 0
    tensors = [fs.get(k) for k in ("in", "stem", "side", "pool")] + [t for ent in fs["blocks"] for t in ent.values()]
    for t in tensors:
        if isinstance(t, torch.Tensor) and t.data_ptr() not in seen:
            seen.add(t.data_ptr())
            total += t.numel() * t.element_size()
    return total


def timed_rounds(routes, warm=3, rounds=20):
    for _ in range(warm):
        for _, fn in routes:
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in routes}
    for _ in range(rounds):
        for name, fn in routes:
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3)
    out = {}
    for name, v in ms.items():
        q = statistics.quantiles(v, n=4)
        out[name] = {"median_ms": round(statistics.median(v), 4), "q1_ms": round(q[0], 4), "q3_ms": round(q[2], 4)}
    return out


def per_shape_table(enc, x):
    """Every launch of the default plan at this batch on its own: [(shape key, launches, ms per launch, GFLOP per launch, TF/s)]."""
    with torch.no_grad():
        feats = enc(x)
    B, C, H, W = x.shape
    fs = enc._frame_set(enc._prepared, B, C, H, W, x.device)
    ops = fs["ops"]
    ops[0].x, ops[len(ops) - 1].y = x.data_ptr(), feats.data_ptr()
    rows = collections.OrderedDict()
    for i in range(len(ops)):
        op = ops[i]
        for _ in range(3):
            _capi.issue_enc_op(op)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            _capi.issue_enc_op(op)
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1) / 10
        kind = KIND_NAMES.get(op.kind, str(op.kind))
        if op.kind == _capi.ENC_EXPAND_DOWN:
            Ho, Wo = (op.H - 1) // op.stride + 1, (op.W - 1) // op.stride + 1
            macs = B * Ho * Wo * op.Cout * (op.Cin + op.Cin_down)
            key = "%s %dx%d/%d  %d+%d -> %d" % (kind, op.H, op.W, op.stride, op.Cin, op.Cin_down, op.Cout)
        elif op.kind in (_capi.ENC_CONV, _capi.ENC_CONV_WINOGRAD):
            k, s = (3, 1) if op.kind == _capi.ENC_CONV_WINOGRAD else (op.KH, op.stride)
            Ho, Wo = (op.H + 2 * (k // 2) - k) // s + 1, (op.W + 2 * (k // 2) - k) // s + 1
            macs = B * Ho * Wo * op.Cout * op.Cin * k * k
            key = "%s %dx%d %dx%d/%d  %d -> %d" % (kind, k, k, op.H, op.W, s, op.Cin, op.Cout)
        elif op.kind == _capi.ENC_STEM_WINOGRAD_POOLED_NCHW:
            macs = B * (op.H // 2) * (op.W // 2) * 64 * 18 * 49
            key = "%s 7x7 %dx%d/2  18 -> 64" % (kind, op.H, op.W)
        else:
            macs, key = 0, "%s %dx%d  %d" % (kind, op.H, op.W, op.Cin)
        r = rows.setdefault(key, [0, 0.0, macs])
        r[0] += 1
        r[1] += ms
    table = []
    for key, (n, ms, macs) in rows.items():
        per = ms / n
        gflop = 2e-9 * macs
        table.append({"shape": key, "launches": n, "ms": round(per, 4), "gflop": round(gflop, 3),
                      "tflops": round(gflop / per, 1) if per > 0 and macs else None})
    return table


def main():
    dev = torch.device("cuda:0")
    sd, _ = S.case("production")
    base = S.build_encoder(S.FULL_LAYERS, sd)
    enc = {"fold": copy.deepcopy(base).to(dev), "two_launch": copy.deepcopy(base).to(dev), "direct": copy.deepcopy(base).to(dev),
           "latency": copy.deepcopy(base).to(dev)}
    enc["two_launch"].fold_downsample = False
    enc["direct"].set_winograd(False)
    enc["latency"].set_latency_mode(True)
    stock = TorchNet(sd, dev)
    out = {"macs_per_image": macs_per_image(base, 256, 256)}
    print("multiply-adds per 256 x 256 x 18 image: %.4f G" % (out["macs_per_image"] * 1e-9), flush=True)
    with torch.no_grad():
        xc = S.seeded_input((1, 18, 256, 256), 3)
        y64 = S.forward(sd, xc.double())
        for name in ("fold", "two_launch", "direct", "latency"):
            e = float((enc[name](xc.to(dev)).cpu().double() - y64).abs().max())
            print("against float64 at B = 1: %-10s max|dev - f64| = %.3e (max|y64| = %.3e)" % (name, e, float(y64.abs().max())), flush=True)
        e = float((stock(xc.to(dev)).cpu().double() - y64).abs().max())
        print("against float64 at B = 1: torch      max|dev - f64| = %.3e" % e, flush=True)
        assert e < 1e-4 * float(y64.abs().max()), "the torch route does not compute the network"
        assert torch.equal(enc["fold"](xc.to(dev)), enc["two_launch"](xc.to(dev)))
        for B in (1, 16, 64):
            x = S.seeded_input((B, 18, 256, 256), 3).to(dev)
            names = ["fold", "two_launch", "direct"] + (["latency"] if B == 1 else []) + ["torch"]
            routes = [(n, (lambda m=enc[n]: m(x)) if n != "torch" else (lambda: stock(x))) for n in names]
            res = timed_rounds(routes)
            for n in ("fold", "two_launch"):
                fs = enc[n]._frame_set(enc[n]._prepared, B, 18, 256, 256, dev)
                res[n]["launches"], res[n]["frame_set_bytes"] = len(fs["ops"]), frame_set_bytes(fs)
            out["B%d" % B] = res
            print("B=%d" % B, json.dumps(res), flush=True)
            if B != 64:
                for m in enc.values():
                    m.invalidate()                   # the frames of this batch size
                torch.cuda.empty_cache()
        table = per_shape_table(enc["fold"], x)
        out["per_shape_B64"] = table
        print("%-44s %8s %9s %9s %7s" % ("layer shape at B = 64 (default plan)", "launches", "ms/launch", "GFLOP", "TF/s"))
        for r in table:
            print("%-44s %8d %9.4f %9.3f %7s" % (r["shape"], r["launches"], r["ms"], r["gflop"], r["tflops"]))
        print("sum over the launches: %.3f ms; fp32 matrix-pipe floor at %.1f TF/s: %.3f ms"
              % (sum(r["ms"] * r["launches"] for r in table), PEAK_TFLOPS, 2e-9 * out["macs_per_image"] * 64 / PEAK_TFLOPS))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
