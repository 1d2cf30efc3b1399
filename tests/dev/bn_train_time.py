"""Times of training-mode BatchNorm on one MI355X: the training-statistics forward and forward + backward beside the eval-mode ones
in the same run, every library call of one training forward + backward by HIP events with the bytes each csrc/bn_train.hip kernel
moves, and the four map kernels beside hps_relu_gate_pad on the stem's map (64 x 128 x 128 x 64).

    python tests/dev/bn_train_time.py [--batch 64] [--size 256] [--out profiles/bn_train_time.txt]

Whole calls: 3 warm-up rounds, then the median of 10 rounds (events around the forward and around the backward, host work included).
Call list: one more round with an event pair around every call into the library (a call = its launches, e.g. hps_bn_batch_stats with its
finish pass).  Bytes: the maps a call reads and writes once (4 B H W C per map; the per-channel vectors and the chunk partials are
not counted).  Rates are given as a fraction of the 8 TB/s HBM peak."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from hierarchicalprobabilistic3dhuman_amd import _capi  # noqa: E402
import encoder_grad_scenario as ES  # noqa: E402

HBM_PEAK = 8.0e12
WARMUP, ROUNDS = 3, 10
P = _capi.ptr
D = lambda t: _capi.ptr(t, torch.float64)
med = lambda v: sorted(v)[len(v) // 2]


def one_round(enc, x, cot):
    enc.zero_grad(set_to_none=True)
    xd = x.detach().requires_grad_(True)
    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    e[0].record()
    feats = enc(xd)
    e[1].record()
    feats.backward(cot)
    e[2].record()
    torch.cuda.synchronize()
    return e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2])


def whole(enc, x, cot):
    t = [one_round(enc, x, cot) for _ in range(WARMUP + ROUNDS)][WARMUP:]
    return med([a for a, _ in t]), med([b for _, b in t])


def plain_forward(enc, x):
    with torch.no_grad():
        for _ in range(WARMUP):
            enc(x)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(ROUNDS):
            enc(x)
        e1.record()
        torch.cuda.synchronize()
    return e0.elapsed_time(e1) / ROUNDS


def call_list(enc, x, cot):
    log, real = [], _capi.call

    def timed_call(name, *args):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        real(name, *args)
        e1.record()
        log.append((name, e0, e1, args))

    _capi.call = timed_call
    try:
        one_round(enc, x, cot)
    finally:
        _capi.call = real
    return [(n, e0.elapsed_time(e1), a) for n, e0, e1, a in log]


def maps_moved(name, a):
    """Number of B H W C maps a csrc/bn_train.hip call (or hps_relu_gate_pad) reads and writes, and (B, H, W, C)."""
    if name == "hps_bn_batch_stats":
        return 1, a[4:8]
    if name == "hps_bn_apply_act_pad":
        return 2 + (a[3] is not None), a[5:9]
    if name == "hps_bn_train_backward_sums":
        return 2 + 2 * (a[2] is not None), a[7:11]
    if name == "hps_bn_train_backward_dz":
        return 3, a[7:11]
    if name == "hps_relu_gate_pad":
        return 3, a[4:8]
    return None, None


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


def stem_map_kernels(dev):
    """[(label, maps moved, ms)] of the four map kernels and hps_relu_gate_pad on 64 x 128 x 128 x 64 (plain frames, as the stem's)."""
    B, H, W, C = 64, 128, 128, 64
    lib, s = _capi.load(), _capi.stream()
    gen = torch.Generator().manual_seed(0)
    z, g, y = (torch.randn(B, H, W, C, generator=gen).to(dev) for _ in range(3))
    out = torch.empty_like(z)
    scale, shift, gamma = (torch.rand(C, generator=gen).to(dev) + 0.5 for _ in range(3))
    mean, var, invstd, sums = (torch.zeros(n, device=dev, dtype=torch.float64) for n in (C, C, C, 2 * C))
    ws = torch.empty(lib.hps_bn_batch_stats_workspace(B, H, W, C) // 8, device=dev, dtype=torch.float64)
    gws = torch.empty(lib.hps_relu_gate_workspace(B, H, W, C) // 8, device=dev, dtype=torch.float64)
    gsum = torch.empty(C, device=dev)
    rows = [("hps_relu_gate_pad (with sums)", 3, timed(lambda: _capi.call("hps_relu_gate_pad", P(g), P(y), D(gws), P(gsum), B, H, W, C, 0, 0, s))),
            ("hps_relu_gate_pad (gate alone)", 3, timed(lambda: _capi.call("hps_relu_gate_pad", P(g), P(y), None, None, B, H, W, C, 0, 0, s))),
            ("hps_bn_batch_stats", 1, timed(lambda: _capi.call("hps_bn_batch_stats", P(z), D(ws), D(mean), D(var), B, H, W, C, 0, s)))]
    invstd.copy_(1.0 / torch.sqrt(var + 1e-5))
    rows += [("hps_bn_apply_act_pad (relu)", 2, timed(lambda: _capi.call("hps_bn_apply_act_pad", P(z), P(scale), P(shift), None, P(out), B, H, W,
                                                                         C, 0, 0, 1, s))),
             ("hps_bn_apply_act_pad (residual, relu)", 3, timed(lambda: _capi.call("hps_bn_apply_act_pad", P(z), P(scale), P(shift), P(y), P(out),
                                                                                   B, H, W, C, 0, 0, 1, s))),
             ("hps_bn_train_backward_sums (gate)", 4, timed(lambda: _capi.call("hps_bn_train_backward_sums", P(g), P(z), P(y), D(mean), D(invstd),
                                                                               D(ws), D(sums), B, H, W, C, 0, 0, 0, s))),
             ("hps_bn_train_backward_sums (no gate)", 2, timed(lambda: _capi.call("hps_bn_train_backward_sums", P(g), P(z), None, D(mean),
                                                                                  D(invstd), D(ws), D(sums), B, H, W, C, 0, 0, 0, s))),
             ("hps_bn_train_backward_dz", 3, timed(lambda: _capi.call("hps_bn_train_backward_dz", P(g), P(z), D(mean), D(invstd), P(gamma), D(sums),
                                                                      P(out), B, H, W, C, 0, 0, 0, s)))]
    return rows, 4.0 * B * H * W * C


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bn_train_time.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    B, S = args.batch, args.size
    g = torch.Generator().manual_seed(0)
    x, cot = torch.rand(B, 18, S, S, generator=g).to(dev), torch.randn(B, 512, generator=g).to(dev)
    lines = ["Training-mode BatchNorm on one MI355X (gfx950): ResNet-18, input %d x 18 x %d x %d, default kernels." % (B, S, S),
             "tests/dev/bn_train_time.py: HIP events; whole calls = median of %d rounds after %d warm-up rounds; the call list is one further"
             % (ROUNDS, WARMUP), "round with an event pair around every call into the library.", ""]
    ev = ES.make_encoder(18).to(dev)
    tr = ES.make_encoder(18).to(dev)
    tr.set_batchnorm_training(True)
    tr.train()
    lines.append("eval mode:      no_grad forward %9.3f ms" % plain_forward(ev, x))
    f, b = whole(ev, x, cot)
    lines.append("eval mode:      differentiable forward %9.3f ms, backward %9.3f ms, together %9.3f ms" % (f, b, f + b))
    lines.append("training mode:  no_grad forward %9.3f ms" % plain_forward(tr, x))
    f2, b2 = whole(tr, x, cot)
    lines.append("training mode:  differentiable forward %9.3f ms, backward %9.3f ms, together %9.3f ms = %.2f x eval mode"
                 % (f2, b2, f2 + b2, (f2 + b2) / (f + b)))
    calls = call_list(tr, x, cot)
    lines += ["", "every library call of one training-mode forward + backward (all parameters and the input), in order:"]
    total, by_name = 0.0, {}
    for name, ms, a in calls:
        n_maps, shape = maps_moved(name, a)
        note = ""
        if n_maps:
            Bc, H, W, C = shape
            nbytes = 4.0 * Bc * H * W * C * n_maps
            note = "  %3d x %3d x %3d x %3d  %d maps %8.1f MB  %6.2f TB/s = %.3f of 8 TB/s" % (
                Bc, H, W, C, n_maps, nbytes / 1e6, nbytes / (ms * 1e-3) / 1e12, nbytes / (ms * 1e-3) / HBM_PEAK)
        lines.append("  %-32s %9.3f ms%s" % (name, ms, note))
        total += ms
        n0, t0, b0 = by_name.get(name, (0, 0.0, 0.0))
        by_name[name] = (n0 + 1, t0 + ms, b0 + (nbytes if n_maps else 0.0))
    lines += ["", "by entry point:"]
    for name, (n, ms, nbytes) in sorted(by_name.items(), key=lambda kv: -kv[1][1]):
        rate = "  %8.1f MB  %.3f of 8 TB/s" % (nbytes / 1e6, nbytes / (ms * 1e-3) / HBM_PEAK) if nbytes else ""
        lines.append("  %-32s %3d calls %9.3f ms  %5.1f %%%s" % (name, n, ms, 100.0 * ms / total, rate))
    lines.append("  %-32s           %9.3f ms" % ("all library calls", total))
    rows, map_bytes = stem_map_kernels(dev)
    lines += ["", "the map kernels on the stem's map, 64 x 128 x 128 x 64 (%.1f MB per map), median of %d calls after %d:" % (map_bytes / 1e6, ROUNDS, WARMUP)]
    gate_rate = None
    for label, n_maps, ms in rows:
        rate = n_maps * map_bytes / (ms * 1e-3)
        if gate_rate is None:
            gate_rate = rate
        lines.append("  %-40s %d maps %9.3f ms  %6.2f TB/s = %.3f of 8 TB/s = %6.2f x hps_relu_gate_pad (with sums)"
                     % (label, n_maps, ms, rate / 1e12, rate / HBM_PEAK, rate / gate_rate))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
