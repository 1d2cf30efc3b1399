"""Times of the encoder backward on one MI355X: ResNet.forward under autograd and its backward, timed in the same run, every
library call of one forward + backward by HIP events, and the weight-gradient GEMMs against the sustained fp32 MFMA rate.

    python tests/dev/encoder_backward_time.py [--batch 64] [--size 256] [--out profiles/encoder_backward_time.txt]

Whole calls: 3 warm-up rounds, then the median of 10 rounds (events around the forward and around the backward, host work included).
Call list: one more round with an event pair around every call into the library (a call = its launches, e.g. hps_conv_wgrad with its
finish pass; the recompute is hps_encoder_run); what the list does not cover is torch glue (the fold-backward's small tensor
operations, allocations).  Weight-gradient rate: 2 B Ho Wo Cout KH KW Cin FLOP per layer against 153.7 TF/s."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from hierarchicalprobabilistic3dhuman_amd import _capi  # noqa: E402
import encoder_grad_scenario as ES  # noqa: E402

MFMA_F32_SUSTAINED = 153.7e12
WARMUP, ROUNDS = 3, 10


def one_round(enc, x, cot, input_grad):
    enc.zero_grad(set_to_none=True)
    xd = x.detach().requires_grad_(input_grad)
    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    e[0].record()
    feats = enc(xd)
    e[1].record()
    feats.backward(cot)
    e[2].record()
    torch.cuda.synchronize()
    return e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2])


def whole(enc, x, cot, input_grad):
    t = [one_round(enc, x, cot, input_grad) for _ in range(WARMUP + ROUNDS)][WARMUP:]
    med = lambda v: sorted(v)[len(v) // 2]
    return med([a for a, _ in t]), med([b for _, b in t])


def call_list(enc, x, cot):
    """[(name, ms, args)] of every library call of one forward + backward, in order."""
    log, real = [], _capi.call

    def timed_call(name, *args):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        real(name, *args)
        e1.record()
        log.append((name, e0, e1, args))

    _capi.call = timed_call
    try:
        one_round(enc, x, cot, True)
    finally:
        _capi.call = real
    return [(n, e0.elapsed_time(e1), a) for n, e0, e1, a in log]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encoder_backward_time.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    enc = ES.make_encoder(18).to(dev)
    B, D = args.batch, args.size
    g = torch.Generator().manual_seed(0)
    x, cot = torch.rand(B, 18, D, D, generator=g).to(dev), torch.randn(B, 512, generator=g).to(dev)
    lines = ["Encoder backward on one MI355X (gfx950): ResNet-18, input %d x 18 x %d x %d, eval-mode BatchNorm, default kernels." % (B, D, D),
             "tests/dev/encoder_backward_time.py: HIP events; whole calls = median of %d rounds after %d warm-up rounds, forward and backward"
             % (ROUNDS, WARMUP),
             "timed in the same round; the call list is one further round with an event pair around every call into the library.", ""]
    with torch.no_grad():
        for _ in range(WARMUP):
            enc(x)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(ROUNDS):
            enc(x)
        e1.record()
        torch.cuda.synchronize()
        plain = e0.elapsed_time(e1) / ROUNDS
    lines.append("no_grad forward (back to back)                         %9.3f ms" % plain)
    for input_grad, what in ((True, "all parameters and the input"), (False, "all parameters, frozen input")):
        fwd, bwd = whole(enc, x, cot, input_grad)
        lines.append("gradients of %-32s forward %9.3f ms, backward %9.3f ms = %.2f x the forward" % (what + ":", fwd, bwd, bwd / fwd))
    enc.requires_grad_(False)
    fwd, bwd = whole(enc, x, cot, True)
    lines.append("gradients of %-32s forward %9.3f ms, backward %9.3f ms = %.2f x the forward" % ("the input alone (frozen encoder):", fwd, bwd, bwd / fwd))
    enc.requires_grad_(True)
    calls = call_list(enc, x, cot)
    lines += ["", "every library call of one forward + backward (all parameters and the input), in order:"]
    total, by_name, wgrad_flop, wgrad_ms = 0.0, {}, 0.0, 0.0
    for name, ms, a in calls:
        note = ""
        if name in ("hps_conv_wgrad", "hps_conv_dgrad"):
            if name == "hps_conv_wgrad":
                Bc, H, W, _, _, cin, cout, kh, kw, stride, pad = a[4:15]
            else:
                Bc, H, W, cin, cout, kh, kw, stride, pad = a[4:13]
            ho, wo = (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kw) // stride + 1
            flop = 2.0 * Bc * ho * wo * cout * kh * kw * cin
            note = "  %3d -> %3d  %dx%d / %d  %3d x %3d -> %3d x %3d  %6.2f GFLOP  %6.1f TF/s = %.3f of the sustained fp32 MFMA rate" % (
                cin, cout, kh, kw, stride, H, W, ho, wo, flop / 1e9, flop / ms / 1e9, flop / (ms * 1e-3) / MFMA_F32_SUSTAINED)
            if name == "hps_conv_wgrad":
                wgrad_flop, wgrad_ms = wgrad_flop + flop, wgrad_ms + ms
        lines.append("  %-32s %9.3f ms%s" % (name, ms, note))
        total += ms
        by_name[name] = by_name.get(name, (0, 0.0))
        by_name[name] = (by_name[name][0] + 1, by_name[name][1] + ms)
    lines += ["", "by entry point:"]
    for name, (n, ms) in sorted(by_name.items(), key=lambda kv: -kv[1][1]):
        lines.append("  %-32s %3d calls %9.3f ms  %5.1f %%" % (name, n, ms, 100.0 * ms / total))
    lines.append("  %-32s           %9.3f ms" % ("all library calls", total))
    lines.append("")
    lines.append("weight-gradient GEMMs together: %.1f GFLOP in %.3f ms = %.1f TF/s = %.3f of the sustained fp32 MFMA rate (153.7 TF/s)"
                 % (wgrad_flop / 1e9, wgrad_ms, wgrad_flop / wgrad_ms / 1e9, wgrad_flop / (wgrad_ms * 1e-3) / MFMA_F32_SUSTAINED))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
