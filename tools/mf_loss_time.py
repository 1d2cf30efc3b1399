"""Times the device matrix-Fisher loss at the training shape (B = 72, Ns = 9, 6890 vertices; tests/mf_loss_scenario.py case b72) with
HIP events, median over --iters after --warmup, and prints one JSON line:
  forward_ms            PoseMFShapeGaussianLoss forward (2 launches)
  forward_backward_ms   forward + backward (3 launches)
  lognorm_fwd_bwd_ms    LogMFNormConstant forward + backward alone on 72 * 23 rows

    python tools/mf_loss_time.py [--iters 200] [--warmup 20]
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/mf_loss_time.py --trace   # one forward + backward after a warm-up
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import mf_loss_scenario as SC  # noqa: E402
from hierarchicalprobabilistic3dhuman_amd.matrix_fisher_loss import LogMFNormConstant, PoseMFShapeGaussianLoss  # noqa: E402


def median_ms(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--trace", action="store_true", help="warm up, then run exactly one forward + backward (for a kernel trace)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    pred, target = SC.loss_inputs("b72")
    target_dict, pred_dict, leaves = SC.make_dicts(pred, target, device=dev)
    loss = PoseMFShapeGaussianLoss(SC.loss_config("b72"), SC.IMG_WH)
    one = torch.ones((), device=dev)

    def fwd():
        with torch.no_grad():
            loss(target_dict, pred_dict)

    def fwd_bwd():                          # gradients start from None, as after optimiser.zero_grad(): no accumulation kernels
        for leaf in leaves:
            leaf.grad = None
        torch.autograd.backward(loss(target_dict, pred_dict), one)

    S = pred["pose_params_S"].reshape(-1, 3).to(dev).requires_grad_(True)
    ones = torch.ones(S.shape[0], device=dev)

    def lognorm():
        S.grad = None
        torch.autograd.backward(LogMFNormConstant.apply(S), ones)

    if args.trace:
        for _ in range(3):
            fwd_bwd()
            lognorm()
        torch.cuda.synchronize()
        fwd_bwd()
        torch.cuda.synchronize()
        print(json.dumps({"traced": "one forward + backward after 3 warm-up rounds of loss and LogMFNormConstant"}))
        return
    res = {"shape": {"B": 72, "Ns": 9, "V": 6890, "rows": S.shape[0]},
           "forward_ms": median_ms(fwd, args.warmup, args.iters),
           "forward_backward_ms": median_ms(fwd_bwd, args.warmup, args.iters),
           "lognorm_fwd_bwd_ms": median_ms(lognorm, args.warmup, args.iters),
           "iters": args.iters, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
