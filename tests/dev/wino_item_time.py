"""Per-layer time of the Winograd kernel's item loop (hps_dev_conv3x3_winograd, ablate = 0: the product form) against the loop and epilogue it
replaced (ablate = 50), interleaved: the four stride-1 geometries of the ResNet-18 encoder at B = 64, with and without residual, REPS rounds
of ITERS launches per arm; prints each arm's median and spread and checks that both arms write the same bits.  Dev library.

HPS_DEV_LIB_ALT=<path> adds the same two arms from a second build of the dev library (for instance one with other per-file flags for
conv_wino.hip), timed in the same rounds.

usage: wino_item_time.py [REPS [ITERS]]"""
import ctypes
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from hierarchicalprobabilistic3dhuman_amd import _capi  # noqa: E402
from hierarchicalprobabilistic3dhuman_amd.resnet import _ConvBN  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
ITERS = int(sys.argv[2]) if len(sys.argv) > 2 else 30
dev = torch.device("cuda:0")
P = _capi.ptr
_V, _I = ctypes.c_void_p, ctypes.c_int
ARGTYPES = [_V] * 6 + [_I] * 8 + [_V, _I, _V]

libs = [("", _capi.load(dev=True))]
if os.environ.get("HPS_DEV_LIB_ALT"):
    alt = ctypes.CDLL(os.environ["HPS_DEV_LIB_ALT"])
    alt.hps_dev_conv3x3_winograd.argtypes = ARGTYPES
    libs.append((" (alt)", alt))


def timeit(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(ITERS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / ITERS


torch.manual_seed(0)
B = 64
for (H, C) in ((64, 64), (32, 128), (16, 256), (8, 512)):
    conv = torch.nn.Conv2d(C, C, 3, 1, 1, bias=False).to(dev)
    bn = torch.nn.BatchNorm2d(C).eval().to(dev)
    bn.running_mean.normal_(); bn.running_var.uniform_(0.5, 2.0)
    cb = _ConvBN(conv, bn)
    ws = torch.empty(4 * B * 64 * C, device=dev)               # split-K workspace of the 8 x 8 geometry
    x = F.pad(torch.relu(torch.randn(B, H, H, C, device=dev)), (0, 0, 1, 1, 1, 1)).contiguous()
    res = torch.randn(B, H + 2, H + 2, C, device=dev)
    for use_res in (False, True):
        arms = [(tag, lib, ab) for tag, lib in libs for ab in (50, 0)]
        outs = [torch.zeros(B, H + 2, H + 2, C, device=dev) for _ in arms]

        def launch(k):
            tag, lib, ab = arms[k]
            rc = lib.hps_dev_conv3x3_winograd(P(x), P(cb.wino_u), P(cb.scale), P(cb.shift), P(res) if use_res else None, P(outs[k]),
                                              B, H, H, 1, C, C, 1, 1, P(ws) if H == 8 else None, ab, _capi.stream())
            assert rc == 0, (tag, ab, rc)

        for k in range(len(arms)):
            launch(k)
        torch.cuda.synchronize()
        same = all(torch.equal(outs[0], o) for o in outs[1:])
        ts = [[] for _ in arms]
        for rep in range(REPS):
            for k in range(len(arms)):
                ts[k].append(timeit(lambda: launch(k)))
        line = "%2dx%-2d C=%3d B=%d residual=%d identical=%s:" % (H, H, C, B, use_res, same)
        for k, (tag, lib, ab) in enumerate(arms):
            line += "  %s%s %.4f ms [%.4f .. %.4f]" % ("earlier loop" if ab == 50 else "product", tag, statistics.median(ts[k]), min(ts[k]), max(ts[k]))
        base = statistics.median(ts[0])
        line += "  | product vs earlier: " + ", ".join("%+.1f %%" % (100 * (statistics.median(ts[k]) / base - 1)) for k in range(1, len(arms)))
        print(line, flush=True)
