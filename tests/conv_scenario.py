"""Seeded cases, CPU references and the accuracy rule of the convolution-kernel tests (tests/test_conv_scenario_host.py,
tests/test_gpu_conv_shapes.py).  Nothing here touches a device.

A case is conv (torch's default init) + eval BatchNorm with non-trivial statistics (the recipe of test_padded_conv_kernel; an odd seed
draws bn.weight from a normal distribution, so some scales are negative) on a (B, Cin, H, W) input, and a residual of the output's
shape.  Three outputs ("modes") are covered:

    "res_relu"  relu(bn(conv(x)) + res)        "lin"  bn(conv(x))        "relu"  relu(bn(conv(x)))    (a block's first convolution)

The truth is y64, the float64 evaluation of the same modules.  The family of legitimate fp32 evaluations it is compared with:

    y_cpu32   torch fp32 on the CPU
    y_seq32   ONE strictly sequential fp32 accumulation over K = k * k * Cin, tap-major then channel: every product formed exactly in
              float64, added to the accumulator in float64 and rounded to fp32 after every addition (a chain of fused multiply-adds);
              scale and shift in fp32.  The worst legitimate fp32 order.  On a fixed seeded sample of at most 20 000 output positions
              that always holds the four corner pixels and one pixel of every border row and column, first and last channel.
    y_wino32  Winograd F(2x2, 3x3) with the textbook G, B^T, A^T: filter transform, input transform, channel sum and output transform
              all in fp32 (3 x 3 / 1 / 1 cases only)

The accuracy rule (smpl_grad_scenario.bound with the family widened; the factor 4 is the project's margin for a summation order other
than the reference's):

    bound = 4 * max(e_cpu32, e_seq32[, e_wino32], 2**-23 * max|y64|)        e_* = max|y_* - y64| over what that reference covers

e_wino32 enters only for launches that run the Winograd kernel.  References are computed once per case and shared: callers must not
modify them.
"""
import copy
import functools

import torch
import torch.nn.functional as F

EPS32 = 2.0 ** -23
MODES = ("res_relu", "lin", "relu")
SAMPLE = 20000


# (B, H, W, Cin, Cout) through csrc/conv_wino.hip (3 x 3 / 1 / 1, ipad 1): one block row with two block columns and the reverse, three
# block rows, blocks_x = 5 with three channel chunks and two output-channel tiles, layer1 of a 256 x 192 crop, an odd item count, the
# long K loop outside the 8 x 8 form, 264 items for 256 workgroups; square controls, the second a partial quad of 8 x 8 maps
WINO_CASES = [(1, 16, 32, 64, 64), (2, 32, 16, 64, 64), (3, 48, 16, 256, 256), (1, 16, 80, 24, 128), (2, 64, 48, 64, 64),
              (5, 16, 32, 128, 128), (1, 16, 48, 512, 512), (11, 64, 48, 64, 128), (2, 32, 32, 128, 128), (5, 8, 8, 512, 512)]
# (B, H, W, Cin, Cout, k, stride, pad, ipad) through csrc/conv_pad.hip; the last three take the row-mode stem
DIRECT_CASES = [(2, 9, 14, 128, 256, 3, 2, 1, 1), (1, 7, 30, 64, 64, 3, 1, 1, 1), (3, 12, 16, 256, 256, 3, 1, 1, 1),
                (2, 8, 6, 512, 512, 3, 1, 1, 1), (2, 6, 8, 512, 512, 3, 1, 1, 1), (3, 14, 10, 64, 64, 3, 1, 1, 2),
                (1, 33, 64, 64, 128, 1, 2, 0, 1), (2, 30, 18, 18, 64, 7, 2, 3, 3), (1, 18, 44, 18, 64, 7, 2, 3, 3),
                (2, 12, 20, 4, 64, 7, 2, 3, 3)]
# (B, H, W, Cin, Cout, k) through hps_conv2d_bn_act_pad_down: the k x k / 2 convolution and the 1 x 1 / 2 down-sample of one input
DOWN_CASES = [(3, 18, 10, 64, 128, 3), (2, 16, 12, 256, 512, 3), (1, 32, 24, 128, 256, 3), (2, 5, 9, 32, 128, 5)]


def wino_case(cfg):
    B, H, W, Cin, Cout = cfg
    return case(B, H, W, Cin, Cout, 3, 1, 1, seed=WINO_CASES.index(cfg))             # odd positions in the list: negative scales


def direct_case(cfg):
    return case(*cfg[:8], seed=DIRECT_CASES.index(cfg))


def down_cases(cfg):
    """(main, down): the block entry's k x k / 2 / (k // 2) convolution and its 1 x 1 / 2 / 0 down-sample on the same input."""
    B, H, W, Cin, Cout, k = cfg
    seed = DOWN_CASES.index(cfg)
    return case(B, H, W, Cin, Cout, k, 2, k // 2, seed=seed), case(B, H, W, Cin, Cout, 1, 2, 0, seed=seed)


@functools.lru_cache(maxsize=None)
def case(B, H, W, Cin, Cout, k, stride, pad, seed=0):
    """fp32 CPU modules and tensors of one case.  The input depends on (B, H, W, Cin, seed) only, so two cases that differ in the
    filter alone (a block's 3 x 3 / 2 convolution and its 1 x 1 / 2 down-sample) see the same x."""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(B + H + W + Cin + Cout + k + stride + pad + 1000 * seed)
        conv = torch.nn.Conv2d(Cin, Cout, k, stride, pad, bias=False)
        bn = torch.nn.BatchNorm2d(Cout).eval()
        bn.running_mean.normal_(); bn.running_var.uniform_(0.5, 2); bn.bias.data.normal_()
        if seed % 2:
            bn.weight.data.normal_()                      # negative scales too
        else:
            bn.weight.data.uniform_(0.5, 1.5)
    gx = torch.Generator().manual_seed(77 + 1000003 * seed + 10007 * B + 101 * H + 13 * W + Cin)
    x = torch.randn(B, Cin, H, W, generator=gx)
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    res = torch.randn(B, Cout, Ho, Wo, generator=torch.Generator().manual_seed(5 + seed + 31 * Cout + Ho * Wo))
    for p in list(conv.parameters()) + list(bn.parameters()):
        p.requires_grad_(False)
    return dict(key=(B, H, W, Cin, Cout, k, stride, pad, seed), conv=conv, bn=bn, x=x, res=res, B=B, H=H, W=W, Cin=Cin, Cout=Cout,
                k=k, stride=stride, pad=pad, Ho=Ho, Wo=Wo, K=k * k * Cin, wino=(k == 3 and stride == 1 and pad == 1 and H % 2 == 0 and W % 2 == 0))


def finish(lin, res, mode):
    """The mode's output from bn(conv(x)) in lin's own dtype."""
    if mode == "lin":
        return lin
    return F.relu(lin + res.to(lin.dtype)) if mode == "res_relu" else F.relu(lin)


def fold_bn(bn, dtype=torch.float32):
    """(scale, shift) of the eval BatchNorm, formed in float64 and rounded once to ``dtype``."""
    scale = bn.weight.double() * torch.rsqrt(bn.running_var.double() + bn.eps)
    return scale.to(dtype), (bn.bias.double() - bn.running_mean.double() * scale).to(dtype)


def sample_positions(c):
    """Flat indices into the (B, Cout, Ho, Wo) output: all of it when it has at most SAMPLE entries, else a seeded sample that holds,
    for the first and the last channel, the four corner pixels and one pixel of each border row and column of a (seeded) image."""
    B, Cout, Ho, Wo = c["B"], c["Cout"], c["Ho"], c["Wo"]
    n = B * Cout * Ho * Wo
    if n <= SAMPLE:
        return torch.arange(n)
    g = torch.Generator().manual_seed(4242 + n)
    r = lambda hi: int(torch.randint(0, hi, (1,), generator=g))
    must = []
    for ch in (0, Cout - 1):
        b = r(B)
        pix = [(0, 0), (0, Wo - 1), (Ho - 1, 0), (Ho - 1, Wo - 1), (0, r(Wo)), (Ho - 1, r(Wo)), (r(Ho), 0), (r(Ho), Wo - 1)]
        must += [((b * Cout + ch) * Ho + i) * Wo + j for i, j in pix]
    rest = torch.randperm(n, generator=g)[:SAMPLE - len(must)]
    return torch.unique(torch.cat([torch.tensor(must, dtype=torch.long), rest]))


def seq32_lin(c, idx):
    """bn(conv(x)) at the flat output positions ``idx`` by one sequential chain over K (module docstring), as fp32."""
    B, Cout, Ho, Wo, k, s, p, Cin = c["B"], c["Cout"], c["Ho"], c["Wo"], c["k"], c["stride"], c["pad"], c["Cin"]
    j = idx % Wo
    i = (idx // Wo) % Ho
    co = (idx // (Wo * Ho)) % Cout
    b = idx // (Wo * Ho * Cout)
    xp = F.pad(c["x"], (p, p, p, p)).permute(0, 2, 3, 1).contiguous().double()      # (B, H + 2p, W + 2p, Cin)
    w = c["conv"].weight.double()                                                    # (Cout, Cin, k, k)
    acc = torch.zeros(idx.numel(), dtype=torch.float64)                              # holds fp32 values
    for ti in range(k):
        for tj in range(k):
            xs = xp[b, i * s + ti, j * s + tj].t().contiguous()                      # (Cin, n)
            ws = w[co, :, ti, tj].t().contiguous()
            for ch in range(Cin):
                acc = (acc + xs[ch] * ws[ch]).float().double()                       # exact product, one rounding to fp32
    scale, shift = fold_bn(c["bn"])
    return acc.float() * scale[co] + shift[co]                                       # two fp32 roundings


_G = [[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]]
_BT = [[1.0, 0.0, -1.0, 0.0], [0.0, 1.0, 1.0, 0.0], [0.0, -1.0, 1.0, 0.0], [0.0, 1.0, 0.0, -1.0]]
_AT = [[1.0, 1.0, 1.0, 0.0], [0.0, 1.0, -1.0, -1.0]]


def wino_conv(x, w, dtype):
    """The 3 x 3 / 1 / 1 convolution of x (B, Cin, H, W; H, W even) with w (Cout, Cin, 3, 3) as Winograd F(2x2, 3x3) in ``dtype``:
    U = G g G^T, V = B^T d B per 4 x 4 input tile (stride 2), M = sum over channels of U * V per position, Y = A^T M A."""
    G, BT, AT = (torch.tensor(m, dtype=dtype) for m in (_G, _BT, _AT))
    x, w = x.to(dtype), w.to(dtype)
    B, Cin, H, W = x.shape
    Cout = w.shape[0]
    U = G @ w @ G.t()                                                                # (Cout, Cin, 4, 4)
    d = F.pad(x, (1, 1, 1, 1)).unfold(2, 4, 2).unfold(3, 4, 2)                       # (B, Cin, H/2, W/2, 4, 4)
    V = BT @ d @ BT.t()
    Um = U.permute(2, 3, 0, 1).reshape(16, Cout, Cin)
    Vm = V.permute(4, 5, 1, 0, 2, 3).reshape(16, Cin, -1)                            # (16, Cin, B * tiles)
    M = torch.bmm(Um, Vm).reshape(4, 4, Cout, B, H // 2, W // 2).permute(3, 2, 4, 5, 0, 1)
    Y = AT @ M @ AT.t()                                                              # (B, Cout, H/2, W/2, 2, 2)
    return Y.permute(0, 1, 2, 4, 3, 5).reshape(B, Cout, H, W)


def wino_lin(c, dtype=torch.float32):
    """bn(conv(x)) with the convolution by wino_conv in ``dtype`` and scale / shift in ``dtype``."""
    scale, shift = fold_bn(c["bn"], dtype)
    return wino_conv(c["x"], c["conv"].weight, dtype) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)


@functools.lru_cache(maxsize=None)
def _reference(key):
    c = case(*key)
    with torch.no_grad():
        lin64 = copy.deepcopy(c["bn"]).double()(copy.deepcopy(c["conv"]).double()(c["x"].double()))
        lin32 = c["bn"](c["conv"](c["x"]))
        idx = sample_positions(c)
        seq = seq32_lin(c, idx)
        wino = wino_lin(c) if c["wino"] else None
    out = {}
    for mode in MODES:
        y64 = finish(lin64, c["res"], mode)
        r = dict(y64=y64, y_cpu32=finish(lin32, c["res"], mode), idx=idx, y_seq32=finish(seq, c["res"].reshape(-1)[idx], mode),
                 y_wino32=finish(wino, c["res"], mode) if wino is not None else None)
        r["scale"] = float(y64.abs().max())
        r["e_cpu32"] = float((r["y_cpu32"].double() - y64).abs().max())
        r["e_seq32"] = float((r["y_seq32"].double() - y64.reshape(-1)[idx]).abs().max())
        r["e_wino32"] = float((r["y_wino32"].double() - y64).abs().max()) if wino is not None else None
        out[mode] = r
    return out


def reference(c, mode="res_relu"):
    """The case's references for one mode: y64, y_cpu32 (whole tensors, NCHW), idx and y_seq32 (the sampled flat positions and the
    chain's values there), y_wino32 (whole tensor or None), scale = max|y64| and the errors e_cpu32, e_seq32, e_wino32."""
    return _reference(c["key"])[mode]


def bound(c, mode="res_relu", wino=False):
    r = reference(c, mode)
    errs = [r["e_cpu32"], r["e_seq32"], EPS32 * r["scale"]]
    if wino:
        assert r["e_wino32"] is not None, "not a Winograd case"
        errs.append(r["e_wino32"])
    return 4.0 * max(errs)


def check(name, y_dev, c, mode="res_relu", wino=False, at=None):
    """Prints the figures, then asserts the accuracy rule for the WHOLE tensor y_dev (B, Cout, Ho, Wo) against y64; returns err / bound.
    ``wino``: the launch ran the Winograd kernel, so the Winograd evaluation belongs to the family.  ``at``: y_dev holds the values at
    these flat positions only (the sampled reference on its own)."""
    r = reference(c, mode)
    y64 = r["y64"] if at is None else r["y64"].reshape(-1)[at]
    y = y_dev.detach().cpu().double()
    assert y.shape == y64.shape, (name, tuple(y.shape), tuple(y64.shape))
    err, b, u = float((y - y64).abs().max()), bound(c, mode, wino), EPS32 * r["scale"]
    print("%-44s %-8s max|dev - f64| = %.3e  max|y64| = %.3e  in 2^-23 max|y64|: dev %.2f  cpu32 %.2f  seq32 %.2f  wino32 %s  err/bound = %.3f"
          % (name, mode, err, r["scale"], err / u, r["e_cpu32"] / u, r["e_seq32"] / u,
             "%.2f" % (r["e_wino32"] / u) if wino else "-", err / b))
    assert err == err and err <= b, (name, mode, err, b)
    return err / b


def assert_halo_untouched(out, opad, fill):
    """Every row and column of the halo of the frame ``out`` (B, Ho + 2 opad, Wo + 2 opad, C), on all four sides, still holds ``fill``."""
    if opad == 0:
        return
    sides = {"top": out[:, :opad], "bottom": out[:, -opad:], "left": out[:, :, :opad], "right": out[:, :, -opad:]}
    for side, t in sides.items():
        assert bool((t == fill).all()), "the %s halo has been written: %d elements differ from %r" % (side, int((t != fill).sum()), fill)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def frame(t_nhwc, pad, fill=0.0):
    """(B, H, W, C) -> (B, H + 2 pad, W + 2 pad, C) with a halo of ``fill``."""
    return F.pad(t_nhwc, (0, 0, pad, pad, pad, pad), value=fill).contiguous()
