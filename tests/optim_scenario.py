"""The optimiser step and the weight refresh restated on the host, independent of csrc/optim.hip.

``adam_update``: torch/optim/adam.py _single_tensor_adam in float64, one tensor, one step (tests/test_optim_host.py holds it to
torch.optim.Adam on float64 parameters).  ``run_refresh_ops``: every hps_refresh_op kind as torch operations on host memory, read and
written through the pointers of the op list itself -- so a list built by ResNet._refresh_list / PoseMFShapeGaussianNet._refresh_list
on a CPU net is checked with its real extents, strides and offsets.  ``derived_tensors``: every tensor of a net's prepared device
state by name, the walk the refresh tests share.
"""
import ctypes

import numpy as np
import torch

from hierarchicalprobabilistic3dhuman_amd import _capi
from hierarchicalprobabilistic3dhuman_amd.resnet import _ConvBN, _STEM_G3, _STEM_G4

EPS32 = 2.0 ** -23
SIZES = (1, 3, 64, 65, 1023, 4097, 70001)       # one launch: below / at / above a 16-byte piece, a partial and 17 full chunks + a tail
WINO_G = [[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]]


def adam_update(p, g, m, v, step, lr, beta1, beta2, eps, weight_decay=0.0, decoupled=False):
    """(p, m, v) after step number ``step`` (1-based), float64 tensors in, float64 tensors out."""
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    if weight_decay != 0 and not decoupled:
        g = g + weight_decay * p
    if weight_decay != 0 and decoupled:
        p = p * (1 - lr * weight_decay)
    m = m + (1 - beta1) * (g - m)
    v = beta2 * v + (1 - beta2) * g * g
    bc1, bc2_sqrt = 1 - beta1 ** step, (1 - beta2 ** step) ** 0.5
    denom = v.sqrt() / bc2_sqrt + eps
    return p - (lr / bc1) * (m / denom), m, v


def gradients(sizes=SIZES, seed=3):
    """Per size a gradient spanning 1e-12 ... 1e3 in magnitude with exact zeros; the tensor of 64 elements is all zeros."""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for n in sizes:
        mag = 10.0 ** (torch.rand(n, generator=gen, dtype=torch.float64) * 15 - 12)
        g = (mag * torch.sign(torch.randn(n, generator=gen, dtype=torch.float64))).float()
        g[::7] = 0.0
        if n == 64:
            g.zero_()
        out.append(g)
    return out


def parameters(sizes=SIZES, seed=4):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=gen) for n in sizes]


# ---- hps_refresh_op on host memory ----
def _view(ptr, n):
    return torch.from_numpy(np.ctypeslib.as_array((ctypes.c_float * n).from_address(ptr)))


def wino_u_flat(w, order=0):
    """G g G^T of (Cout, Cin, 3, 3) in float64, term by term in one of two summation orders, in hps_conv3x3_winograd's layout
    (decoded index by index, not by reshape / permute), rounded once."""
    cout, cin = w.shape[:2]
    g, G, dev = w.double(), WINO_G, w.device                  # on the weight's device: IEEE float64 adds and products either way
    t = torch.arange(16 * cin * cout, device=dev)
    j, n, kq, p = t & 3, (t >> 2) & 63, (t >> 8) & 1, (t >> 9) & 15
    ct, chunk = (t >> 13) % (cout // 64), (t >> 13) // (cout // 64)
    U = torch.zeros(4, 4, cout, cin, dtype=torch.float64, device=dev)
    for a in range(4):
        for b in range(4):
            s = torch.zeros(cout, cin, dtype=torch.float64, device=dev)
            for x in range(3):
                inner = torch.zeros(cout, cin, dtype=torch.float64, device=dev)
                for y in range(3):
                    inner = inner + (g[:, :, x, y] * G[b][y] if order == 0 else g[:, :, y, x] * G[a][y])
                s = s + (G[a][x] if order == 0 else G[b][x]) * inner
            U[a, b] = s
    return U[p >> 2, p & 3, ct * 64 + n, chunk * 8 + kq * 4 + j].float()


def stem_u_flat(w, order=0):
    """The 81 positions of (64, 18, 7, 7) in hps_stem_winograd's layout, float64 term by term in one of two orders, rounded once."""
    g = w.double()
    t = torch.arange(81 * 1152)
    pos, r = t // 1152, t % 1152
    half, q = r // 576, r % 576
    lo = q < 512
    c = torch.where(lo, 8 * (q >> 8) + 2 * (q & 3) + ((q >> 7) & 1), 16 + ((q - 512) >> 5))
    co = half * 32 + torch.where(lo, (q >> 2) & 31, (q - 512) & 31)
    out = torch.zeros(81 * 1152, dtype=torch.float64)
    first = 0
    for ry in (0, 1):
        for rx in (0, 1):
            gy, gx = (_STEM_G4 if ry == 0 else _STEM_G3), (_STEM_G4 if rx == 0 else _STEM_G3)
            taps = g[:, :, ry::2, rx::2]
            u = torch.zeros(len(gy), len(gx), 64, 18, dtype=torch.float64)
            for i in range(len(gy)):
                for k in range(len(gx)):
                    s = torch.zeros(64, 18, dtype=torch.float64)
                    outer, inner_n = (len(gy[0]), len(gx[0])) if order == 0 else (len(gx[0]), len(gy[0]))
                    for a in range(outer):
                        inner = torch.zeros(64, 18, dtype=torch.float64)
                        for b in range(inner_n):
                            inner = inner + (taps[:, :, a, b] * gx[k][b] if order == 0 else taps[:, :, b, a] * gy[i][b])
                        s = s + (gy[i][a] if order == 0 else gx[k][a]) * inner
                    u[i, k] = s
            count = len(gy) * len(gx)
            sel = (pos >= first) & (pos < first + count)
            local = pos[sel] - first
            out[sel] = u[local // len(gx), local % len(gx), co[sel], c[sel]]
            first += count
    return out.float()


def run_refresh_ops(ops):
    """Every op of a RefreshList's ``ops`` on HOST memory."""
    for op in ops:
        n, ss, ds = list(op.n), list(op.sstride), list(op.dstride)
        if op.kind == _capi.REFRESH_PERMUTE:
            grids = torch.meshgrid(*[torch.arange(k) for k in n], indexing="ij")
            so, to = sum(i * s for i, s in zip(grids, ss)).reshape(-1), sum(i * s for i, s in zip(grids, ds)).reshape(-1)
            val = _view(op.src, int(so.max()) + 1)[so]
            if op.aux0:
                val = (val.double() * _view(op.aux0, n[op.scale_dim])[grids[op.scale_dim].reshape(-1)].double()).float()
            _view(op.dst, int(to.max()) + 1)[to] = val
        elif op.kind == _capi.REFRESH_FOLD:
            c = n[0]
            gamma, beta, mean, var = (_view(ptr, c).double() for ptr in (op.src, op.aux0, op.aux1, op.aux2))
            scale = gamma * torch.rsqrt(var + op.eps)
            _view(op.dst, c).copy_(scale.float())
            _view(op.dst2, c).copy_((beta - mean * scale).float())
        elif op.kind == _capi.REFRESH_WINO_U:
            cout, cin = n[:2]
            _view(op.dst, 16 * cout * cin).copy_(wino_u_flat(_view(op.src, cout * cin * 9).view(cout, cin, 3, 3)))
        elif op.kind == _capi.REFRESH_STEM_U:
            _view(op.dst, 81 * 1152).copy_(stem_u_flat(_view(op.src, 64 * 18 * 49).view(64, 18, 7, 7)))
        else:
            raise AssertionError(op.kind)


# ---- the prepared state by name ----
def _walk(obj, name, out):
    if isinstance(obj, torch.Tensor):
        out[name] = obj
    elif isinstance(obj, dict):
        for k, v in obj.items():
            if k not in ("versions", "stale_bn"):
                _walk(v, "%s.%s" % (name, k), out)
    elif isinstance(obj, (list, tuple)):
        for i, v in enumerate(obj):
            _walk(v, "%s.%d" % (name, i), out)
    elif isinstance(obj, _ConvBN):
        _walk(vars(obj), name, out)


def derived_tensors(net):
    """{name: tensor} of every tensor under the encoder's and the head's ``prep`` (the backward's entries included)."""
    out = {}
    _walk(net.image_encoder._prepared, "enc", out)
    _walk(net._prepared, "head", out)
    return out


def build_backward_entries(net):
    """What the first backward adds to the two prepared states, for every layer in both forms (a CPU net cannot run one)."""
    enc = net.image_encoder
    prep = enc._prepared
    convs = [prep["stem"]] + [c for blk in prep["blocks"] for c in blk if c is not None]
    for (name, conv, _), cb in zip(enc._enc_layers(), convs):
        enc._dgrad_filter(prep, name, conv, cb, raw=False)
        enc._dgrad_filter(prep, name, conv, cb, raw=True)
    net._prepare_backward(net._prepared)


def ulp_distance(a, b):
    """Per element, in units of the last place (same-sign fp32 values; a sign change counts through zero)."""
    ia, ib = a.contiguous().view(torch.int32).long(), b.contiguous().view(torch.int32).long()
    ia, ib = torch.where(ia < 0, -(ia & 0x7FFFFFFF), ia), torch.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return (ia - ib).abs()


def compare_states(got, want):
    """Bit-equal tensor by tensor; stem_u within 1 ulp with at most 1 % of its elements different (its coefficients include 1/6: two
    float64 evaluations may round differently at a tie).  Returns {name: number of differing elements} for the report."""
    assert set(got) == set(want), sorted(set(got) ^ set(want))
    report = {}
    for name in sorted(want):
        if name.endswith("_ptrs"):                 # addresses of the net's own copies
            continue
        a, b = got[name].detach().cpu(), want[name].detach().cpu()
        assert a.shape == b.shape and a.dtype == b.dtype, name
        if name.endswith(".stem_u"):
            d = ulp_distance(a, b)
            report[name] = int((d != 0).sum())
            assert int(d.max()) <= 1 and report[name] <= 0.01 * a.numel(), (name, int(d.max()), report[name])
        else:
            bad = int((a != b).sum())
            assert bad == 0 and torch.equal(a, b), "%s: %d of %d elements differ from a fresh build" % (name, bad, a.numel())
    return report
