"""GPU: the metric, checksum and small front-end kernels (csrc/metrics.hip: hps_pointset_errors, hps_sums_f64; csrc/frontend.hip:
heatmap_argmax_kernel, proxy_rep_kernel, sample_j2d_error_kernel) against the float64 truths and derived bounds of
tests/eval_scenario.py, through the product's entry points, at the sizes where their unrolled loops, tails, reductions, alignment
switches and block boundaries can go wrong.  tests/test_eval_scenario_host.py shows on the host that every rule used here catches the
wrong kernels it is meant to catch.  Every test prints its worst err / bound."""
import ctypes

import numpy as np
import pytest
import torch

import eval_scenario as E
from hierarchicalprobabilistic3dhuman_amd import _capi, eval_utils, sharding
from hierarchicalprobabilistic3dhuman_amd.label_conversions import (convert_heatmaps_to_2Djoints_coordinates_torch,
                                                                    make_proxy_representation)

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
PAD = 64                     # guard elements on each side of an output placed inside a larger buffer


def _same_bits(a, b):
    """Bit-identical tensors (NaNs included)."""
    view = {torch.float64: torch.int64, torch.float32: torch.int32}[a.dtype]
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(view), b.contiguous().view(view))


def _guarded(n, dev, dtype=torch.float32):
    """(buffer of PAD + n + PAD sentinels, its interior view, the interior's device address)."""
    buf = torch.full((2 * PAD + n,), SENTINEL, device=dev, dtype=dtype)
    return buf, buf[PAD:PAD + n], ctypes.c_void_p(buf.data_ptr() + PAD * buf.element_size())


def _assert_guards_intact(buf, what):
    head, tail = buf[:PAD].cpu(), buf[-PAD:].cpu()
    assert bool((head == SENTINEL).all()), "%s: %d elements in front of the output were written" % (what, int((head != SENTINEL).sum()))
    assert bool((tail == SENTINEL).all()), "%s: %d elements behind the output were written" % (what, int((tail != SENTINEL).sum()))


# ---------------------------------------------------------------------------------------------------------------------
# hps_pointset_errors
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,names", E.POINTSET_FAMILIES, ids=[f for f, _ in E.POINTSET_FAMILIES])
def test_pointset_errors_match_float64(family, names, dev):
    """eval_utils.pointset_errors with and without the transformed output: error sums and transformed points inside the bounds of
    eval_scenario (the two ill-posed inputs as stated there), sums bit-identical with and without the transformed output and across
    calls, and group = g bit-identical to group = 1 against the repeated targets."""
    worst = {m: 0.0 for m in E.MODES}
    for name in names:
        c = E.pointset_case(name)
        pred, target = torch.from_numpy(c["pred"]).to(dev), torch.from_numpy(c["target"]).to(dev)
        for mode in E.MODES:
            err_only = eval_utils.pointset_errors(pred, target, mode, group=c["group"])
            err, q = eval_utils.pointset_errors(pred, target, mode, group=c["group"], return_transformed=True)
            assert err.dtype == torch.float64 and err.shape == (c["S"],) and q.dtype == torch.float32 and q.shape == pred.shape
            assert _same_bits(err_only, err), (name, mode, "the sums depend on the transformed output being asked for")
            again = eval_utils.pointset_errors(pred, target, mode, group=c["group"])
            assert _same_bits(again, err), (name, mode, "the sums differ between two calls")
            worst[mode] = max(worst[mode], E.check_pointsets("device", c, mode, err.cpu().numpy(), q.cpu().numpy()))
            if c["group"] > 1:
                repeated = torch.from_numpy(np.ascontiguousarray(E.targets(c))).to(dev)
                err1, q1 = eval_utils.pointset_errors(pred, repeated, mode, group=1, return_transformed=True)
                assert _same_bits(q1, q) and _same_bits(err1, err), (name, mode, "group = %d differs from group = 1" % c["group"])
    print("worst err / bound, point sets, %s: %s" % (family, ", ".join("%s %.3f" % (E.MODE_NAMES[m], worst[m]) for m in E.MODES)))


@pytest.mark.parametrize("name", ["P257", "P1025", "S65", "g7x3", "P1"])
def test_pointset_transformed_output_stays_inside_its_buffer(name, dev):
    """hps_pointset_errors writing its transformed points and its sums into the interior of larger sentinel-filled buffers: the
    sentinels in front and behind are intact, and the interior holds what eval_utils.pointset_errors returns, bit for bit."""
    c = E.pointset_case(name)
    S, P = c["S"], c["P"]
    pred, target = torch.from_numpy(c["pred"]).to(dev), torch.from_numpy(c["target"]).to(dev)
    for mode in E.MODES:
        want_err, want_q = eval_utils.pointset_errors(pred, target, mode, group=c["group"], return_transformed=True)
        qbuf, q, q_addr = _guarded(S * P * 3, dev)
        ebuf, e, e_addr = _guarded(S, dev, torch.float64)
        xbuf, _, x_addr = _guarded(S * 12, dev)
        stats = torch.empty(S, 17, device=dev, dtype=torch.float64)
        _capi.call("hps_pointset_errors", _capi.ptr(pred), _capi.ptr(target), S, c["group"], P, mode, _capi.ptr(stats, torch.float64),
                   x_addr, e_addr, q_addr, _capi.stream())
        for buf, what in ((qbuf, "transformed points"), (ebuf, "error sums"), (xbuf, "transforms")):
            _assert_guards_intact(buf, "%s, mode %s, %s" % (name, E.MODE_NAMES[mode], what))
        assert _same_bits(q.view(S, P, 3), want_q) and _same_bits(e, want_err)


# ---------------------------------------------------------------------------------------------------------------------
# hps_sums_f64
# ---------------------------------------------------------------------------------------------------------------------
def _upload(n, dev, seed=0):
    """The case's values on the device; n = 0: a one-element allocation (the entry point refuses a null table entry)."""
    x = E.sum_values(n, seed)
    return x, (torch.from_numpy(x.copy()).to(dev) if n else torch.zeros(1, device=dev))


def _sums(dev, tensors, ns, take_abs, first, accumulate=None):
    """One hps_sums_f64 call; the (1 + count,) result sits inside a guarded buffer."""
    count = len(tensors)
    ws = torch.empty(4 * 128, dtype=torch.float64, device=dev)
    obuf, out, o_addr = _guarded(1 + count, dev, torch.float64)
    xs = (ctypes.c_void_p * count)(*[t.data_ptr() for t in tensors])
    _capi.call("hps_sums_f64", xs, (ctypes.c_int64 * count)(*ns), (ctypes.c_int32 * count)(*take_abs), count, float(first),
               _capi.ptr(ws, torch.float64), o_addr, _capi.ptr(accumulate, torch.float64) if accumulate is not None else None,
               _capi.stream())
    _assert_guards_intact(obuf, "hps_sums_f64 out, count %d" % count)
    return out.clone()


def test_checksums_match_fsum_at_every_length(dev):
    """Every length of eval_scenario.SUM_LENGTHS, plain and absolute in one call: within n 2^-53 sum|x| of math.fsum, out[0] == first,
    bitwise repeatable."""
    worst = 0.0
    for n in E.SUM_LENGTHS:
        x, t = _upload(n, dev)
        a = _sums(dev, [t, t], [n, n], [0, 1], 3.5 + n)
        b = _sums(dev, [t, t], [n, n], [0, 1], 3.5 + n)
        assert _same_bits(a, b), n
        a = a.cpu()
        assert float(a[0]) == 3.5 + n
        worst = max(worst, E.check_sum("device", a[1], x, 0), E.check_sum("device", a[2], x, 1))
    print("worst err / bound, checksum, every length: %.3g" % worst)


@pytest.mark.parametrize("lengths,take_abs", [((536633,), (1,)), ((0, 536633), (1, 0)), ((229377, 0, 257), (1, 1, 0)),
                                             ((32769, 536633, 1, 491521), (1, 0, 0, 1)), ((262149, 255, 229376, 0), (0, 0, 1, 1))],
                         ids=lambda v: "-".join(str(i) for i in v))
def test_checksums_with_one_to_four_tensors(lengths, take_abs, dev):
    """count 1 to 4 with a different n per tensor (n = 0 beside the longest) and take_abs patterns other than (0, 1, 1)."""
    xs, ts = zip(*[_upload(n, dev, seed=j) for j, n in enumerate(lengths)])
    out = _sums(dev, ts, lengths, take_abs, -2.0).cpu()
    assert out.shape == (1 + len(lengths),) and float(out[0]) == -2.0
    worst = max(E.check_sum("device, tensor %d of %d" % (j, len(lengths)), out[1 + j], xs[j], take_abs[j]) for j in range(len(lengths)))
    assert _same_bits(out, _sums(dev, ts, lengths, take_abs, -2.0).cpu())
    print("worst err / bound, checksum, %d tensors: %.3g" % (len(lengths), worst))


def test_checksum_accumulator_adds_in_float64(dev):
    """accumulate: after two calls it holds exactly a0 + s1 + s2, as float64 additions in that order leave it -- through the raw entry
    point and through sharding.batch_metric_sums (bench.py's route: three tensors, take_abs (0, 1, 1), first = the image count)."""
    lengths = (229377, 536633, 257)
    xs1, ts1 = zip(*[_upload(n, dev, seed=1) for n in lengths])
    xs2, ts2 = zip(*[_upload(n, dev, seed=2) for n in lengths])
    a0 = torch.tensor([0.1, 1e6 + 1.0 / 3, -12345.678, 2.0 ** -30], dtype=torch.float64)
    acc = a0.to(dev)
    s1 = _sums(dev, ts1, lengths, (0, 1, 1), 7.0, accumulate=acc).cpu()
    s2 = _sums(dev, ts2, lengths, (1, 0, 0), 9.0, accumulate=acc).cpu()
    assert float(s1[0]) == 7.0 and float(s2[0]) == 9.0
    assert _same_bits(acc.cpu(), (a0 + s1) + s2)
    assert _same_bits(s1, _sums(dev, ts1, lengths, (0, 1, 1), 7.0).cpu()), "the sums depend on the accumulator being given"
    # the product's wrapper on the same tensors, shaped like an infer() result
    res1 = {"unc": ts1[0].view(3, -1), "verts_mode": ts1[1], "joints_samples": ts1[2]}
    res2 = {"unc": ts2[0].view(3, -1), "verts_mode": ts2[1], "joints_samples": ts2[2]}
    acc = a0.to(dev)
    b1 = sharding.batch_metric_sums(res1, accumulate=acc).cpu()
    b2 = sharding.batch_metric_sums(res2, accumulate=acc).cpu()
    assert float(b1[0]) == 3.0 and _same_bits(b1[1:], s1[1:])
    assert _same_bits(acc.cpu(), (a0 + b1) + b2)
    assert _same_bits(b2, sharding.batch_metric_sums(res2).cpu())
    worst = 0.0
    for j in range(3):
        worst = max(worst, E.check_sum("batch_metric_sums", b1[1 + j], xs1[j], (0, 1, 1)[j]), E.check_sum("batch_metric_sums", b2[1 + j], xs2[j], (0, 1, 1)[j]))
    print("worst err / bound, checksum, batch_metric_sums: %.3g" % worst)


# ---------------------------------------------------------------------------------------------------------------------
# heatmap_argmax_kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("H,W", E.HEAT_SHAPES)
def test_heatmap_argmax_equals_numpy_argmax(H, W, aligned, dev):
    """convert_heatmaps_to_2Djoints_coordinates_torch on the maps of eval_scenario.heat_case, exactly; ``misaligned``: the maps start four
    bytes into an allocation (a contiguous view at element offset 1), which takes the scalar loop."""
    heat, labels = E.heat_case(H, W, aligned)
    n = heat.size
    buf = torch.zeros(n + 4, device=dev)
    off = 0 if aligned else 1
    h = buf[off:off + n].view(heat.shape)
    h.copy_(torch.from_numpy(heat.copy()))
    assert h.is_contiguous() and h.data_ptr() % 16 == 4 * off
    j, vis = convert_heatmaps_to_2Djoints_coordinates_torch(h)
    assert j.shape == (1, len(labels), 2) and vis.shape == (1, len(labels)) and vis.dtype == torch.bool
    checked = E.check_heat("device", j.cpu().numpy(), vis.cpu().numpy(), heat, labels)
    print("heat-maps %d x %d, %s: %d maps equal numpy.argmax" % (H, W, "aligned" if aligned else "misaligned", checked))


# ---------------------------------------------------------------------------------------------------------------------
# proxy_rep_kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", E.PROXY_CASES, ids=lambda c: "x".join(str(v) for v in c[:4]))
def test_proxy_representation_matches_float64(cfg, dev):
    """hps_proxy_rep into the interior of a sentinel-filled buffer: heat-maps inside the bound, channel 0 the edge plane bit for bit,
    guards intact; then once without visibilities and once without an edge plane (channel 0 is left alone)."""
    c = E.proxy_case(cfg)
    B, K, H, W, std = cfg
    n = B * (K + 1) * H * W
    edge, vis = c["edge"].to(dev), c["vis"].to(dev)
    joints = c["joints"].to(dev) if K else torch.zeros(2, device=dev)      # K = 0: nothing is read, but the table must not be null
    P = _capi.ptr

    def run(edge_t, vis_t):
        buf, out, addr = _guarded(n, dev)
        _capi.call("hps_proxy_rep", P(edge_t) if edge_t is not None else None, P(joints), P(vis_t) if vis_t is not None and K else None,
                   addr, B, K, H, W, float(std), _capi.stream())
        _assert_guards_intact(buf, "hps_proxy_rep %s" % (cfg,))
        return out.view(B, K + 1, H, W)

    full = run(edge, vis)
    worst = E.check_proxy("device", full, c, with_vis=True)
    no_vis = run(edge, None)
    worst = max(worst, E.check_proxy("device, visib == NULL", no_vis, c, with_vis=False))
    no_edge = run(None, vis)
    assert bool((no_edge[:, 0] == SENTINEL).all()), "channel 0 was written without an edge plane"
    assert _same_bits(no_edge[:, 1:], full[:, 1:])
    if H == W and K:
        assert _same_bits(make_proxy_representation(edge, c["joints"].to(dev), vis, H, std), full.contiguous())
    print("worst err / bound, proxy representation %s: %.3f" % (cfg, worst))


# ---------------------------------------------------------------------------------------------------------------------
# sample_j2d_error_kernel
# ---------------------------------------------------------------------------------------------------------------------
def _sample_errors(c, dev):
    N = c["N"]
    buf, err, addr = _guarded(N, dev)
    coco = torch.tensor(E.COCO_MAP, dtype=torch.int32, device=dev)
    joints, in_j2d, in_vis, cam = (c[k].to(dev) for k in ("joints", "in_j2d", "in_vis", "cam"))      # alive until the call has been issued
    _capi.call("hps_sample_joints2d_error", _capi.ptr(joints), _capi.iptr(coco), 90, _capi.ptr(in_j2d), _capi.ptr(in_vis), _capi.ptr(cam),
               float(E.IMG_WH), addr, N, len(E.COCO_MAP), _capi.stream())
    _assert_guards_intact(buf, "hps_sample_joints2d_error N = %d" % N)
    return err.clone()


def test_sample_joints2d_errors_match_float64(dev):
    worst = 0.0
    for N in E.SAMPLE_NS:
        c = E.sample_case(N)
        got = _sample_errors(c, dev)
        assert _same_bits(got, _sample_errors(c, dev))
        worst = max(worst, E.check_sample_errors("device", got, c))
    print("worst err / bound, sample 2-D error: %.3f" % worst)


def test_sample_joints2d_error_with_every_joint_invisible(dev):
    # the kernel's maximum over no joint is -inf; the reference raises on the empty maximum (torch.max of an empty dimension)
    c = E.sample_case(65, all_invisible=True)
    got = _sample_errors(c, dev).cpu()
    assert got.shape == (65,) and bool((got == float("-inf")).all())
    with pytest.raises((RuntimeError, IndexError)):
        E.sample_errors(c, torch.float32)
