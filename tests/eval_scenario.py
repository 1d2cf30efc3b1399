"""Seeded cases, float64 truths, fp32 restatements and the accuracy rules of the evaluation and small front-end kernel tests
(tests/test_eval_scenario_host.py, tests/test_gpu_eval_kernels.py): csrc/metrics.hip (hps_pointset_errors, hps_sums_f64) and
csrc/frontend.hip (heatmap_argmax_kernel, proxy_rep_kernel, sample_j2d_error_kernel).  Nothing here touches a device; references
are computed once per case and shared (callers must not modify them).

POINT SETS.  A case is (pred (S, P, 3) fp32, target (ceil(S / group), P, 3) fp32, group); set s is compared with target s // group, in
the three modes of eval_utils.pointset_errors (raw, scale-and-translation, Procrustes).  The truth q64 is the reference's formulas as
oracle/ref_cpu.py states them (compute_similarity_transform, scale_and_translation_transform_batch, the raw route) evaluated in float64
on the fp32 inputs; q32 is the same with EVERY array in float32 (the fp32 restatement).  The rule, this project's usual one:

    bound_pts = 4 * max(e32, 2**-23 * max(|q64|, |pred|))        e32 = max|q32 - q64|        (maxima over the whole case)
    bound_sum = sqrt(3) * P * bound_pts                           on a set's sum of point-wise L2 errors

bound_sum is the triangle inequality: | |a| - |b| | <= |a - b| <= sqrt(3) max|a - b| per point, P points; the kernel sums in float64,
so nothing more is owed.  Two inputs are ILL-POSED and are the only exclusions:

  * P = 1 in the SC and PA modes: the variance is zero, the reference divides 0 by 0; only "the result is non-finite, as the
    reference's is" is asserted.
  * a collinear target with a noisy 3-D prediction in the PA mode: K = X1 X2^T has rank one, the rotation about the target's line is
    undetermined and the reference's own fp32 points are off by O(0.1).  The transformed points are not compared.  The error SUM is
    invariant under that rotation (a rotation about the line keeps every distance to a point ON the line, and the scale tr(R K) / var1
    is the one non-zero singular value over var1), so it is held to the floor alone: sqrt(3) * P * 4 * 2**-23 * scale.
    (P = 2 is NOT of this kind although its K has rank one too: the centred prediction lies on one line, so q does not move.)

CHECKSUMS.  Truth: math.fsum of the fp32 values (or of their absolute values).  Bound: n * 2**-53 * sum|x|, the textbook bound of any
fixed-order float64 summation -- derived, not measured.  The values are distinct, of mixed signs, never below 0.05 in magnitude and
with a few entries a thousand times larger, so a dropped, repeated or un-absed element moves the sum by far more than the bound.

HEAT-MAPS.  Truth: numpy.argmax (first occurrence guaranteed), the reference's outputs (idx % W, floor(idx / W)) and max > eps, compared
exactly.  No map holds a NaN: the reference's heat-maps (network outputs through finite arithmetic) never do, and neither numpy's nor the
kernel's ordering says anything about them.  The maps of a shape place their maxima on the first and last element of every load path of
heatmap_argmax_kernel (load_paths restates its index partition for that placement only -- the truth never looks at it).

PROXY REPRESENTATION.  Truth: exp(-((row - v) / std)**2 / 2 - ((col - u) / std)**2 / 2) * vis in float64; the fp32 restatement is the same
in torch float32; bound 4 * max(e32, 2**-23) (the values are <= 1).  Channel 0 is a copy of the edge plane: bit for bit.

SAMPLE 2-D ERROR.  Truth: the expression of oracle.joints2d_error_sorted in front of the sort, in float64; bound
4 * max(e32, 2**-23 * max(|u|, |v|, img_wh)) with (u, v) the projected pixel coordinates.
"""
import functools
import math

import numpy as np
import torch

EPS32 = 2.0 ** -23
MODE_RAW, MODE_SC, MODE_PA = 0, 1, 2
MODES = (MODE_RAW, MODE_SC, MODE_PA)
MODE_NAMES = {MODE_RAW: "raw", MODE_SC: "SC", MODE_PA: "PA"}


# =====================================================================================================================
# point sets
# =====================================================================================================================
SIZES = (1, 2, 3, 4, 14, 255, 256, 257, 769, 1023, 1024, 1025, 1100, 2049)
GROUPS = ((7, 3), (8, 4), (5, 5), (1, 4))
NOISE = 0.05            # the "noisy" similarity transform: far above every bound, so that a lost point shows in a sum
FAMILIES = ("offset", "coplanar_clean", "coplanar_noisy", "collinear_clean", "collinear_noisy", "reflected", "copy", "exact_similarity",
            "cube", "scale_1e-3", "scale_1e3", "slab")
P_FAMILY = 300


def _rotation(rs):
    q, _ = np.linalg.qr(rs.randn(3, 3))
    return q * np.sign(np.linalg.det(q))


def _similar(rs, t, noise):
    """A similarity transform (scale 0.7 .. 1.3, proper rotation, offset ~ 0.2) of the (P, 3) cloud t, plus isotropic noise."""
    s, R, off = 0.7 + 0.6 * rs.rand(), _rotation(rs), 0.2 * rs.randn(3)
    return s * t.dot(R.T) + off + noise * rs.randn(*t.shape)


def _f32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


@functools.lru_cache(maxsize=None)
def pointset_case(name):
    """dict(name, pred, target, group, S, P) of the case ``name``: "P<n>" (two sets of n points), "S65" / "S130" (P = 14), "g<S>x<group>"
    (P = 300, one target per group), or a family of FAMILIES (two sets of 300 points; the cube: 8)."""
    rs = np.random.RandomState(sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) + 20240)
    cloud = lambda P: 0.3 * rs.randn(P, 3)
    group = 1
    if name[0] == "P" or name[0] == "S":
        S, P = (2, int(name[1:])) if name[0] == "P" else (int(name[1:]), 14)
        target = np.stack([cloud(P) for _ in range(S)])
        pred = np.stack([_similar(rs, t, NOISE) for t in target])
    elif name[0] == "g":
        S, group = (int(v) for v in name[1:].split("x"))
        target = np.stack([cloud(P_FAMILY) for _ in range(-(-S // group))])            # a different target per group
        pred = np.stack([_similar(rs, target[s // group], NOISE) for s in range(S)])
    else:
        S, P = 2, P_FAMILY
        if name == "cube":
            corners = 0.3 * np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=np.float64)
            target = np.stack([corners.dot(_rotation(rs).T) for _ in range(S)])      # K has three equal singular values ...
            pred = np.stack([_similar(rs, t, 1e-3) for t in target])                   # ... up to the 1e-3 noise
        elif name.startswith("coplanar") or name.startswith("collinear"):
            rank = 2 if name.startswith("coplanar") else 1
            target = []
            for _ in range(S):
                basis = _rotation(rs)[:rank]                                          # orthonormal rows spanning the plane / the line
                target.append((0.3 * rs.randn(P, rank)).dot(basis) + 0.2 * rs.randn(3))
            target = np.stack(target)
            pred = np.stack([_similar(rs, t, NOISE if name.endswith("noisy") else 0.0) for t in target])
        else:
            target = np.stack([cloud(P) for _ in range(S)])
            if name == "slab":
                target[..., 2] *= 1e-4                                                # relative thickness 1e-4
            if name == "copy":
                pred = target.copy()
            elif name == "exact_similarity":
                pred = np.stack([_similar(rs, t, 0.0) for t in target])
            else:
                pred = np.stack([_similar(rs, t, NOISE) for t in target])
            if name == "offset":                                                      # a common offset of ~100 m on both sets
                off = np.array([70.0, -60.0, 40.0])
                target, pred = target + off, pred + off
            if name == "reflected":
                pred[..., 0] *= -1.0                                                  # det K < 0
            if name.startswith("scale_"):
                f = float(name[len("scale_"):])
                target, pred = target * f, pred * f
    pred, target = _f32(pred), _f32(target)
    return dict(name=name, pred=pred, target=target, group=group, S=pred.shape[0], P=pred.shape[1])


SIZE_CASES = tuple("P%d" % p for p in SIZES)
BATCH_CASES = ("S65", "S130")
GROUP_CASES = tuple("g%dx%d" % sg for sg in GROUPS)
POINTSET_CASES = SIZE_CASES + BATCH_CASES + GROUP_CASES + FAMILIES
# test parameters: (family id, case names)
POINTSET_FAMILIES = (("sizes", SIZE_CASES), ("batches", BATCH_CASES), ("groups", GROUP_CASES)) + tuple((f, (f,)) for f in FAMILIES)


def similarity_transform(S1, S2, dtype, det_fix=True, sc_scale=False, translation=True):
    """oracle.ref_cpu.compute_similarity_transform for (N, 3) inputs with every array in ``dtype`` (the oracle's np.eye(3) is float64
    and promotes what follows it; here Z has the inputs' dtype).  The keyword switches build the wrong kernels of the host tests: no
    determinant fix, the SC mode's scale sqrt(var2 / var1), no translation."""
    S1, S2 = np.asarray(S1, dtype=dtype).T, np.asarray(S2, dtype=dtype).T
    mu1, mu2 = S1.mean(axis=1, keepdims=True), S2.mean(axis=1, keepdims=True)
    X1, X2 = S1 - mu1, S2 - mu2
    var1 = np.sum(X1 ** 2)
    K = X1.dot(X2.T)
    U, s, Vh = np.linalg.svd(K)
    V = Vh.T
    Z = np.eye(3, dtype=dtype)
    if det_fix:
        Z[-1, -1] *= np.sign(np.linalg.det(U.dot(V.T)))
    R = V.dot(Z.dot(U.T))
    scale = np.sqrt(np.sum(X2 ** 2) / var1) if sc_scale else np.trace(R.dot(K)) / var1
    t = mu2 - scale * (R.dot(mu1)) if translation else np.zeros_like(mu2)
    out = (scale * R.dot(S1) + t).T
    assert out.dtype == dtype
    return out


def scale_and_translation(P, T, dtype, translation=True):
    """oracle.ref_cpu.scale_and_translation_transform_batch with every array in ``dtype``."""
    P, T = np.asarray(P, dtype=dtype), np.asarray(T, dtype=dtype)
    P_mean = np.mean(P, axis=1, keepdims=True)
    P_trans = P - P_mean
    P_scale = np.sqrt(np.sum(P_trans ** 2, axis=(1, 2), keepdims=True) / dtype(P.shape[1]))
    T_mean = np.mean(T, axis=1, keepdims=True)
    T_scale = np.sqrt(np.sum((T - T_mean) ** 2, axis=(1, 2), keepdims=True) / dtype(T.shape[1]))
    out = P_trans / P_scale * T_scale + (T_mean if translation else 0)
    assert out.dtype == dtype
    return out


def transformed(c, mode, dtype=np.float64, target_of=None, **wrong):
    """(S, P, 3) ``dtype``: the case's predictions after the mode's alignment to target s // group.  ``target_of``: another map from
    set to target index (the host tests' s % group); ``wrong``: the switches of similarity_transform / scale_and_translation."""
    T = targets(c, target_of)
    with np.errstate(invalid="ignore", divide="ignore"):
        if mode == MODE_RAW:
            return c["pred"].astype(dtype)
        if mode == MODE_SC:
            return scale_and_translation(c["pred"], T, dtype, **wrong)
        return np.stack([similarity_transform(c["pred"][s], T[s], dtype, **wrong) for s in range(c["S"])])


def targets(c, target_of=None):
    """(S, P, 3) fp32: the target each set is compared with."""
    idx = [(s // c["group"]) if target_of is None else target_of(s) for s in range(c["S"])]
    return c["target"][idx]


def error_sums(q, T):
    """(S,) float64: per set, the sum over its points of |q - target| in float64."""
    return np.linalg.norm(np.asarray(q, dtype=np.float64) - T.astype(np.float64), axis=-1).sum(-1)


def ill_posed(c, mode):
    """None, "nonfinite" (P = 1, SC / PA) or "sum_only" (collinear target, noisy 3-D prediction, PA): module docstring."""
    if c["P"] == 1 and mode != MODE_RAW:
        return "nonfinite"
    if c["name"] == "collinear_noisy" and mode == MODE_PA:
        return "sum_only"
    return None


@functools.lru_cache(maxsize=None)
def _pointset_reference(name, mode):
    c = pointset_case(name)
    q64, q32 = transformed(c, mode, np.float64), transformed(c, mode, np.float32)
    T = targets(c)
    r = dict(q64=q64, q32=q32, err64=error_sums(q64, T), err32=error_sums(q32, T), ill=ill_posed(c, mode))
    if r["ill"] == "nonfinite":
        r.update(e32=float("nan"), scale=float("nan"), bound_pts=float("nan"), bound_sum=float("nan"))
        return r
    r["e32"] = float(np.abs(q32.astype(np.float64) - q64).max())
    r["scale"] = float(max(np.abs(q64).max(), np.abs(c["pred"]).max()))
    floor = EPS32 * r["scale"]
    r["bound_pts"] = 4.0 * (floor if r["ill"] == "sum_only" else max(r["e32"], floor))
    r["bound_sum"] = math.sqrt(3.0) * c["P"] * r["bound_pts"]
    return r


def pointset_reference(c, mode):
    """q64, q32 (S, P, 3), err64, err32 (S,), e32, scale = max(|q64|, |pred|), bound_pts, bound_sum and ill (ill_posed) of one mode."""
    return _pointset_reference(c["name"], mode)


def check_pointsets(tag, c, mode, err, q=None):
    """Prints the figures, then asserts the rules for a device result: err (S,) error sums and, if given, q (S, P, 3) transformed
    points.  Returns the worst err / bound of what was compared (0.0 for the non-finite case)."""
    r = pointset_reference(c, mode)
    err = np.asarray(err, dtype=np.float64).reshape(-1)
    assert err.shape == (c["S"],), (tag, err.shape)
    if r["ill"] == "nonfinite":
        print("%-28s %-3s %-18s ill-posed (P = 1): device sums %s, reference's %s" % (tag, MODE_NAMES[mode], c["name"], err, r["err32"]))
        assert not np.isfinite(r["err32"]).any()
        assert not np.isfinite(err).any(), (tag, c["name"], mode, err)
        return 0.0
    e_sum = float(np.abs(err - r["err64"]).max())
    ratio = e_sum / r["bound_sum"]
    line = "%-28s %-3s %-18s S=%-3d P=%-4d e32 = %.2e  floor = %.2e  sums: err = %.3e bound = %.3e ratio = %.3f" % (
        tag, MODE_NAMES[mode], c["name"], c["S"], c["P"], r["e32"], EPS32 * r["scale"], e_sum, r["bound_sum"], ratio)
    e_pts = None
    if q is not None and r["ill"] is None:
        q = np.asarray(q, dtype=np.float64)
        assert q.shape == r["q64"].shape, (tag, q.shape)
        e_pts = float(np.abs(q - r["q64"]).max())
        line += "  points: err = %.3e bound = %.3e ratio = %.3f" % (e_pts, r["bound_pts"], e_pts / r["bound_pts"])
        ratio = max(ratio, e_pts / r["bound_pts"])
    print(line)
    assert np.isfinite(err).all() and e_sum <= r["bound_sum"], (tag, c["name"], MODE_NAMES[mode], "sums", e_sum, r["bound_sum"])
    if e_pts is not None:
        assert e_pts == e_pts and e_pts <= r["bound_pts"], (tag, c["name"], MODE_NAMES[mode], "points", e_pts, r["bound_pts"])
    return ratio


# =====================================================================================================================
# checksums
# =====================================================================================================================
# ends of a block (256) and of the grid stride (128 * 256 = 32768), the first and last n around the entry of the eight-deep loop
# (i + 7 * 32768 < n), its second trip (n > 15 * 32768 = 491520), and a length with a ragged tail behind two trips
SUM_LENGTHS = (0, 1, 255, 256, 257, 32767, 32768, 32769, 229375, 229376, 229377, 262149, 491519, 491521, 536633)


@functools.lru_cache(maxsize=None)
def sum_values(n, seed=0):
    """(n,) fp32, read-only: distinct values of mixed signs, 0.05 <= |x|, entries 0, n // 3 and n - 1 a thousand times larger, x[0] < 0."""
    rs = np.random.RandomState(9000 + 7 * n + seed)
    x = rs.randn(n)
    x = (np.sign(x) * (np.abs(x) + 0.05)).astype(np.float32)
    if n:
        for i in {0, n // 3, n - 1}:
            x[i] *= np.float32(1000.0)
        x[0] = -abs(x[0])
    for _ in range(64):                                          # re-draw repeated values until all are distinct
        _, first = np.unique(x, return_index=True)
        dup = np.setdiff1d(np.arange(n), first)
        if dup.size == 0:
            break
        d = rs.randn(dup.size)
        x[dup] = (np.sign(d) * (np.abs(d) + 0.05)).astype(np.float32)
    assert np.unique(x).size == n
    x.setflags(write=False)
    return x


def sum_truth(x, take_abs):
    v = np.abs(x) if take_abs else x
    return math.fsum(v.astype(np.float64).tolist())


def sum_bound(x):
    return x.size * 2.0 ** -53 * math.fsum(np.abs(x).astype(np.float64).tolist())


def check_sum(tag, got, x, take_abs):
    """Prints the figures, asserts |got - fsum| <= n 2^-53 sum|x|; returns err / bound (0.0 where both are zero)."""
    want, b = sum_truth(x, take_abs), sum_bound(x)
    err = abs(float(got) - want)
    print("%-34s n=%-7d abs=%d  got = %.17g  fsum = %.17g  err = %.3e  bound = %.3e" % (tag, x.size, int(bool(take_abs)), float(got), want, err, b))
    assert err == err and err <= b, (tag, x.size, take_abs, float(got), want, err, b)
    return err / b if b > 0 else 0.0


# =====================================================================================================================
# heat-maps
# =====================================================================================================================
# (60, 60): 900 float4 -- lanes 0..131 take the four-deep loop, lanes 132..255 the float4 tail for the same elements' neighbours
HEAT_SHAPES = ((1, 1), (7, 9), (31, 64), (64, 64), (96, 72), (256, 256), (60, 60))
HEAT_EPS = 1e-6                     # the product's default; the kernel receives it as fp32
PATH_MAIN, PATH_TAIL4, PATH_SCALAR = 0, 1, 2


def load_paths(HW, aligned):
    """(HW,) int: which loop of heatmap_argmax_kernel loads each element -- the four-deep float4 loop (a lane's trip k runs while
    lane + 768 + 1024 k < HW / 4), the float4 tail, or the scalar loop (everything when HW % 4 != 0 or the map is not 16-byte aligned)."""
    n4 = HW // 4 if (HW % 4 == 0 and aligned) else 0
    i4 = np.arange(n4)
    main = (i4 % 256) + 768 + 1024 * (i4 // 1024) < n4
    path = np.full(HW, PATH_SCALAR)
    path[:4 * n4] = np.repeat(np.where(main, PATH_MAIN, PATH_TAIL4), 4)
    return path


def heat_placements(H, W, aligned):
    """[(label, positions, value)]: one map each -- ``value`` written at the flat ``positions`` of a map of small random values."""
    HW = H * W
    path = load_paths(HW, aligned)
    one = np.float32(1.0)
    out = [("max at index 0", (0,), one), ("max at the last index", (HW - 1,), one)]
    ends = []
    for p, pname in ((PATH_MAIN, "float4 loop"), (PATH_TAIL4, "float4 tail"), (PATH_SCALAR, "scalar loop")):
        idx = np.nonzero(path == p)[0]
        if idx.size:
            ends.append((int(idx[0]), int(idx[-1])))
            out += [("max at the first element of the %s" % pname, (int(idx[0]),), one),
                    ("max at the last element of the %s" % pname, (int(idx[-1]),), one)]
    if len(ends) >= 2:                                           # a tie between two positions in different paths
        out.append(("tie across load paths", (ends[0][1], ends[1][0] + min(5, ends[1][1] - ends[1][0])), one))
        out.append(("tie across load paths, far apart", (ends[0][0] + min(3, ends[0][1]), ends[1][1]), one))
    else:
        out.append(("tie of the first and the last element", (0, HW - 1), one))
    lane = 4 if path[0] != PATH_SCALAR else 1                    # elements per lane and pass
    if 64 * lane < HW:
        out.append(("tie of lanes 63 and 64 of one pass", (63 * lane + lane - 1, 64 * lane), one))
    if 65 * lane < HW:
        out.append(("tie of lanes 63 and 64, inner elements", (63 * lane, 64 * lane + lane - 1), one))
    if 266 * lane + 2 < HW:                                      # the lower index sits in the higher lane (200) of the earlier pass
        out.append(("tie of lane 200, pass 0 and lane 10, pass 1", (200 * lane + lane - 1, 266 * lane), one))
    if 3 * 64 * lane + 1 < HW:                                   # a three-way tie whose lowest index the last wavefront holds
        a = 3 * 64 * lane + 1
        out.append(("three-way tie over wavefronts", (a, min(a + 1, HW - 1), HW - 1), one))
    eps32 = np.float32(HEAT_EPS)
    out += [("all zero (invisible)", (), None),
            ("max equals eps exactly (invisible)", (HW // 2,), eps32),
            ("max one ulp above eps (visible)", (HW // 2,), np.nextafter(eps32, np.float32(1.0))),
            ("max equals eps exactly at the last index (invisible)", (HW - 1,), eps32)]
    return out


@functools.lru_cache(maxsize=None)
def heat_case(H, W, aligned=True):
    """(heat (1, M, H, W) fp32 read-only, labels): the maps of heat_placements over seeded backgrounds (values in [0, 0.5), far below 1;
    below eps / 2 where the map's maximum is about eps; no NaN)."""
    rs = np.random.RandomState(31 * H + W + 1000 * int(aligned))
    plc = heat_placements(H, W, aligned)
    heat = np.zeros((1, len(plc), H * W), dtype=np.float32)
    for m, (label, pos, value) in enumerate(plc):
        if value is None:
            continue
        top = 0.5 if value == np.float32(1.0) else 0.5 * HEAT_EPS
        heat[0, m] = (rs.rand(H * W) * top).astype(np.float32)
        heat[0, m, list(pos)] = value
    heat = heat.reshape(1, len(plc), H, W)
    heat.setflags(write=False)
    return heat, tuple(p[0] for p in plc)


def heat_truth(heat, eps=HEAT_EPS, tie="first", visible=lambda mx, eps: mx > eps):
    """(joints (N, K, 2) fp32, vis (N, K) bool) by numpy.argmax; invisible joints are (-1, -1).  ``tie`` = "last" and another
    ``visible`` are the wrong kernels of the host tests."""
    N, K, H, W = heat.shape
    flat = heat.reshape(N, K, H * W)
    assert not np.isnan(flat).any()
    idx = np.argmax(flat, axis=-1) if tie == "first" else H * W - 1 - np.argmax(flat[..., ::-1], axis=-1)
    mx = flat.max(axis=-1)
    vis = visible(mx, np.float32(eps))
    j = np.stack([idx % W, np.floor(idx / float(W))], axis=-1).astype(np.float32)
    j[~vis] = -1.0
    return j, vis


def check_heat(tag, j, vis, heat, labels, eps=HEAT_EPS):
    """Exact equality with heat_truth, map by map (the failing map's label in the message)."""
    jw, vw = heat_truth(heat, eps)
    j, vis = np.asarray(j, dtype=np.float32).reshape(jw.shape), np.asarray(vis).astype(bool).reshape(vw.shape)
    for m, label in enumerate(labels):
        assert np.array_equal(j[0, m], jw[0, m]) and vis[0, m] == vw[0, m], (tag, heat.shape, label, j[0, m], vis[0, m], jw[0, m], vw[0, m])
    return len(labels)


# =====================================================================================================================
# proxy representation
# =====================================================================================================================
# (B, K, H, W, std): no joint; one pixel; a second column block with a ragged row block; K at its limit with W = 256 + 1; the product's
PROXY_CASES = ((1, 0, 8, 8, 4.0), (3, 1, 1, 1, 4.0), (2, 17, 13, 300, 2.5), (1, 32, 9, 257, 3.0), (2, 17, 64, 64, 4.0))


@functools.lru_cache(maxsize=None)
def proxy_case(cfg):
    """dict(edge (B, 1, H, W), joints (B, K, 2) (u = column, v = row), vis (B, K)) fp32 torch tensors: fractional joints inside the image,
    on its border, outside it and negative; about a quarter of the visibilities zero."""
    B, K, H, W, std = cfg
    g = torch.Generator().manual_seed(B + 10 * K + 100 * H + 1000 * W)
    j = torch.rand(B, K, 2, generator=g) * torch.tensor([float(W), float(H)])
    special = [(0.0, 0.0), (W - 1.0, H - 1.0), (-3.25, 0.5 * H), (0.5 * W, -7.5), (W + 5.75, H + 2.5), (-0.5, -0.5), (W - 0.5, 0.0)]
    for k in range(min(K, len(special))):
        j[k % B, k] = torch.tensor(special[k])
    vis = (torch.rand(B, K, generator=g) > 0.25).float()
    edge = torch.rand(B, 1, H, W, generator=g)
    edge[edge < 0.5] = 0.0
    return dict(cfg=cfg, B=B, K=K, H=H, W=W, std=std, edge=edge, joints=j, vis=vis)


def proxy_heat(c, dtype, with_vis=True):
    """(B, K, H, W) ``dtype``: the formula of utils/label_conversions.py:123 on an H x W grid, times the visibility."""
    ii, jj = torch.meshgrid(torch.arange(c["H"]), torch.arange(c["W"]), indexing="ij")
    ii, jj = ii[None, None].to(dtype), jj[None, None].to(dtype)
    u = c["joints"].to(dtype)[:, :, 0, None, None]
    v = c["joints"].to(dtype)[:, :, 1, None, None]
    heat = torch.exp(-(((ii - v) / c["std"]) ** 2) / 2 - (((jj - u) / c["std"]) ** 2) / 2)
    assert heat.dtype == dtype
    return heat * c["vis"].to(dtype)[:, :, None, None] if with_vis else heat


@functools.lru_cache(maxsize=None)
def _proxy_reference(cfg, with_vis):
    c = proxy_case(cfg)
    h64, h32 = proxy_heat(c, torch.float64, with_vis), proxy_heat(c, torch.float32, with_vis)
    e32 = float((h32.double() - h64).abs().max()) if h64.numel() else 0.0
    return dict(h64=h64, h32=h32, e32=e32, bound=4.0 * max(e32, EPS32))


def proxy_reference(c, with_vis=True):
    return _proxy_reference(c["cfg"], with_vis)


def check_proxy(tag, out, c, with_vis=True, with_edge=True):
    """out (B, K + 1, H, W): channels 1.. against the float64 heat-maps within the bound, channel 0 equal to the edge plane bit for bit
    (``with_edge`` False: not looked at).  Returns err / bound."""
    r = proxy_reference(c, with_vis)
    out = out.detach().cpu()
    assert out.shape == (c["B"], c["K"] + 1, c["H"], c["W"]) and out.dtype == torch.float32, (tag, tuple(out.shape))
    if with_edge:
        assert torch.equal(out[:, :1], c["edge"]), (tag, "channel 0 is not the edge plane")
    err = float((out[:, 1:].double() - r["h64"]).abs().max()) if c["K"] else 0.0
    print("%-30s %-22s vis=%d  e32 = %.2e  err = %.3e  bound = %.3e  ratio = %.3f" % (tag, c["cfg"], with_vis, r["e32"], err, r["bound"], err / r["bound"]))
    assert err == err and err <= r["bound"], (tag, c["cfg"], err, r["bound"])
    return err / r["bound"]


# =====================================================================================================================
# sample 2-D error
# =====================================================================================================================
SAMPLE_NS = (1, 63, 64, 65, 130)
COCO_MAP = (24, 26, 25, 28, 27, 16, 17, 18, 19, 20, 21, 1, 2, 4, 5, 7, 8)          # label_conversions.ALL_JOINTS_TO_COCO_MAP
IMG_WH = 256.0


@functools.lru_cache(maxsize=None)
def sample_case(N, all_invisible=False):
    """dict(joints (N, 90, 3), in_j2d (17, 2), in_vis (17,), cam (3,)) fp32 torch tensors; joints 7 and 9 invisible (or all of them)."""
    g = torch.Generator().manual_seed(600 + N)
    joints = torch.randn(N, 90, 3, generator=g) * 0.4
    in_j2d = torch.rand(17, 2, generator=g) * 200 + 20
    vis = torch.ones(17)
    vis[[7, 9]] = 0.0
    if all_invisible:
        vis[:] = 0.0
    in_j2d[vis == 0] = -1.0
    return dict(N=N, joints=joints, in_j2d=in_j2d, in_vis=vis, cam=torch.tensor([0.9, 0.05, -0.1]), all_invisible=all_invisible)


def sample_projection(c, dtype):
    """(N, 17, 2) ``dtype``: the projected COCO joints in pixels, as oracle.joints2d_error_sorted forms them."""
    cam = c["cam"].to(dtype)[None]
    jc = c["joints"].to(dtype)[:, list(COCO_MAP), :] * torch.tensor([1.0, -1.0, -1.0], dtype=dtype)
    proj = cam[:, None, [0]] * (jc[:, :, :2] + cam[:, None, 1:])
    return (proj + 1) * (IMG_WH / 2.0)


def sample_errors(c, dtype):
    """(N,) ``dtype``: per sample, the largest distance over the visible joints (in front of the reference's sort)."""
    proj, keep = sample_projection(c, dtype), c["in_vis"] > 0
    l2 = torch.norm(proj[:, keep, :] - c["in_j2d"].to(dtype)[None, keep, :], dim=-1)
    assert l2.dtype == dtype
    return l2.max(dim=-1)[0]


@functools.lru_cache(maxsize=None)
def _sample_reference(N):
    c = sample_case(N)
    e64, e32, proj = sample_errors(c, torch.float64), sample_errors(c, torch.float32), sample_projection(c, torch.float64)
    err32 = float((e32.double() - e64).abs().max())
    scale = max(float(proj.abs().max()), IMG_WH)
    return dict(e64=e64, e32=e32, err32=err32, scale=scale, bound=4.0 * max(err32, EPS32 * scale))


def sample_reference(c):
    assert not c["all_invisible"]
    return _sample_reference(c["N"])


def check_sample_errors(tag, got, c):
    r = sample_reference(c)
    got = got.detach().cpu().double().reshape(-1)
    assert got.shape == r["e64"].shape, (tag, tuple(got.shape))
    err = float((got - r["e64"]).abs().max())
    print("%-24s N=%-4d e32 = %.2e  floor = %.2e  err = %.3e  bound = %.3e  ratio = %.3f" % (tag, c["N"], r["err32"], EPS32 * r["scale"], err, r["bound"], err / r["bound"]))
    assert err == err and err <= r["bound"], (tag, c["N"], err, r["bound"])
    return err / r["bound"]
