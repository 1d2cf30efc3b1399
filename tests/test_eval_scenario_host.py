"""The evaluation and front-end kernel tests' references and accuracy rules on their own (tests/eval_scenario.py; no device): every
fp32 restatement of every case of tests/test_gpu_eval_kernels.py stays inside its bound, the float64 truth is the oracle's, and the rules
have teeth -- a kernel that drops or repeats a point, takes s % group for s // group, loses the determinant fix, the Procrustes scale or
the translation, drops, repeats or does not abs a checksum element, returns the last of two tied maxima or tests visibility with >= is
each caught.  The argument checks of the entry points, which return before any launch, run here too (the library loads without a device)."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import eval_scenario as E
from hierarchicalprobabilistic3dhuman_amd import _capi
from oracle import ref_cpu as O


# ---------------------------------------------------------------------------------------------------------------------
# point sets
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,names", E.POINTSET_FAMILIES, ids=[f for f, _ in E.POINTSET_FAMILIES])
def test_pointset_restatements_stay_inside_the_bound(family, names):
    for name in names:
        c = E.pointset_case(name)
        assert c["pred"].dtype == np.float32 and c["target"].dtype == np.float32
        assert c["target"].shape == (-(-c["S"] // c["group"]), c["P"], 3)
        for mode in E.MODES:
            r = E.pointset_reference(c, mode)
            assert r["q64"].dtype == np.float64 and r["q32"].dtype == np.float32
            E.check_pointsets("cpu32", c, mode, r["err32"], r["q32"])
            E.check_pointsets("f64", c, mode, r["err64"], r["q64"])


def test_pointset_truth_is_the_oracle_in_float64():
    for name in ("P14", "P257", "reflected", "coplanar_noisy", "offset"):
        c = E.pointset_case(name)
        p, t = c["pred"].astype(np.float64), E.targets(c).astype(np.float64)
        assert np.array_equal(E.pointset_reference(c, E.MODE_PA)["q64"], O.procrustes_analysis_batch(p, t))
        assert np.array_equal(E.pointset_reference(c, E.MODE_SC)["q64"], O.scale_and_translation_transform_batch(p, t))
        assert np.array_equal(E.pointset_reference(c, E.MODE_RAW)["q64"], p)


def test_exact_similarity_transform_is_recovered():
    for name in ("exact_similarity", "coplanar_clean", "collinear_clean"):
        c = E.pointset_case(name)
        # a transform built in float64 is recovered to 1e-9; from the case's fp32 inputs the truth is a few fp32 roundings of the
        # data away from the target
        # (not the collinear target: rounded to fp32 it is 1e-8 off its line, and the undetermined rotation about the line moves that)
        if name != "collinear_clean":
            rs = np.random.RandomState(5)
            t = E.targets(c)[0].astype(np.float64)
            p = E._similar(rs, t, 0.0)
            assert np.abs(E.similarity_transform(p, t, np.float64) - t).max() <= 1e-9
        r = E.pointset_reference(c, E.MODE_PA)
        assert np.abs(r["q64"] - E.targets(c)).max() <= 8 * E.EPS32 * r["scale"]
    c = E.pointset_case("copy")
    assert np.abs(E.pointset_reference(c, E.MODE_PA)["q64"] - c["target"]).max() <= 1e-12


def test_ill_posed_inputs_are_the_two_stated_ones():
    ill = {(n, m): E.ill_posed(E.pointset_case(n), m) for n in E.POINTSET_CASES for m in E.MODES}
    assert {k for k, v in ill.items() if v} == {("P1", E.MODE_SC), ("P1", E.MODE_PA), ("collinear_noisy", E.MODE_PA)}
    assert ill[("P1", E.MODE_SC)] == ill[("P1", E.MODE_PA)] == "nonfinite" and ill[("collinear_noisy", E.MODE_PA)] == "sum_only"
    # the reference's fp32 points are off by O(0.1) on the collinear target, its sum is not
    r = E.pointset_reference(E.pointset_case("collinear_noisy"), E.MODE_PA)
    assert r["e32"] > 0.01 and np.abs(r["err32"] - r["err64"]).max() <= r["bound_sum"]
    assert r["bound_pts"] == 4 * E.EPS32 * r["scale"]


def _caught(c, mode, err, q=None):
    with pytest.raises(AssertionError):
        E.check_pointsets("mutant", c, mode, err, q)


@pytest.mark.parametrize("P", [p for p in E.SIZES if p >= 2])
def test_a_dropped_or_repeated_point_is_caught(P):
    c = E.pointset_case("P%d" % P)
    T = E.targets(c)
    for mode in E.MODES:
        r = E.pointset_reference(c, mode)
        # the last point left out of the second set's sum (P = 2, PA: the fit of two points is exact, the term is zero -- no defect)
        if not (P == 2 and mode == E.MODE_PA):
            err = r["err64"].copy()
            err[1] = np.linalg.norm(r["q64"][1, :-1] - T[1, :-1], axis=-1).sum()
            _caught(c, mode, err)
        # point 256 k processed in place of point 256 k + 1 (the next lane's), in the points and in the sum
        for k in range((P - 2) // 256 + 1):
            q = r["q64"].copy()
            q[0, 256 * k + 1] = q[0, 256 * k]
            _caught(c, mode, E.error_sums(q, T), q)
            _caught(c, mode, E.error_sums(q, T))                           # the sum alone shows it too
            _caught(c, mode, r["err64"], q)


@pytest.mark.parametrize("name", ["g7x3", "g8x4"])
def test_the_wrong_target_of_a_group_is_caught(name):
    c = E.pointset_case(name)
    n_t = c["target"].shape[0]
    wrong = lambda s: (s % c["group"]) % n_t
    for mode in E.MODES:
        q = E.transformed(c, mode, np.float64, target_of=wrong)
        _caught(c, mode, E.error_sums(q, E.targets(c, wrong)))
        if mode != E.MODE_RAW:
            _caught(c, mode, E.pointset_reference(c, mode)["err64"], q)


def test_wrong_procrustes_kernels_are_caught():
    c = E.pointset_case("reflected")
    T = E.targets(c)
    q = E.transformed(c, E.MODE_PA, np.float64, det_fix=False)                # the improper rotation fits the reflected copy far better
    assert E.error_sums(q, T).max() < 0.5 * E.pointset_reference(c, E.MODE_PA)["err64"].min()
    _caught(c, E.MODE_PA, E.error_sums(q, T), q)
    _caught(c, E.MODE_PA, E.error_sums(q, T))
    for name in ("P14", "P1100", "slab", "scale_1e3"):
        c = E.pointset_case(name)
        T = E.targets(c)
        q = E.transformed(c, E.MODE_PA, np.float64, sc_scale=True)            # the SC mode's scale in the PA mode
        _caught(c, E.MODE_PA, E.error_sums(q, T), q)
        _caught(c, E.MODE_PA, E.error_sums(q, T))
    c = E.pointset_case("offset")
    T = E.targets(c)
    for mode in (E.MODE_SC, E.MODE_PA):
        q = E.transformed(c, mode, np.float64, translation=False)
        _caught(c, mode, E.error_sums(q, T), q)
        _caught(c, mode, E.error_sums(q, T))


# ---------------------------------------------------------------------------------------------------------------------
# checksums
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", E.SUM_LENGTHS)
def test_checksum_rule_and_its_mutants(n):
    x = E.sum_values(n)
    assert x.dtype == np.float32 and x.shape == (n,) and np.unique(x).size == n
    x64 = x.astype(np.float64)
    for take_abs in (0, 1):
        v = np.abs(x64) if take_abs else x64
        # legitimate float64 summations: numpy's pairwise one, a strictly sequential one, the kernel's order restated (a lane sums its
        # elements i, i + 32768, ... in index order; 256 lanes by a tree; 128 blocks in sequence)
        assert E.check_sum("pairwise", v.sum(), x, take_abs) <= 1.0
        assert E.check_sum("sequential", float(np.cumsum(v)[-1]) if n else 0.0, x, take_abs) <= 1.0
        pad = np.zeros(-(-max(n, 1) // 32768) * 32768)
        pad[:n] = v
        lanes = np.zeros(32768)
        for row in pad.reshape(-1, 32768):
            lanes = lanes + row
        blocks = lanes.reshape(128, 256)
        s = 128
        while s:
            blocks = blocks[:, :s] + blocks[:, s:2 * s]
            s //= 2
        total = 0.0
        for b in blocks[:, 0]:
            total += float(b)
        assert E.check_sum("kernel order", total, x, take_abs) <= 1.0
    if n == 0:
        assert E.sum_truth(x, 0) == 0.0 and E.sum_bound(x) == 0.0
        return
    assert x[0] < 0 and float(np.abs(x).min()) >= 0.05 and float(np.abs(x).max()) >= 50.0
    for take_abs in (0, 1):
        v = np.abs(x64) if take_abs else x64
        for pos in sorted({0, n // 2, n - 1}):
            with pytest.raises(AssertionError):                                # one element dropped
                E.check_sum("dropped", math.fsum(np.delete(v, pos).tolist()), x, take_abs)
            with pytest.raises(AssertionError):                                # one element repeated (read twice)
                E.check_sum("repeated", math.fsum(v.tolist() + [v[pos]]), x, take_abs)
            if n > 1:
                w = v.copy()
                w[pos] = v[pos - 1]                                            # the neighbour read in its place
                with pytest.raises(AssertionError):
                    E.check_sum("neighbour", math.fsum(w.tolist()), x, take_abs)
    with pytest.raises(AssertionError):                                        # abs missing / abs where none was asked
        E.check_sum("abs missing", E.sum_truth(x, 0), x, 1)
    with pytest.raises(AssertionError):
        E.check_sum("abs unasked", E.sum_truth(x, 1), x, 0)


# ---------------------------------------------------------------------------------------------------------------------
# heat-maps
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("H,W", E.HEAT_SHAPES)
def test_heatmap_truth_and_its_mutants(H, W, aligned):
    heat, labels = E.heat_case(H, W, aligned)
    assert heat.dtype == np.float32 and heat.shape == (1, len(labels), H, W) and not np.isnan(heat).any()
    j, vis = E.heat_truth(heat)
    jo, vo = O.heatmaps_to_joints2d(torch.from_numpy(heat.copy()))             # the oracle's torch.max route agrees with numpy's
    assert np.array_equal(j, jo.numpy()) and np.array_equal(vis, vo.numpy())
    assert E.check_heat("truth", j, vis, heat, labels) == len(labels)
    path = E.load_paths(H * W, aligned)
    if not aligned or (H * W) % 4:
        assert (path == E.PATH_SCALAR).all()
    for m, label in enumerate(labels):
        flat = heat[0, m].reshape(-1)
        if "invisible" in label:
            assert not vis[0, m] and (j[0, m] == -1).all()
        else:
            assert vis[0, m] and j[0, m, 1] * W + j[0, m, 0] == np.nonzero(flat == flat.max())[0][0]
    n_ties = sum(1 for label in labels if "tie" in label and H * W > 1)
    assert n_ties >= 1 or H * W == 1
    if (H, W) in ((96, 72), (60, 60)) and aligned:
        assert set(path) == {E.PATH_MAIN, E.PATH_TAIL4} and any("across load paths" in label for label in labels)
    if H * W > 1:
        jl, vl = E.heat_truth(heat, tie="last")                                # the last of the tied indices returned
        with pytest.raises(AssertionError, match="tie"):
            E.check_heat("last of a tie", jl, vl, heat, labels)
    jg, vg = E.heat_truth(heat, visible=lambda mx, eps: mx >= eps)             # >= in the visibility test
    with pytest.raises(AssertionError, match="equals eps"):
        E.check_heat(">=", jg, vg, heat, labels)


def test_load_paths_restate_the_kernels_partition():
    """Lane by lane, as the kernel's three loops run."""
    for HW, aligned in ((3600, True), (6912, True), (4096, True), (1984, True), (63, True), (4096, False), (1, True)):
        want = np.full(HW, -1)
        n4 = HW // 4 if (HW % 4 == 0 and aligned) else 0
        for lane in range(256):
            i = lane
            while i + 3 * 256 < n4:
                for q in range(4):
                    want[4 * (i + q * 256):4 * (i + q * 256) + 4] = E.PATH_MAIN
                i += 4 * 256
            while i < n4:
                want[4 * i:4 * i + 4] = E.PATH_TAIL4
                i += 256
            want[4 * n4 + lane:HW:256] = E.PATH_SCALAR
        assert np.array_equal(want, E.load_paths(HW, aligned)), (HW, aligned)


# ---------------------------------------------------------------------------------------------------------------------
# proxy representation, sample 2-D error
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", E.PROXY_CASES, ids=lambda c: "x".join(str(v) for v in c[:4]))
def test_proxy_restatement_stays_inside_the_bound(cfg):
    c = E.proxy_case(cfg)
    B, K, H, W, std = cfg
    for with_vis in (True, False):
        r = E.proxy_reference(c, with_vis)
        assert r["h64"].dtype == torch.float64 and r["h32"].dtype == torch.float32 and r["h64"].shape == (B, K, H, W)
        E.check_proxy("cpu32", torch.cat([c["edge"], r["h32"]], 1), c, with_vis)
    if H == W and K:
        assert torch.equal(E.proxy_reference(c, False)["h32"], O.joints2d_to_gaussian_heatmaps(c["joints"], H, std))
    if K >= 7:
        j = c["joints"].reshape(-1, 2)
        assert bool((j < 0).any()) and bool((j[:, 0] > W).any()) and bool((j != j.round()).any()) and bool((c["vis"] == 0).any())
        bad = torch.cat([c["edge"], E.proxy_reference(c, True)["h32"]], 1).clone()
        for what in ("rows and columns exchanged", "visibility ignored", "edge plane off by one ulp"):
            d = bad.clone()
            if what.startswith("rows"):
                jt = dict(c, joints=c["joints"].flip(-1))
                d[:, 1:] = E.proxy_heat(jt, torch.float32)
            elif what.startswith("vis"):
                d[:, 1:] = E.proxy_reference(c, False)["h32"]
            else:
                d[0, 0, H // 2, W // 2] = torch.nextafter(d[0, 0, H // 2, W // 2] + 0.5, torch.tensor(2.0))
            with pytest.raises(AssertionError):
                E.check_proxy(what, d, c, True)


@pytest.mark.parametrize("N", E.SAMPLE_NS)
def test_sample_error_restatement_stays_inside_the_bound(N):
    c = E.sample_case(N)
    r = E.sample_reference(c)
    E.check_sample_errors("cpu32", r["e32"], c)
    # the truth is the oracle's expression: its ordering is the ordering of these errors
    heat = torch.zeros(1, 17, 256, 256)
    for k in range(17):
        if c["in_vis"][k] > 0:
            heat[0, k, int(c["in_j2d"][k, 1]), int(c["in_j2d"][k, 0])] = 1.0
    cc = dict(c, in_j2d=torch.where(c["in_vis"][:, None] > 0, c["in_j2d"].floor(), c["in_j2d"]))
    verts = torch.arange(N, dtype=torch.float32).reshape(N, 1, 1).expand(N, 2, 3)
    _, order = O.joints2d_error_sorted(verts, c["joints"], heat, c["cam"][None], list(E.COCO_MAP))
    assert torch.equal(order, torch.sort(E.sample_errors(cc, torch.float32), stable=True)[1])
    # a kernel that looks at an invisible joint, or misses the last visible one, is caught
    for keep in (torch.ones(17), torch.cat([c["in_vis"][:16], torch.zeros(1)])):
        if N < 63:
            continue
        bad = E.sample_errors(dict(c, in_vis=keep), torch.float32)
        with pytest.raises(AssertionError):
            E.check_sample_errors("wrong joints", bad, c)


# ---------------------------------------------------------------------------------------------------------------------
# argument checks that return before any launch
# ---------------------------------------------------------------------------------------------------------------------
def test_argument_checks_return_before_any_launch():
    if not os.path.exists(_capi.LIB_PATH):
        pytest.skip("libhps.so is not built")
    lib = _capi.load()
    P = ctypes.c_void_p
    buf = (ctypes.c_double * 64)()                                   # host memory: never dereferenced by a call that returns here
    a = ctypes.cast(buf, P)
    xs, ns, ab = (P * 4)(a, a, a, a), (ctypes.c_int64 * 4)(1, 1, 1, 1), (ctypes.c_int32 * 4)(0, 0, 0, 0)

    def refused(rc, text):
        assert rc == -1, rc                                          # HPS_E_BADARG
        msg = lib.hps_last_error()
        assert msg.startswith(b"bad argument") and text in msg, msg

    refused(lib.hps_sums_f64(xs, ns, ab, 0, 0.0, a, a, None, None), b"1..4 tensors")
    refused(lib.hps_sums_f64(xs, ns, ab, 5, 0.0, a, a, None, None), b"1..4 tensors")
    refused(lib.hps_sums_f64(None, ns, ab, 1, 0.0, a, a, None, None), b"null pointer")
    refused(lib.hps_sums_f64(xs, None, ab, 1, 0.0, a, a, None, None), b"null pointer")
    refused(lib.hps_sums_f64((P * 4)(a, None, a, a), ns, ab, 2, 0.0, a, a, None, None), b"tensor")
    refused(lib.hps_sums_f64(xs, (ctypes.c_int64 * 4)(1, -1, 1, 1), ab, 2, 0.0, a, a, None, None), b"tensor")
    refused(lib.hps_pointset_errors(a, a, 1, 0, 14, 0, a, a, a, None, None), b"group / P / mode")
    refused(lib.hps_pointset_errors(a, a, 1, 1, 0, 0, a, a, a, None, None), b"group / P / mode")
    refused(lib.hps_pointset_errors(a, a, 1, 1, 14, 3, a, a, a, None, None), b"group / P / mode")
    refused(lib.hps_pointset_errors(a, a, 1, 1, 14, -1, a, a, a, None, None), b"group / P / mode")
    refused(lib.hps_pointset_errors(None, a, 1, 1, 14, 0, a, a, a, None, None), b"null pointer")
    refused(lib.hps_proxy_rep(a, a, a, a, 1, 33, 8, 8, 4.0, None), b"at most 32 joints")
    refused(lib.hps_proxy_rep(a, a, a, a, 1, -1, 8, 8, 4.0, None), b"at most 32 joints")
    refused(lib.hps_proxy_rep(a, None, a, a, 1, 17, 8, 8, 4.0, None), b"null pointer")
    taps = (ctypes.c_float * 5)(0.1, 0.2, 0.4, 0.2, 0.1)
    refused(lib.hps_canny_edge_map(a, ctypes.cast(taps, P), 5, a, 8 * 8 - 1, 1, 3, 8, 8, 0.0, 1, None), b"edge_batch_stride")
    refused(lib.hps_heatmaps_to_joints2d(None, a, a, 1, 8, 8, 1e-6, None), b"null pointer")
    refused(lib.hps_sample_joints2d_error(a, None, 90, a, a, a, 256.0, a, 1, 17, None), b"null pointer")
