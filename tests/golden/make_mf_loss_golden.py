"""Generates tests/golden/mf_loss_vectors.npz by IMPORTING THE REFERENCE's losses/matrix_fisher_loss.py (only possible where the
reference checkout exists).  What is committed is data: the reference's results, and the inputs too small to need a recipe.

    python tests/golden/make_mf_loss_golden.py            # write the file
    python tests/golden/make_mf_loss_golden.py --check    # regenerate in memory and report max |delta| against the committed file

Contents (results of the reference run in float64 on the fp32 inputs, rounded to fp32 -- except the S sweep, kept in fp64):
  sweep_S (40,3) fp32        make_golden.py's 7-row concentration sweep (rows 0-6), zeros, equal values, factor arguments straddling
                             3.75, negative s3, tiny values, (2000, 1500, 1000), (1e4, 9e3, 8e3), 15 log-uniform rows in [1e-3, 1e4]
  sweep_logc_f64 / sweep_dlogc_f64   LogMFNormConstant and the gradient of its sum, reference in float64
  sweep_logc_f32 / sweep_dlogc_f32   the same, reference in float32 (rows 0-6 of the gradient equal reference_vectors.npz's
                                     sweep_dlogc_dS)
  nll_<case>_{F,U,S,V,R,gw}  matrix_fisher_nll inputs: U, S, V = torch.svd(F) (about half the rows with det(U V^T) = -1); in the n40
                             cases rows 0-3 get non-orthogonal U, V; gw weights the rows of the NLL whose sum is differentiated
  nll_<case>_overreg, nll_<case>_{nll,gF,gS}    overreg, and the reference's values and gradients of sum(gw * nll) (F, S)
  loss_<case>_total, loss_<case>_g<name>        PoseMFShapeGaussianLoss for the cases of tests/mf_loss_scenario.py (inputs rebuilt
                             there from seeded torch.rand recipes): the total and the gradient of every prediction leaf; for b72
                             (the training shape B = 72, Ns = 9, 6890 vertices) every gradient but the vertices'
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
OUT = os.path.join(HERE, "mf_loss_vectors.npz")
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mf_loss_scenario as SC  # noqa: E402

SWEEP = [[0., 0., 0.], [1.9, .78, .6], [5., 5., 5.], [20., 15., 10.], [100., 80., 50.], [500., 400., 300.], [50., 1., .1],
         [2., 2., 2.], [10., 10., 10.], [3., 3., 0.],
         [6., 5., .5], [4., 3.76, 0.], [3.75, 3.75, 3.75], [8., 4., .2], [4.5, .5, .25],
         [5., 3., -1.], [20., 15., -10.], [1., .5, -.5], [300., 200., -100.],
         [1e-3, 1e-4, 1e-5], [1e-5, 1e-5, 1e-5], [1e-3, 1e-3, 0.], [1e-4, 0., 0.],
         [2000., 1500., 1000.], [1e4, 9e3, 8e3]]


def f32(t):
    return t.detach().float().numpy()


def main(check=False):
    sys.path.insert(0, REF)
    from losses.matrix_fisher_loss import LogMFNormConstant, matrix_fisher_nll, PoseMFShapeGaussianLoss

    out = {}
    # ---- the S sweep ----
    g = torch.Generator().manual_seed(2024)
    rnd = torch.sort(10.0 ** (torch.rand(15, 3, generator=g, dtype=torch.float64) * 7.0 - 3.0), dim=1, descending=True).values
    S = torch.cat([torch.tensor(SWEEP, dtype=torch.float32), rnd.float()])
    out["sweep_S"] = S.numpy()
    for tag, dt in (("f64", torch.float64), ("f32", torch.float32)):
        Sg = S.to(dt).requires_grad_(True)
        logc = LogMFNormConstant.apply(Sg)
        logc.sum().backward()
        out["sweep_logc_" + tag], out["sweep_dlogc_" + tag] = logc.detach().numpy(), Sg.grad.numpy()
    old = np.load(os.path.join(HERE, "reference_vectors.npz"))["sweep_dlogc_dS"]
    assert np.array_equal(out["sweep_dlogc_f32"][:7], old), "sweep rows 0-6 no longer reproduce reference_vectors.npz"
    # ---- matrix_fisher_nll ----
    g = torch.Generator().manual_seed(7)
    for case, shape, overreg, spread in (("b3", (3, 23), 1.025, 2.0), ("n40_or1", (40,), 1.0, 5.0), ("n40_or1005", (40,), 1.005, 60.0)):
        F = (torch.rand(*shape, 3, 3, generator=g) * 2.0 - 1.0) * spread
        U, Sv, V = torch.svd(F)
        if len(shape) == 1:
            U[:4] = U[:4] + (torch.rand(4, 3, 3, generator=g) - 0.5) * 0.1
            V[:4] = V[:4] + (torch.rand(4, 3, 3, generator=g) - 0.5) * 0.1
        R = SC.rotmats(g, int(np.prod(shape))).view(*shape, 3, 3)
        gw = torch.rand(*shape, generator=g) + 0.5
        for k, v in (("F", F), ("U", U), ("S", Sv), ("V", V), ("R", R), ("gw", gw)):
            out["nll_%s_%s" % (case, k)] = f32(v.contiguous())
        out["nll_%s_overreg" % case] = np.float64(overreg)
        F64, S64 = F.double().requires_grad_(True), Sv.double().requires_grad_(True)
        nll = matrix_fisher_nll(F64, U.double(), S64, V.double(), R.double(), overreg=overreg)
        (nll * gw.double().reshape(-1)).sum().backward()
        out["nll_%s_nll" % case], out["nll_%s_gF" % case], out["nll_%s_gS" % case] = f32(nll.view(shape)), f32(F64.grad), f32(S64.grad)
    # ---- PoseMFShapeGaussianLoss ----
    for case in SC.LOSS_CASES:
        pred, target = SC.loss_inputs(case)
        target_dict, pred_dict, leaves = SC.make_dicts(pred, target, torch.float64)
        total = PoseMFShapeGaussianLoss(SC.loss_config(case), SC.IMG_WH)(target_dict, pred_dict)
        total.backward()
        out["loss_%s_total" % case] = np.float32(total.item())
        for name, leaf in zip(SC.GRAD_NAMES, leaves):
            if case == "b72" and name == "verts":
                continue
            out["loss_%s_g%s" % (case, name)] = f32(leaf.grad)
    if check:
        old = np.load(OUT)
        assert sorted(old.files) == sorted(out), "key sets differ"
        worst = 0.0
        for k in out:
            a, b = old[k].astype(np.float64), np.asarray(out[k], np.float64)
            d = np.where(np.isnan(a) & np.isnan(b), 0.0, np.abs(a - b))       # NaN where the reference gives NaN; elsewhere a NaN counts
            worst = max(worst, float(np.max(d, initial=0.0)) if not np.isnan(d).any() else float("inf"))
        print("max |delta| = %g over %d arrays" % (worst, len(out)))
        return
    np.savez_compressed(OUT, **{k: np.asarray(v) for k, v in out.items()})
    print("wrote", OUT, os.path.getsize(OUT), "bytes", {k: np.shape(v) for k, v in out.items()})


if __name__ == "__main__":
    main(check="--check" in sys.argv)
