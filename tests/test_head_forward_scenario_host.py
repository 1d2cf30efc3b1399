"""CPU: the head forward scenario (head_forward_scenario) can tell right from wrong.  The feature filter keeps enough rows on every
tree, the spread recipe yields improper matrices where the tree has depth, the sliced family members and the sliced float64
evaluation stay inside their bounds, and every mutant of the fp32 restatement breaks the bound on a named output."""
import pytest
import torch

import head_forward_scenario as FS
import head_grad_scenario as HS

B = 9
TREE_NAMES = ("smpl", "chain7", "star6", "mixed12")
# the joint levels' case of tests/test_gpu_head_forward.py: widths the module cannot produce
LEVELS_CASE = ("mixed12", "spread", 5, 2, (24, 16, 2, 6, 3, 40, 128))
TRUNK_WIDTHS = ((40, 24, 1, 6, 3, 20, 128), (512, 512, 10, 6, 3, 256, 128))


@pytest.mark.parametrize("recipe", ["default", "spread"])
@pytest.mark.parametrize("tree", TREE_NAMES)
def test_quarter_condition_and_improper_share(tree, recipe):
    c = FS.case(tree, recipe, B)
    print("%s %s: %d of %d candidate rows kept" % (tree, recipe, c["kept"], c["candidates"]))
    assert c["feats"].shape == (B, 512) and 4 * c["kept"] >= c["candidates"]
    out = FS.run(c, torch.float64)
    assert float(HS.min_gap(out["pose_S"]).min()) >= HS.MIN_GAP
    share = HS.improper_share(out)
    print("share of matrices with det U det V = -1: %.3f" % share)
    if recipe == "spread" and tree in FS.DEEP_TREES:
        assert share >= 0.05
    if recipe == "default":
        assert share == 0.0


def test_the_custom_width_cases_meet_the_quarter_condition():
    c = FS.case(*LEVELS_CASE)
    print("levels case: %d of %d kept, improper share %.3f" % (c["kept"], c["candidates"], HS.improper_share(FS.run(c, torch.float64))))
    assert 4 * c["kept"] >= c["candidates"]
    for w in TRUNK_WIDTHS:
        for b in (1, 9):
            c = FS.case("single", "default", b, w[2], w)
            assert 4 * c["kept"] >= c["candidates"] and c["feats"].shape == (b, w[0])


@pytest.mark.parametrize("recipe", ["default", "spread"])
@pytest.mark.parametrize("tree", TREE_NAMES)
def test_sliced_family_members_stay_inside_the_bound(tree, recipe):
    """Members b and c against the rule built from a alone, 4 max(e_a, 2^-23 max|y64|): a summation order other than torch's is
    inside the project's margin on every output (and so the family's bound is no wider than it has to be)."""
    c = FS.case(tree, recipe, B)
    pin = FS.run(c)["pose_U"]                                       # on the CPU the run under test is the fp32 restatement itself
    y64, fam = FS.reference(c, pin)
    worst = {}
    for m in ("b", "c"):
        for name in FS.ALL_OUTPUTS:
            worst[name] = max(worst.get(name, 0.0), FS._check_one("%s %s member %s" % (tree, recipe, m), name, fam[m][name], y64[name],
                                                                  [fam["a"][name]], "a"))
    print("%s %s sliced members in max(e_a, 2^-23 max|y64|): %s" % (tree, recipe, {k: round(v, 2) for k, v in worst.items()}))
    res = FS.check("%s %s restatement" % (tree, recipe), FS.run(c), c)          # the run under test against its own truth
    assert max(res.values()) <= 1.0 + 1e-12


@pytest.mark.parametrize("tree,recipe,b,num_betas", sorted(set([(t, r, B, 10) for t in TREE_NAMES for r in ("default", "spread")] + FS.DEVICE_CASES)))
def test_sliced_float64_evaluation_stays_inside_bound64(tree, recipe, b, num_betas):
    """Float64 sums in K slices against float64 sums in torch's order, both with the 40-digit SVD: on every tree and recipe at B = 9
    and on the cases the device test applies the float64 rule to."""
    c = FS.case(tree, recipe, b, num_betas)
    pin = FS.run(c)["pose_U"]
    sliced = FS.run(c, torch.float64, pin, FS.Ops(FS.TRUNK_SLICES, FS.JOINT_SLICES, exact_svd=True))
    res = FS.check("%s %s B=%d float64 sliced" % (tree, recipe, b), sliced, c, pin, rule64=True)
    print("%s %s B=%d float64 sliced worst in 2^-29 max(e_a, 2^-23 max|y64|): %.2f" % (tree, recipe, b, max(res.values())))


def _acts(mutant, tree, recipe):
    _, needs_depth, needs_improper, _ = FS.MUTANTS[mutant]
    if needs_depth and tree not in FS.DEEP_TREES:
        return False
    return not needs_improper or recipe == "spread"


@pytest.mark.parametrize("mutant", sorted(FS.MUTANTS))
def test_every_mutant_breaks_the_bound_on_its_named_outputs(mutant):
    """On every tree and recipe where the mutant can act, each output named for it leaves the bound (ratio > 4); where it cannot act
    (no ancestors, no improper matrix), the mutant run is the restatement and stays inside."""
    named = FS.MUTANTS[mutant][0]
    acted = 0
    for tree in TREE_NAMES:
        for recipe in ("default", "spread"):
            c = FS.case(tree, recipe, B)
            out = FS.mutant_run(c, mutant)
            r = FS.ratios(out, c, out["pose_U"], strict=False)
            print("%-44s %-8s %-8s %s" % (mutant, tree, recipe, "  ".join("%s %.3g" % (k, r[k]) for k in named)))
            if _acts(mutant, tree, recipe):
                acted += 1
                for name in named:
                    assert r[name] > 4.0, (mutant, tree, recipe, name, r[name])
            elif FS.MUTANTS[mutant][1] and tree not in FS.DEEP_TREES:
                assert max(r.values()) <= 4.0, (mutant, tree, recipe, r)
    assert acted >= 2


def test_linear_case_references_agree_and_the_chain_is_the_worst_order():
    for K, N, b, act, addend in [(1, 1, 1, 0, False), (17, 17, 9, 1, True), (113, 15, 1, 0, False), (1792, 29, 8, 2, True)]:
        lc = FS.linear_case(K, N, b, act, addend)
        FS.check_linear("linear_case K=%d member a" % K, lc["y_a"], lc)
        FS.check_linear("linear_case K=%d member d" % K, lc["y_d"], lc)
        if act:
            assert bool((lc["y64"] <= 0).any()) or K == 1                         # the activation cuts
        wrong = FS.activate(lc["y_a"] - lc["x"][:, -1:] * lc["wt"][-1:], 0) if act == 0 else None
        if wrong is not None and K > 1:
            with pytest.raises(AssertionError):
                FS.check_linear("last k dropped", wrong, lc)
