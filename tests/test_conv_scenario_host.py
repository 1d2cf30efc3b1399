"""The convolution tests' references and accuracy rule on their own (tests/conv_scenario.py; no device): every reference of every case
of tests/test_gpu_conv_shapes.py stays inside the bound, the Winograd emulation is the same function as the convolution, and the rule
has teeth -- one dropped product, one wrongly padded border pixel, one image's map with rows and columns exchanged and one overwritten
halo element are each caught."""
import pytest
import torch
import torch.nn.functional as F

import conv_scenario as S

ALL_CASES = [S.wino_case(c) for c in S.WINO_CASES] + [S.direct_case(c) for c in S.DIRECT_CASES] + \
            [c for cfg in S.DOWN_CASES for c in S.down_cases(cfg)]
# K = 144, 576, 4608; all on non-square maps
TEETH = [(1, 16, 32, 16, 64, 3, 1, 1, 0), (2, 32, 16, 64, 64, 3, 1, 1, 1), (1, 16, 48, 512, 512, 3, 1, 1, 6)]


@pytest.mark.parametrize("c", ALL_CASES, ids=lambda c: "-".join(map(str, c["key"])))
def test_references_stay_inside_the_bound(c):
    for mode in S.MODES:
        r = S.reference(c, mode)
        assert r["scale"] > 0 and r["y64"].dtype == torch.float64 and r["y_cpu32"].dtype == torch.float32
        assert r["idx"].numel() <= S.SAMPLE
        S.check("cpu32", r["y_cpu32"], c, mode)
        S.check("seq32", r["y_seq32"], c, mode, at=r["idx"])
        if c["wino"]:
            S.check("wino32", r["y_wino32"], c, mode, wino=True)
            assert S.bound(c, mode, wino=True) >= S.bound(c, mode)
        # the sample holds the corners and the borders of the first and the last channel
        i, j = (r["idx"] // c["Wo"]) % c["Ho"], r["idx"] % c["Wo"]
        ch = (r["idx"] // (c["Wo"] * c["Ho"])) % c["Cout"]
        for want_ch in (0, c["Cout"] - 1):
            m = ch == want_ch
            for ci in (0, c["Ho"] - 1):
                for cj in (0, c["Wo"] - 1):
                    assert bool((m & (i == ci) & (j == cj)).any())


def test_the_sequential_chain_is_the_convolution():
    """On a case small enough to be covered whole: the fp32 chain is within K roundings of y64 at every position, and it is another
    order than torch's, not a copy of it."""
    c = S.case(2, 9, 14, 32, 64, 3, 2, 1, 1)
    r = S.reference(c, "lin")
    assert r["idx"].numel() == 2 * 64 * 5 * 7                                    # small case: every position
    seq = r["y_seq32"].reshape(r["y64"].shape)
    assert float((seq.double() - r["y64"]).abs().max()) <= c["K"] * S.EPS32 * r["scale"]
    assert not torch.equal(seq, r["y_cpu32"])


@pytest.mark.parametrize("cfg", [(1, 16, 32, 16, 64), (2, 32, 16, 64, 64), (1, 16, 48, 512, 512), (5, 8, 8, 24, 128)])
def test_winograd_emulation_is_the_same_function(cfg):
    B, H, W, Cin, Cout = cfg
    c = S.case(B, H, W, Cin, Cout, 3, 1, 1, 1)
    y64 = S.reference(c, "lin")["y64"]
    w64 = S.wino_lin(c, torch.float64)
    assert float((w64 - y64).abs().max()) <= 1e-12 * float(y64.abs().max())
    assert S.wino_lin(c).dtype == torch.float32


def _lin_defects(c):
    """name -> a copy of y_cpu32 ("lin") with one defect."""
    r = S.reference(c, "lin")
    y, x, w = r["y_cpu32"], c["x"], c["conv"].weight
    scale, _ = S.fold_bn(c["bn"])
    out = {}
    # one output pixel with a single product x * w missing: the product of median magnitude of that pixel's K
    b, co, i, j = c["B"] - 1, c["Cout"] // 2, c["Ho"] // 2, c["Wo"] - 2
    win = F.pad(x, (1, 1, 1, 1))[b, :, i:i + 3, j:j + 3]
    prod = (win * w[co]).reshape(-1)
    drop = prod[prod.abs().argsort()[prod.numel() // 2]]
    d = y.clone()
    d[b, co, i, j] = y[b, co, i, j] - scale[co] * drop
    out["one product dropped"] = d
    # one border pixel as if the padding repeated the neighbouring pixel
    with torch.no_grad():
        rep = c["bn"](F.conv2d(F.pad(x, (1, 1, 1, 1), mode="replicate"), w))
    d = y.clone()
    d[0, :, c["Ho"] - 1, c["Wo"] // 2] = rep[0, :, c["Ho"] - 1, c["Wo"] // 2]
    out["replicated padding at one border pixel"] = d
    # one image's map written with rows and columns exchanged (a pitch of W taken for H)
    assert c["Ho"] != c["Wo"]
    d = y.clone()
    d[b] = y[b].transpose(1, 2).reshape(y[b].shape)
    out["rows and columns exchanged"] = d
    return out


@pytest.mark.parametrize("key", TEETH, ids=lambda k: "K%d" % (9 * k[3]))
def test_the_rule_catches_injected_defects(key):
    c = S.case(*key)
    assert c["K"] in (144, 576, 4608) and c["wino"]
    r = S.reference(c, "lin")
    S.check("intact", r["y_cpu32"], c, "lin")
    for name, bad in _lin_defects(c).items():
        for wino in (False, True):                           # the wider family of a Winograd launch catches them too
            with pytest.raises(AssertionError):
                S.check(name, bad, c, "lin", wino=wino)
    # the same through the residual and the ReLU, at a pixel the ReLU leaves alone
    rr = S.reference(c, "res_relu")
    pos = (rr["y_cpu32"] > 1.0).nonzero()[0]
    bad = rr["y_cpu32"].clone()
    bad[tuple(pos)] += _lin_defects(c)["one product dropped"].sub(r["y_cpu32"]).abs().max()
    with pytest.raises(AssertionError):
        S.check("one product dropped, res_relu", bad, c, "res_relu", wino=True)
    # a halo element set to 0 instead of the fill value, on each of the four sides
    fr = S.frame(S.nhwc(r["y_cpu32"]), 1, fill=7.0)
    S.assert_halo_untouched(fr, 1, 7.0)
    S.assert_halo_untouched(S.nhwc(r["y_cpu32"]), 0, 7.0)
    Hf, Wf = fr.shape[1], fr.shape[2]
    for side, (i, j) in {"top": (0, Wf // 2), "bottom": (Hf - 1, 1), "left": (Hf // 2, 0), "right": (Hf - 2, Wf - 1)}.items():
        bad = fr.clone()
        bad[c["B"] - 1, i, j, 3] = 0.0
        with pytest.raises(AssertionError, match=side):
            S.assert_halo_untouched(bad, 1, 7.0)
    two = S.frame(S.nhwc(r["y_cpu32"]), 2, fill=7.0)
    S.assert_halo_untouched(two, 2, 7.0)
    two[0, 1, 5, 0] = 0.0                                    # the inner ring of a two-pixel halo
    with pytest.raises(AssertionError):
        S.assert_halo_untouched(two, 2, 7.0)
