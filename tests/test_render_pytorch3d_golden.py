"""The restatement of tests/render_scenario.py against pytorch3d's own output (tests/golden/render_pytorch3d.npz, written by
tests/golden/make_render_golden.py where pytorch3d is installed).  The fixture has never been produced: this test skips until it is,
and the restatement's rules stay unchecked against pytorch3d until then."""
import os

import numpy as np
import pytest

import render_scenario as S

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "render_pytorch3d.npz")


def test_float32_restatement_matches_pytorch3d():
    if not os.path.exists(PATH):
        pytest.skip("pytorch3d fixture absent: run tests/golden/make_render_golden.py where pytorch3d is installed")
    z = np.load(PATH)
    for name in sorted({k.split("/")[0] for k in z.files}):
        scene, r32, r64 = S.reference(name)
        got = {k: z["%s/%s" % (name, k)] for k in ("pix_to_face", "zbuf", "bary", "iuv", "rgb")}
        dev = S.deviations(scene, r32, r64)
        agree, differing, covered, w_min, excess = S.agreement(scene, got, r64)
        assert differing <= S.NEAR_TIE_CAP * covered, name
        if differing:
            assert w_min > -S.FACTOR * dev["bary"] and excess < S.FACTOR * dev["zbuf"], name
        on = agree & (r64["pix_to_face"] >= 0)
        for k in ("zbuf", "bary", "iuv", "rgb"):
            assert np.abs(got[k].astype(np.float64) - r64[k])[on].max() <= S.FACTOR * dev[k], (name, k)
