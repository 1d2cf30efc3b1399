"""CPU: the mask branch's restatement (tests/detector_mask_scenario.py) checked against definitions it does not share code with, the
parts of the device mask branch that need no GPU (struct sizes, argument validation before any launch, the refusals, the default
route's keys), and the preconditions of the committed scenario that tests/test_gpu_detector_mask.py relies on."""
import ctypes

import pytest
import torch

import detector_mask_scenario as M
import detector_scenario as S
from hierarchicalprobabilistic3dhuman_amd import _capi, detection

CFG = S.config(**S.TINY)


def test_explicit_paste_equals_the_interpolate_one():
    g = torch.Generator().manual_seed(4)
    for H, W in M.PASTE_SIZES:
        names, boxes = M.paste_boxes(H, W)
        probs = 0.05 + 0.9 * torch.rand(len(names), M.SIZE, M.SIZE, generator=g, dtype=torch.float64)
        ib = M.expand_and_truncate(boxes)
        a, b = M.paste(probs, ib, H, W), M.paste_explicit(probs, ib, H, W)
        assert float((a - b).abs().max()) <= 1e-12
        if (H, W) == (23, 31):
            cut = {n: (int(ib[k, 0]) < 0, int(ib[k, 1]) < 0, int(ib[k, 2]) + 1 > W, int(ib[k, 3]) + 1 > H) for k, n in enumerate(names)}
            assert cut["inside"] == (False,) * 4 and cut["left"] == (True, False, False, False) and cut["top"] == (False, True, False, False)
            assert cut["right"] == (False, False, True, False) and cut["bottom"] == (False, False, False, True) and cut["larger"] == (True,) * 4
            filled = {n: int((a[k] != 0).sum()) for k, n in enumerate(names)}
            assert filled["outside"] == 0 and filled["zero"] == 1 and filled["larger"] == H * W and 0 < filled["inside"] < H * W
        # the expanded corner in (-1, 0) becomes 0, not -1
        k = names.index("truncation")
        b32 = boxes[k]
        corner = float((b32[2] + b32[0]) * 0.5 - (b32[2] - b32[0]) * 0.5 * M.SCALE)
        assert -1.0 < corner < 0.0 and int(ib[k, 0]) == 0 and int(ib[k, 1]) == 0


def test_expand_and_truncate_written_out():
    ib = M.expand_and_truncate(torch.tensor([[2.0, 4.0, 16.0, 32.0], [-0.5, 1.0, 0.5, 1.0]]))
    # centre (9, 18), half sizes 7 * 30 / 28 = 7.5 and 15; centre (0, 1), half sizes 0.5357 and 0
    assert ib.tolist() == [[1, 3, 16, 33], [0, 1, 0, 1]] and ib.dtype == torch.int64


def test_transposed_convolution_is_four_1x1_products():
    sd = S.cast(S.make_weights(S.SEED, 3), torch.float64)
    x = torch.randn(3, 256, 5, 4, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    a, b = M.upsample(x, sd), M.upsample_as_products(x, sd)
    assert a.shape == (3, 256, 10, 8) and float((a - b).abs().max()) <= 1e-12 * float(a.abs().max())
    # and the kernel-side weight form holds W[2 s + (lane >> 5)][32 t + (lane & 31)][dy][dx]
    W = sd["roi_heads.mask_predictor.conv5_mask.weight"].float()
    k = detection.mask_weights(W)
    assert tuple(k.shape) == (4, 128, 64, 8)
    for tap, s, lane, t in ((0, 0, 0, 0), (1, 5, 37, 3), (2, 127, 63, 7), (3, 64, 31, 6)):
        assert float(k[tap, s, lane, t]) == float(W[2 * s + (lane >> 5), 32 * t + (lane & 31), tap >> 1, tap & 1])


def test_structs_match_the_library():
    lib = _capi.load()
    assert lib.hps_sizeof_det_mask_predict_args() == ctypes.sizeof(_capi.DetMaskPredictArgs)
    assert lib.hps_sizeof_det_paste_masks_args() == ctypes.sizeof(_capi.DetPasteMasksArgs)
    assert lib.hps_sizeof_det_roi_align_args() == ctypes.sizeof(_capi.DetRoiAlignArgs)
    for name in ("hps_det_roi_align_halo", "hps_det_mask_predict", "hps_det_paste_masks", "hps_sizeof_det_mask_predict_args",
                 "hps_sizeof_det_paste_masks_args"):
        assert name in _capi.EXPORTED_SYMBOLS
    assert lib.hps_version() == 502


def test_bad_arguments_are_refused_before_any_launch():
    lib = _capi.load()
    err = lambda: lib.hps_last_error()
    assert lib.hps_det_mask_predict(None, None) == -1 and b"null pointer" in err()
    assert lib.hps_det_paste_masks(None, None) == -1 and b"null pointer" in err()
    assert lib.hps_det_roi_align_halo(None, 1, None) == -1 and b"null pointer" in err()
    p = 4096                                                          # an aligned non-null address; nothing is launched
    good = dict(struct_bytes=ctypes.sizeof(_capi.DetMaskPredictArgs), K=2, NC=3, x=p, wd=p, bd=p, wl=p, bl=p, labels=p, scores=None, probs=p,
                logits=None)
    for kw, msg in ((dict(struct_bytes=8), b"struct_bytes"), (dict(K=-1), b"detections"), (dict(K=70000), b"detections"), (dict(NC=1), b"NC"),
                    (dict(x=None), b"null pointer"), (dict(wd=None), b"null pointer"), (dict(labels=None), b"null pointer"),
                    (dict(probs=None), b"null pointer"), (dict(x=p + 4), b"unaligned"), (dict(labels=p + 4), b"unaligned")):
        a = _capi.DetMaskPredictArgs(**dict(good, **kw))
        assert lib.hps_det_mask_predict(ctypes.byref(a), None) == -1 and msg in err(), (kw, err())
    assert lib.hps_det_mask_predict(ctypes.byref(_capi.DetMaskPredictArgs(**dict(good, K=0, x=None))), None) == 0
    good = dict(struct_bytes=ctypes.sizeof(_capi.DetPasteMasksArgs), n=2, H=8, W=8, binary=0, threshold=0.0, probs=p, boxes=p, out=p)
    for kw, msg in ((dict(struct_bytes=4), b"struct_bytes"), (dict(n=-1), b"image size"), (dict(H=0), b"image size"), (dict(W=40000), b"image size"),
                    (dict(binary=2), b"binary"), (dict(binary=1, threshold=0.0), b"threshold"), (dict(binary=1, threshold=1.0), b"threshold"),
                    (dict(binary=1, threshold=float("nan")), b"threshold"), (dict(probs=None), b"null pointer"), (dict(out=None), b"null pointer"),
                    (dict(boxes=p + 4), b"unaligned"), (dict(out=p + 8), b"unaligned")):
        a = _capi.DetPasteMasksArgs(**dict(good, **kw))
        assert lib.hps_det_paste_masks(ctypes.byref(a), None) == -1 and msg in err(), (kw, err())
    assert lib.hps_det_paste_masks(ctypes.byref(_capi.DetPasteMasksArgs(**dict(good, n=0, out=None))), None) == 0
    a = _capi.DetRoiAlignArgs(struct_bytes=ctypes.sizeof(_capi.DetRoiAlignArgs), B=1, R=1, C=4, bins=14, n_levels=1, boxes=p, scores=p, y=p)
    a.level[0].x, a.level[0].h, a.level[0].w, a.level[0].pad, a.level[0].scale = p, 4, 4, 1, 0.25
    for halo in (-1, 9):
        assert lib.hps_det_roi_align_halo(ctypes.byref(a), halo, None) == -1 and b"halo" in err()


def test_refusals():
    probs, boxes = torch.zeros(2, 28, 28), torch.zeros(2, 4)
    with pytest.raises(_capi.HpsError):
        detection.paste_masks(probs, boxes, (8, 8))                   # no CPU path
    for t in (0.0, 1.0, -0.5, 1.5):
        with pytest.raises(ValueError):
            detection.paste_masks(probs, boxes, (8, 8), threshold=t)
    det = detection.maskrcnn_resnet50_fpn(**S.TINY)
    with pytest.raises(ValueError):
        det([torch.zeros(3, 8, 8)], masks=True, mask_threshold=1.0)
    with pytest.raises(_capi.HpsError):
        det([torch.zeros(3, 8, 8)], masks=True)
    with pytest.raises(_capi.HpsError):
        detection.multiscale_roi_align([(torch.zeros(1, 6, 6, 4), 1, 0.25)], torch.zeros(1, 1, 4), bins=14, halo=1)
    with pytest.raises(_capi.HpsError):
        detection.mask_predict(torch.zeros(1, 16, 16, 256), torch.zeros(4, 128, 64, 8), torch.zeros(256), torch.zeros(3, 256), torch.zeros(3),
                               torch.zeros(1, dtype=torch.int64))


def test_default_forward_still_has_three_keys(monkeypatch):
    det = detection.maskrcnn_resnet50_fpn(**S.TINY)
    calls = []

    def padded(images, frame=None, masks=False):
        calls.append(masks)
        out = (torch.zeros(1, 10, 4), torch.zeros(1, 10, dtype=torch.int64), torch.zeros(1, 10), torch.tensor([2], dtype=torch.int32))
        return out + (torch.zeros(1, 10, 28, 28),) if masks else out

    monkeypatch.setattr(det, "detect_padded", padded)
    out = det([torch.zeros(3, 8, 8)])
    assert calls == [False] and len(out) == 1 and set(out[0]) == {"boxes", "labels", "scores"} and out[0]["boxes"].shape == (2, 4)
    import inspect
    for fn in (detection.MaskRCNNBoxDetector.forward, detection.MaskRCNNBoxDetector.detect_padded):
        assert inspect.signature(fn).parameters["masks"].default is False
    assert inspect.signature(detection.multiscale_roi_align).parameters["halo"].default == 0


@pytest.fixture(scope="module")
def chains():
    ims, sd = S.scenario_inputs(S.SEED)
    c64 = M.mask_chain([im.double() for im in ims], S.cast(sd, torch.float64), CFG)
    c32 = M.mask_chain(ims, sd, CFG)
    return ims, c64, c32


def test_committed_seed_meets_the_mask_tests_preconditions(chains):
    """What tests/test_gpu_detector_mask.py relies on, asserted as conditions: it fails, never skips, when they stop holding."""
    ims, c64, c32 = chains
    for b, (a, c) in enumerate(zip(c64, c32)):
        H, W = ims[b].shape[1:]
        n = a["labels"].numel()
        assert n >= 3, (b, n)
        assert set(a["labels"].tolist()) == {1, 2}, "both labels present"
        positive = float((a["pre"] > 0).double().mean())
        assert 0.25 <= positive <= 0.75, positive
        above = float((a["probs"] > 0.5).double().mean())
        assert 0.0 < above < 1.0 and float(a["logits"].min()) < 0 < float(a["logits"].max()), "both signs among the selected logits"
        cut = sum(M.cut_by_border(a["iboxes"][k], H, W) for k in range(n))
        assert cut >= 1, "a paste box cut by an image border"
        assert torch.equal(a["iboxes"], c["iboxes"]) and a["labels"].tolist() == c["labels"].tolist(), "the float32 chain's integer boxes"
        lv, _ = S.level_of(a["rois"])
        print("image %d: %d detections, labels %s, pre-activations positive %.3f, probabilities above 0.5 %.3f, %d boxes cut, levels %s"
              % (b, n, sorted(set(a["labels"].tolist())), positive, above, cut, sorted(set(lv.tolist()))))
        assert a["masks"].shape == (n, H, W) and float(a["masks"].min()) >= 0.0 and float(a["masks"].max()) <= 1.0
        assert float((M.paste_explicit(a["probs"], a["iboxes"], H, W) - a["masks"]).abs().max()) <= 1e-12
