"""CPU: the float64 restatement of the person detector (tests/detector_scenario.py) checked against definitions it does not share code
with, and the parts of detection.MaskRCNNBoxDetector that need no GPU: its state-dict keys and the loading rules, the refusals."""
import math

import pytest
import torch
import torch.nn.functional as F

import detector_scenario as S
from hierarchicalprobabilistic3dhuman_amd import detection


# ---- the scenario's own stages --------------------------------------------------------------------------------------------------------
def test_nms_equals_the_brute_force_definition():
    g = torch.Generator().manual_seed(3)
    for n in (1, 2, 17, 120):
        xy = torch.rand(n, 2, generator=g, dtype=torch.float64) * 40
        wh = torch.rand(n, 2, generator=g, dtype=torch.float64) * 30
        boxes = torch.cat([xy, xy + wh], dim=1)
        boxes[::7, 2:] = boxes[::7, :2]                              # zero-area boxes
        if n > 2:
            boxes[2] = boxes[1]                                      # identical boxes
        scores = torch.rand(n, generator=g, dtype=torch.float64)
        for thresh in (0.3, 0.7):
            keep, margin = S.nms(boxes, scores, thresh)
            assert keep == S.nms_brute(boxes, scores, thresh)
            assert margin > 0
    cats = torch.tensor([0, 1, 0, 1, 2])
    boxes = torch.tensor([[0, 0, 10, 10], [0, 0, 10, 10], [1, 0, 10, 10], [20, 20, 30, 30], [0, 0, 10, 10]], dtype=torch.float64)
    scores = torch.tensor([0.9, 0.8, 0.7, 0.6, 0.5], dtype=torch.float64)
    keep, _ = S.nms_per_category(boxes, scores, cats, 0.5)
    assert keep == [0, 1, 3, 4]                                      # 2 falls to 0 (same category); 1 and 4 equal 0 but in other categories


def test_roi_align_of_a_linear_ramp_is_the_ramp_at_the_bin_centres():
    C = 3
    coef = torch.tensor([[0.5, 2.0, -1.0], [1.0, -0.25, 0.75], [-3.0, 0.0, 1.5]], dtype=torch.float64)      # a + b y + c x

    def ramp(h, w):
        ys, xs = torch.arange(h, dtype=torch.float64)[:, None], torch.arange(w, dtype=torch.float64)[None, :]
        return torch.stack([coef[c, 0] + coef[c, 1] * ys + coef[c, 2] * xs for c in range(C)])

    levels = [ramp(64, 64), ramp(32, 32), ramp(16, 16), ramp(8, 8)]
    boxes = torch.tensor([[20.0, 24.0, 70.0, 80.0], [8.0, 40.0, 200.0, 180.0], [16.5, 33.25, 40.0, 90.0]], dtype=torch.float64)
    lv, margin = S.level_of(boxes)
    assert lv.tolist() == [0, 1, 0] and margin > 1e-3
    out = S.roi_align(levels, boxes)
    for r in range(boxes.shape[0]):
        scale = 1.0 / (4 << int(lv[r]))
        x1, y1, x2, y2 = (boxes[r] * scale).tolist()
        bw, bh = max(x2 - x1, 1.0) / 7, max(y2 - y1, 1.0) / 7
        for ph in range(7):
            for pw in range(7):
                yc, xc = y1 + (ph + 0.5) * bh, x1 + (pw + 0.5) * bw
                want = coef[:, 0] + coef[:, 1] * yc + coef[:, 2] * xc
                assert torch.allclose(out[r, :, ph, pw], want, rtol=0, atol=1e-11)


def test_anchors_of_a_2x3_map_written_out():
    base = S.base_anchors(32)
    assert base.tolist() == [[-23.0, -11.0, 23.0, 11.0], [-16.0, -16.0, 16.0, 16.0], [-11.0, -23.0, 11.0, 23.0]]
    assert torch.equal(detection.base_anchors(32).double(), base)
    for size in S.LEVEL_SIZES:
        assert torch.equal(detection.base_anchors(size).double(), S.base_anchors(size))
    a = S.anchors(32, 2, 3, 8, 4)
    assert a.shape == (18, 4)
    want = []
    for y in (0, 8):
        for x in (0, 4, 8):
            for b in base.tolist():
                want.append([b[0] + x, b[1] + y, b[2] + x, b[3] + y])
    assert a.tolist() == want
    assert a[3 * 4 + 1].tolist() == [4.0 - 16, 8.0 - 16, 4.0 + 16, 8.0 + 16]          # (y 1, x 1, ratio 1)


@pytest.mark.parametrize("hw,out", [((50, 37), (86, 64)), ((48, 80), (57, 96)), ((20, 20), (64, 64))])
def test_resize_equals_interpolate(hw, out):
    cfg = S.config(**S.TINY)
    assert S.resized_size(hw[0], hw[1], cfg) == out
    assert detection.resized_size(hw[0], hw[1], cfg["min_size"], cfg["max_size"]) == out
    g = torch.Generator().manual_seed(hw[0])
    x = torch.rand(3, hw[0], hw[1], generator=g, dtype=torch.float64)
    want = F.interpolate(x[None], size=out, mode="bilinear", align_corners=False)[0]
    assert torch.allclose(S.resize_bilinear(x, out[0], out[1]), want, rtol=0, atol=1e-13)


def test_transform_places_images_top_left_in_a_frame_of_multiples_of_32():
    cfg = S.config(**S.TINY)
    ims, _ = S.scenario_inputs(0)
    batch, sizes = S.transform([im.double() for im in ims], cfg)
    assert sizes == [(86, 64), (57, 96)] and tuple(batch.shape) == (2, 3, 96, 96)
    assert float(batch[0, :, 86:].abs().max()) == 0 and float(batch[0, :, :, 64:].abs().max()) == 0 and float(batch[1, :, 57:].abs().max()) == 0


def test_decode_clamps_and_clips():
    boxes = torch.tensor([[10.0, 10.0, 30.0, 50.0]], dtype=torch.float64)
    out = S.decode(torch.tensor([[0.5, -0.25, 100.0, math.log(2.0)]], dtype=torch.float64), boxes, (1.0, 1.0, 1.0, 1.0))
    w = 20 * 1000.0 / 16.0
    assert torch.allclose(out, torch.tensor([[30 - w / 2, 20 - 40.0, 30 + w / 2, 20 + 40.0]], dtype=torch.float64))
    assert S.clip(out, (48, 64)).tolist() == [[0.0, 0.0, 64.0, 48.0]]


# ---- the module ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def detector():
    return detection.maskrcnn_resnet50_fpn()


def test_state_dict_keys_and_shapes_are_the_released_file_s(detector):
    want = S.expected_keys(91)
    sd = detector.state_dict()
    assert set(sd) == set(want)
    for k, shape in want.items():
        assert tuple(sd[k].shape) == shape, k
    assert not any("num_batches_tracked" in k for k in sd)
    assert "masks" not in sd and any(k.startswith("roi_heads.mask_predictor.") for k in sd)       # held, never run
    other = {k: torch.full_like(v, 0.5) for k, v in sd.items()}
    res = detector.load_state_dict(other, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert float(detector.roi_heads.box_head.fc6.weight[3, 5]) == 0.5 and float(detector.backbone.body.layer3[2].bn2.running_var[1]) == 0.5


def test_later_spelling_and_num_batches_tracked_load_strictly(detector):
    sd = {}
    for k, v in detector.state_dict().items():
        parts = k.split(".")
        if k.startswith("backbone.fpn."):
            parts.insert(4, "0")
        elif k.startswith("rpn.head.conv."):
            parts[3:3] = ["0", "0"]
        sd[".".join(parts)] = torch.full_like(v, 0.25)
    assert "backbone.fpn.inner_blocks.2.0.weight" in sd and "rpn.head.conv.0.0.bias" in sd and "rpn.head.conv.bias" not in sd
    for k in list(sd):
        if k.endswith("running_var"):
            sd[k[:-len("running_var")] + "num_batches_tracked"] = torch.tensor(7)
    res = detector.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert float(detector.backbone.fpn.layer_blocks[1].weight[0, 0, 0, 0]) == 0.25 and float(detector.rpn.head.conv.bias[0]) == 0.25
    with pytest.raises(RuntimeError):
        detector.load_state_dict(dict(sd, **{"roi_heads.box_head.fc8.weight": torch.zeros(1)}), strict=True)


def test_refusals_and_keywords(detector):
    with pytest.raises(NotImplementedError):
        detection.maskrcnn_resnet50_fpn(pretrained=True)
    with pytest.raises(NotImplementedError):
        detector.train()
    assert detector.eval() is detector and not detector.training and not detector.backbone.body.training
    with pytest.raises(RuntimeError, match="requires grad"):
        detector([torch.zeros(3, 8, 8, requires_grad=True)])
    from hierarchicalprobabilistic3dhuman_amd import _capi
    with pytest.raises(_capi.HpsError):
        detector([torch.zeros(3, 8, 8)])                            # no CPU path
    d = detection.maskrcnn_resnet50_fpn(**S.TINY)
    assert (d.num_classes, d.min_size, d.max_size, d.rpn_pre_nms_top_n, d.rpn_post_nms_top_n, d.box_detections_per_img) == (3, 64, 96, 50, 30, 10)
    assert (detector.rpn_nms_thresh, detector.box_score_thresh, detector.box_nms_thresh, detector.frozen_bn_eps) == (0.7, 0.05, 0.5, 0.0)
    assert detector.backbone.body.bn1.eps == 0.0 and detection.maskrcnn_resnet50_fpn(frozen_bn_eps=1e-5, num_classes=2).backbone.body.bn1.eps == 1e-5
    assert tuple(d.roi_heads.box_predictor.bbox_pred.weight.shape) == (12, 1024)
    with pytest.raises(ValueError):
        detection.maskrcnn_resnet50_fpn(rpn_pre_nms_top_n_test=5000)


def test_committed_seed_meets_the_end_to_end_preconditions():
    """The seed tests/test_gpu_detector.py uses: the oracle alone returns at least 3 detections per image and every margin of the chain
    is at least 8 bounds wide."""
    ims, sd = S.scenario_inputs(S.SEED)
    r, _, bounds, problems = S.chain_preconditions(ims, sd, S.config(**S.TINY))
    assert not problems, problems
    assert all(len(x["scores"]) >= 3 for x in r)
