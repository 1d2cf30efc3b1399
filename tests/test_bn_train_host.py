"""CPU: the training-mode BatchNorm reference of bn_train_scenario is torch's own training step (real nn.BatchNorm2d modules in
training mode: features, running buffers, counters), its float64 gradients agree with central differences, the fp32 restatement's
own error on the gradient cases stays under the cap, and the switch's host-side contract (default, survival, refusals before any
launch) holds without a device."""
import copy

import pytest
import torch
import torch.nn.functional as F

import bn_train_scenario as BS
import encoder_grad_scenario as ES


def module_forward(enc, x):
    """models/resnet.py:202-217 on the parameter-holding children themselves (their own nn.Module forwards)."""
    y = F.max_pool2d(F.relu(enc.bn1(enc.conv1(x))), 3, 2, 1)
    for layer in (enc.layer1, enc.layer2, enc.layer3, enc.layer4):
        for blk in layer:
            identity = y if blk.downsample is None else blk.downsample(y)
            out = F.relu(blk.bn1(blk.conv1(y)))
            y = F.relu(blk.bn2(blk.conv2(out)) + identity)
    return y.mean(dim=(2, 3))


def frozen(enc):
    """enc.train() with the stem and layer1 in eval: the mixed mode."""
    enc.train()
    enc.bn1.eval()
    enc.layer1.eval()
    return enc


def mixed_train(sd):
    return [k for k in BS.layer_keys(sd) if k != "stem" and not k.startswith("layer1.")]


@pytest.mark.parametrize("mixed", [False, True])
def test_restatement_is_torchs_training_step(mixed):
    """Two steps, momentum 0.5 on one layer: features, every running buffer and every counter against nn.BatchNorm2d in training mode."""
    enc = ES.make_encoder(18)
    enc.layer2[0].bn1.momentum = 0.5
    sd = {k: v.clone() for k, v in enc.state_dict().items()}
    train = mixed_train(sd) if mixed else None
    frozen(enc) if mixed else enc.train()
    x, _ = ES.case("sq64")
    # all layers training: the very operations, in the same order.  Mixed: the modules' eval layers run torch's (z - mean) / sqrt(var +
    # eps) * w + b, the restatement (as the device) the folded z * scale + shift -- another fp32 rounding per eval layer, amplified by
    # the normalisations behind it: the project's feature tolerance against the reference (1e-4, tests/test_gpu_net.py)
    tol = 1e-4 if mixed else 1e-6
    with torch.no_grad():
        for step in range(2):
            want = module_forward(enc, x + step)
            got, _, stats = BS.forward(sd, x + step, None, train, {"layer2.0.c1": 0.5}, update=True)
            assert float((got - want).abs().max()) <= tol * float(want.abs().max())
    assert len(stats) == (20 if not mixed else 15)
    real = enc.state_dict()
    for k, v in real.items():
        if "running" in k:
            assert float((sd[k] - v).abs().max()) <= tol * float(v.abs().max()), k
        elif k.endswith("num_batches_tracked"):
            assert int(sd[k]) == int(v) == (0 if mixed and (k.startswith("layer1.") or k == "bn1.num_batches_tracked") else 2), k
    if mixed:
        assert torch.equal(real["bn1.running_mean"], ES.state(18)["bn1.running_mean"])


def test_float64_gradients_agree_with_central_differences():
    """Pinned masks and winners make the function smooth: directional derivatives along random directions over all leaves."""
    sd32, (x, cot) = ES.state(5), ES.case("c5")
    with torch.no_grad():
        pins = ES.pins_from_maps(BS.forward(sd32, x)[1])
    g64, _ = BS.vjp(sd32, x, pins, cot, torch.float64)
    names = ES.param_names(sd32)
    gen = torch.Generator().manual_seed(5)

    def value(step, direction):
        sd = BS.cast(sd32, torch.float64)
        for k in names:
            sd[k] = sd[k] + step * direction[k]
        with torch.no_grad():
            feats, _, _ = BS.forward(sd, x.double() + step * direction["input"], pins)
        return float((cot.double() * feats).sum())

    for trial in range(3):
        direction = {k: torch.randn(g64[k].shape, generator=gen, dtype=torch.float64) for k in g64}
        if trial == 1:                                           # the BatchNorm affine parameters alone
            direction = {k: (v if ("bn" in k or "downsample.1" in k) else torch.zeros_like(v)) for k, v in direction.items()}
        h = 1e-6
        numeric = (value(h, direction) - value(-h, direction)) / (2 * h)
        analytic = float(sum((g64[k] * direction[k]).sum() for k in g64))
        print("direction %d: numeric %.9e analytic %.9e" % (trial, numeric, analytic))
        assert abs(numeric - analytic) <= 1e-6 * abs(analytic)


@pytest.mark.parametrize("name", BS.GRADIENT_CASES)
def test_fp32_restatement_stays_under_the_cap(name):
    cin, _ = ES.CASES[name]
    x, cot = ES.case(name)
    with torch.no_grad():
        pins = ES.pins_from_maps(BS.forward(ES.state(cin), x)[1])
    (g64, _), (g32, _) = BS.reference((name, "self"), ES.state(cin), x, pins, cot)
    err = BS.own_error(g64, g32)
    print("%s: fp32 restatement's worst-tensor error = %.1f x 2^-23 max|g|" % (name, err))
    assert err <= BS.CAP


def test_switch_defaults_off_and_survives_copies_and_loads(net_cpu):
    enc = ES.make_encoder(18)
    assert enc._bn_training is False
    enc.train()
    with pytest.raises(RuntimeError):                            # off: refused, on a CPU tensor too (before any device check)
        enc(torch.zeros(2, 18, 32, 32))
    enc.set_batchnorm_training(True)
    assert enc._bn_training is True
    assert copy.deepcopy(enc)._bn_training is True
    enc.load_state_dict(ES.state(18))
    assert enc.float()._bn_training is True and enc._bn_training is True
    enc.set_batchnorm_training(False)
    assert enc._bn_training is False
    net = copy.deepcopy(net_cpu[0])
    net.set_batchnorm_training(True)
    assert net.image_encoder._bn_training is True


def test_refusals_come_before_any_device_work():
    """torch's wording for one value per channel; momentum=None; track_running_stats=False; the inference pipeline's arguments --
    all raised for CPU tensors, i.e. before anything looks for a device, and no buffer or counter moves."""
    from hierarchicalprobabilistic3dhuman_amd import _capi
    from hierarchicalprobabilistic3dhuman_amd.resnet import FilledStemFrames
    enc = ES.make_encoder(18)
    enc.set_batchnorm_training(True)
    enc.train()
    before = {k: v.clone() for k, v in enc.state_dict().items()}
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        enc(torch.zeros(1, 18, 32, 32))                          # layer4: 1 x 1 maps, batch 1
    enc.layer3[1].bn2.momentum = None
    with pytest.raises(NotImplementedError):
        enc(torch.zeros(2, 18, 64, 64))
    enc.layer3[1].bn2.momentum = 0.1
    enc.layer3[1].bn2.track_running_stats = False
    with pytest.raises(NotImplementedError):
        enc(torch.zeros(2, 18, 64, 64))
    enc.layer3[1].bn2.track_running_stats = True
    with pytest.raises(RuntimeError, match="inference pipeline"):
        enc(torch.zeros(2, 18, 64, 64), _gate=lambda: None)
    with pytest.raises(RuntimeError, match="inference pipeline"):
        enc(FilledStemFrames(None, (2, 18, 64, 64), None))
    with pytest.raises(_capi.HpsError):                          # nothing wrong but the device: the product has no CPU path
        enc(torch.zeros(2, 18, 64, 64))
    with pytest.raises(RuntimeError):
        enc.activations(torch.zeros(2, 18, 64, 64))
    assert all(torch.equal(v, before[k]) for k, v in enc.state_dict().items())
    # every BatchNorm in eval: the switch changes nothing, the eval path looks for its device
    enc.eval()
    enc.train(False)
    assert enc._train_flags() is None
    enc.layer4[1].bn2.train()                                    # one layer decides for itself
    flags = enc._train_flags()
    assert flags["layer4.1.c2"] and sum(flags.values()) == 1
