"""CPU: the float64 restatement of the Adam update (optim_scenario.adam_update) against torch.optim.Adam on float64 parameters, and the
restatements of every hps_refresh_op kind (optim_scenario.run_refresh_ops) run over the REAL refresh lists of a CPU net against a
fresh ``prepare()`` -- the lists' extents, strides and offsets are checked here, before any device run."""
import copy
import ctypes

import pytest
import torch

import encoder_grad_scenario as ES
import head_grad_scenario as HS
import optim_scenario as OS
from hierarchicalprobabilistic3dhuman_amd import _capi
from hierarchicalprobabilistic3dhuman_amd.resnet import _ConvBN, _stem_winograd_filters


def chain_net_cpu():
    """tests/test_gpu_encoder_backward.chain_net before its .to(device): the seeded weights of the device refresh tests."""
    net = HS.make_net("spread")
    ES.randomize_bn(net.image_encoder)
    return net


@pytest.mark.parametrize("weight_decay,decoupled", [(0.0, False), (0.01, False), (0.01, True)])
def test_restatement_matches_torch_adam_in_float64(weight_decay, decoupled):
    """Two groups with their own lr / betas / eps; one parameter without a gradient on step 2, whose ``step`` then lags."""
    gen = torch.Generator().manual_seed(11)
    shapes = [(7,), (3, 5), (64,), (2, 3, 4)]
    params = [torch.randn(*s, generator=gen, dtype=torch.float64).requires_grad_(True) for s in shapes]
    hyper = [dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8), dict(lr=3e-3, betas=(0.8, 0.95), eps=1e-6)]
    opt = torch.optim.Adam([dict(params=params[:2], **hyper[0]), dict(params=params[2:], **hyper[1])], weight_decay=weight_decay,
                           decoupled_weight_decay=decoupled)
    mine = [(p.detach().clone(), torch.zeros_like(p), torch.zeros_like(p), 0) for p in params]
    for step in range(1, 6):
        grads = [torch.randn(*s, generator=gen, dtype=torch.float64) for s in shapes]
        if step == 2:
            grads[1] = None
        for i, (p, g) in enumerate(zip(params, grads)):
            p.grad = g
            if g is not None:
                h = hyper[0] if i < 2 else hyper[1]
                q, m, v, t = mine[i]
                mine[i] = OS.adam_update(q, g, m, v, t + 1, h["lr"], h["betas"][0], h["betas"][1], h["eps"], weight_decay, decoupled) + (t + 1,)
        opt.step()
        for i, p in enumerate(params):
            q, m, v, t = mine[i]
            st = opt.state[p]
            assert float(st["step"]) == t
            for a, b in ((p.detach(), q), (st["exp_avg"], m), (st["exp_avg_sq"], v)):
                assert float((a - b).abs().max()) <= 1e-14 * float(b.abs().max()), (step, i)
    assert mine[1][3] == 4 and mine[0][3] == 5


def test_entry_and_op_mirrors_have_the_library_layout():
    lib = _capi.load()
    assert lib.hps_sizeof_adam_entry() == ctypes.sizeof(_capi.AdamEntry) and lib.hps_sizeof_refresh_op() == ctypes.sizeof(_capi.RefreshOp)
    assert lib.hps_adam_step(None, 0, None, 0, None) == 0 and lib.hps_weights_refresh(None, 0, None) == 0      # nothing to do
    assert lib.hps_adam_step(None, 3, None, 1, None) == -1 and b"null pointer" in lib.hps_last_error()
    ops = (_capi.RefreshOp * 1)(_capi.RefreshOp(kind=99, src=16, dst=16))
    assert lib.hps_weights_refresh(ops, 1, None) == -1 and b"unknown op kind" in lib.hps_last_error()
    for kind in (_capi.REFRESH_PERMUTE, _capi.REFRESH_FOLD, _capi.REFRESH_WINO_U, _capi.REFRESH_STEM_U):
        ops = (_capi.RefreshOp * 1)(_capi.RefreshOp(kind=kind))
        assert lib.hps_weights_refresh(ops, 1, None) == -1 and b"null pointer" in lib.hps_last_error()
    ops = (_capi.RefreshOp * 1)(_capi.RefreshOp(kind=_capi.REFRESH_FOLD, src=16, dst=16, dst2=16, aux0=16, aux1=16))
    assert lib.hps_weights_refresh(ops, 1, None) == -1 and b"null pointer" in lib.hps_last_error()


def test_winograd_sums_are_exact_for_the_seeded_weights():
    """The precondition of the device check of wino_u: G has only 0, +-1/2 and 1, so every term is an fp32 value times 1, 1/2 or 1/4;
    for the seeded weights of the device tests every float64 sum of the transform is exact -- two summation orders give equal float64
    bits, hence equal fp32 -- and equals _ConvBN's einsum.  stem_u (coefficients with 1/6): two orders stay within one fp32 ulp on
    at most 1 % of the elements, the cap the device test uses."""
    enc = chain_net_cpu().image_encoder
    n_wino = 0
    for name, conv, bn in enc._enc_layers():
        cb = _ConvBN(conv, bn, cin_pad=20 if name == "stem" else None)
        if cb.wino_u is not None:
            a, b = OS.wino_u_flat(conv.weight.detach(), 0), OS.wino_u_flat(conv.weight.detach(), 1)
            assert torch.equal(a, b) and torch.equal(a, cb.wino_u.reshape(-1)), name
            n_wino += 1
    assert n_wino >= 10
    w = enc.conv1.weight.detach()
    a, b, c = OS.stem_u_flat(w, 0), OS.stem_u_flat(w, 1), _stem_winograd_filters(w)[:81 * 1152]
    for x, y in ((a, b), (a, c)):
        d = OS.ulp_distance(x, y)
        print("stem_u: %d of %d elements differ, max %d ulp" % (int((d != 0).sum()), d.numel(), int(d.max())))
        assert int(d.max()) <= 1 and int((d != 0).sum()) <= 0.01 * d.numel()


def test_refresh_lists_reproduce_a_fresh_prepare_on_the_host():
    """Every derived tensor after (perturb the parameters and statistics in place, run the net's own refresh lists through the host
    restatement) equals a fresh prepare() of the perturbed net bit for bit (stem_u: compare_states' cap); a derived tensor without an
    op is named."""
    net = chain_net_cpu()
    net.image_encoder.prepare()
    net.prepare()
    OS.build_backward_entries(net)
    before = {k: v.clone() for k, v in OS.derived_tensors(net).items()}
    gen = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0.05 * torch.randn(p.shape, generator=gen))
        for name, b in net.named_buffers():
            if name.endswith("running_mean"):
                b.add_(0.1 * torch.randn(b.shape, generator=gen))
            elif name.endswith("running_var"):
                b.mul_(1.0 + 0.5 * torch.rand(b.shape, generator=gen))
    lists = [net.image_encoder._refresh_list(net.image_encoder._prepared, None), net._refresh_list(net._prepared, None)]
    for ref in lists:
        OS.run_refresh_ops(ref.ops)
    fresh = copy.deepcopy(net)
    assert fresh._prepared is None and fresh.image_encoder._prepared is None
    fresh.image_encoder.prepare()
    fresh.prepare()
    OS.build_backward_entries(fresh)
    got, want = OS.derived_tensors(net), OS.derived_tensors(fresh)
    print(OS.compare_states(got, want))
    # coverage by name: whatever is not an op's destination is a parameter / buffer itself or did not depend on one
    covered = set().union(*[ref.covered for ref in lists])
    own = {t.data_ptr() for t in list(net.parameters()) + list(net.buffers())}
    for name, t in got.items():
        if t.data_ptr() not in covered and t.data_ptr() not in own and not name.endswith("_ptrs"):
            assert torch.equal(t, before[name]) and torch.equal(t, want[name]), "%s is derived from a parameter and has no refresh op" % name
    changed = [name for name in got if not name.endswith("_ptrs") and not torch.equal(got[name], before[name])]
    assert len(changed) > 150 and len(covered) > 150
