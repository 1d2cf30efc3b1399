"""GPU: the device Adam step (hps_adam_step through device_optim.DeviceAdam) against the float64 restatement of optim_scenario, and
the in-place refresh of the kernel-side weights (hps_weights_refresh through refresh_weights()) against a freshly built net.

Tolerances.  One step: p, m and v are float64 results rounded once, so |dev - ref| <= 2^-23 |ref| against the float64 restatement
evaluated from the same fp32 state (for p a floor of 2^-40 (|p_old| + |delta|) where cancellation leaves p near zero: the device's
float64 and the host's differ in the last places of the update).  Ten steps: the project's rule, error <= 4 max(torch's own CPU fp32
Adam error, 2^-23 max|p|) per tensor.  Refresh: bit-equal to a fresh build; stem_u within 1 ulp on at most 1 % of its elements
(tests/test_optim_host.py shows two float64 summation orders stay inside that cap)."""
import copy
import ctypes

import pytest
import torch

import encoder_grad_scenario as ES
import optim_scenario as OS
from hierarchicalprobabilistic3dhuman_amd import _capi
from hierarchicalprobabilistic3dhuman_amd.device_optim import DeviceAdam, RefreshList
from hierarchicalprobabilistic3dhuman_amd.resnet import _ConvBN
from test_gpu_encoder_backward import chain_loss, chain_net

pytestmark = pytest.mark.gpu

GUARD = 12345.0
HYPER = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
WD_FORMS = {"none": dict(weight_decay=0.0), "l2": dict(weight_decay=0.01), "decoupled": dict(weight_decay=0.01, decoupled_weight_decay=True)}


def guarded(values, dev, align):
    """``values`` as views into one buffer full of guard words, a guard gap between them; align 4: every view starts on 16 bytes,
    align 1: none does (the 4-byte route).  Returns (buffer, views, mask of the guard words)."""
    starts, at = [], align
    for v in values:
        if align == 1 and at % 4 == 0:
            at += 1
        starts.append(at)
        at = (at + v.numel() + align + align - 1) // align * align
    buf = torch.full((at + 4,), GUARD, device=dev)
    mask = torch.ones(at + 4, dtype=torch.bool, device=dev)
    views = []
    for s, v in zip(starts, values):
        buf[s:s + v.numel()] = v.to(dev)
        mask[s:s + v.numel()] = False
        views.append(buf[s:s + v.numel()])
        assert (views[-1].data_ptr() % 16 == 0) == (align == 4)
    return buf, views, mask


def preload(opt, params, ms, vs, step0):
    for p, m, v in zip(params, ms, vs):
        opt.state[p] = {"step": torch.tensor(float(step0)), "exp_avg": m, "exp_avg_sq": v}


@pytest.mark.parametrize("step0", [0, 999])
@pytest.mark.parametrize("align", [1, 4])
def test_one_step_against_the_float64_restatement(dev, align, step0):
    """Seven tensors of 1 ... 70 001 elements in one launch, every weight-decay form, v from zero and at step 1000; guard words around
    every parameter, exp_avg and exp_avg_sq stay as they were."""
    gen = torch.Generator().manual_seed(8 + step0)
    p0, g0 = OS.parameters(), OS.gradients()
    m0 = [torch.zeros_like(p) if step0 == 0 else 0.1 * torch.randn(p.shape, generator=gen) * g.abs().clamp_min(1e-6) for p, g in zip(p0, g0)]
    v0 = [torch.zeros_like(p) if step0 == 0 else (torch.rand(p.shape, generator=gen) + 0.5) * g * g for p, g in zip(p0, g0)]
    for form, wd in WD_FORMS.items():
        bufs = [guarded(t, dev, align) for t in (p0, m0, v0)]
        (pb, ps, pmask), (mb, ms, mmask), (vb, vs, vmask) = bufs
        opt = DeviceAdam(ps, **HYPER, **wd)
        preload(opt, ps, ms, vs, step0)
        for p, g in zip(ps, g0):
            p.grad = g.to(dev)
        opt.step()
        for buf, _, mask in bufs:
            assert bool((buf[mask] == GUARD).all()), "memory outside the tensors was written"
        worst = 0.0
        for i, (p, m, v) in enumerate(zip(ps, ms, vs)):
            rp, rm, rv = OS.adam_update(p0[i], g0[i], m0[i], v0[i], step0 + 1, HYPER["lr"], *HYPER["betas"], HYPER["eps"],
                                        wd["weight_decay"], wd.get("decoupled_weight_decay", False))
            floor = 2.0 ** -40 * (p0[i].double().abs() + (rp - p0[i].double()).abs())
            for name, got, ref, fl in (("p", p, rp, floor), ("m", m, rm, 0.0), ("v", v, rv, 0.0)):
                err = (got.cpu().double() - ref).abs()
                tol = torch.maximum(OS.EPS32 * ref.abs(), torch.as_tensor(fl, dtype=torch.float64))
                worst = max(worst, float((err / tol.clamp_min(1e-300)).max()))
                assert bool((err <= tol).all()), (form, i, name, float((err - tol).max()))
            assert float(opt.state[p]["step"]) == step0 + 1
        print("align %d step0 %d %s: worst error / tolerance = %.3f" % (align, step0, form, worst))


def trajectory_inputs(steps=10):
    gen = torch.Generator().manual_seed(31)
    p0 = OS.parameters()
    base = OS.gradients()
    grads = [[g * (0.5 + torch.rand(g.shape, generator=gen)) * torch.sign(torch.randn(g.shape, generator=gen)) for g in base] for _ in range(steps)]
    return p0, grads


def reference_trajectories(p0, grads, wd):
    """(float64 trajectory, torch's CPU fp32 Adam) after all steps."""
    f64 = [(p.double(), torch.zeros_like(p, dtype=torch.float64), torch.zeros_like(p, dtype=torch.float64)) for p in p0]
    cpu = [p.clone() for p in p0]
    opt = torch.optim.Adam(cpu, foreach=False, **HYPER, **wd)
    for t, gs in enumerate(grads, 1):
        f64 = [OS.adam_update(p, g, m, v, t, HYPER["lr"], *HYPER["betas"], HYPER["eps"], wd["weight_decay"],
                              wd.get("decoupled_weight_decay", False)) for (p, m, v), g in zip(f64, gs)]
        for p, g in zip(cpu, gs):
            p.grad = g.clone()
        opt.step()
    return [p for p, _, _ in f64], cpu


def check_trajectory(tag, got, f64, cpu32):
    for i, (g, r, c) in enumerate(zip(got, f64, cpu32)):
        err, ref_err = float((g.cpu().double() - r).abs().max()), float((c.double() - r).abs().max())
        bound = 4.0 * max(ref_err, OS.EPS32 * float(r.abs().max()))
        print("%s tensor %d: max|dev - f64| = %.3e  max|cpu32 - f64| = %.3e  bound %.3e" % (tag, i, err, ref_err, bound))
        assert err <= bound, (tag, i, err, bound)


def run(opt, params, grads, dev):
    for gs in grads:
        for p, g in zip(params, gs):
            p.grad = g.to(dev)
        opt.step()


@pytest.mark.parametrize("form", sorted(WD_FORMS))
def test_ten_steps_and_state_dict_round_trips(dev, form):
    """Against the float64 trajectory by the project's rule; torch.optim.Adam continues a DeviceAdam state dict and the reverse."""
    wd = WD_FORMS[form]
    p0, grads = trajectory_inputs()
    f64, cpu32 = reference_trajectories(p0, grads, wd)
    ps = [p.to(dev) for p in p0]
    opt = DeviceAdam(ps, **HYPER, **wd)
    run(opt, ps, grads, dev)
    check_trajectory("device", ps, f64, cpu32)
    # five device steps, then torch continues
    ps = [p.to(dev) for p in p0]
    first = DeviceAdam(ps, **HYPER, **wd)
    run(first, ps, grads[:5], dev)
    sd = first.state_dict()
    assert all(s["step"].device.type == "cpu" and s["step"].dtype == torch.float32 and set(s) == {"step", "exp_avg", "exp_avg_sq"}
               for s in sd["state"].values())
    second = torch.optim.Adam(ps, **HYPER, **wd)
    second.load_state_dict(sd)
    run(second, ps, grads[5:], dev)
    check_trajectory("device then torch", ps, f64, cpu32)
    # five torch steps, then the device continues
    ps = [p.to(dev) for p in p0]
    first = torch.optim.Adam(ps, **HYPER, **wd)
    run(first, ps, grads[:5], dev)
    second = DeviceAdam(ps, **HYPER, **wd)
    second.load_state_dict(first.state_dict())
    run(second, ps, grads[5:], dev)
    check_trajectory("torch then device", ps, f64, cpu32)
    assert all(float(second.state[p]["step"]) == 10 for p in ps)


def test_repeatable_independent_of_the_launch_and_none_gradients(dev):
    p0, g0 = OS.parameters(), OS.gradients()

    def once(indices, none=()):
        ps = [p0[i].to(dev) for i in indices]
        opt = DeviceAdam(ps, **HYPER, weight_decay=0.01)
        for _ in range(2):
            versions = [p._version for p in ps]
            for k, (p, i) in enumerate(zip(ps, indices)):
                p.grad = None if i in none else g0[i].to(dev)
            opt.step()
            assert [p._version - v for p, v in zip(ps, versions)] == [0 if i in none else 1 for i in indices]
        return ps, opt

    a, opt_a = once(range(7))
    b, _ = once(range(7))
    assert all(torch.equal(x, y) for x, y in zip(a, b))                      # two runs: equal bits
    for i in (0, 4, 6):                                                      # alone and inside the seven-tensor launch: equal bits
        alone, opt1 = once([i])
        assert torch.equal(alone[0], a[i])
        assert torch.equal(opt1.state[alone[0]]["exp_avg_sq"], opt_a.state[a[i]]["exp_avg_sq"])
    c, opt_c = once(range(7), none=(2, 5))
    for i in range(7):
        if i in (2, 5):                                                      # no gradient: bit-unchanged, no state, no step
            assert torch.equal(c[i].cpu(), p0[i]) and len(opt_c.state[c[i]]) == 0
        else:
            assert torch.equal(c[i], a[i]) and float(opt_c.state[c[i]]["step"]) == 2
    # a gradient that arrives later starts that tensor's own count; a non-contiguous gradient is made contiguous on the host side
    wide = torch.stack([g0[5], g0[5]], 1).to(dev)
    c[5].grad = wide[:, 0]
    assert not c[5].grad.is_contiguous()
    for i in (0, 1, 2, 3, 4, 6):
        c[i].grad = None
    opt_c.step()
    assert float(opt_c.state[c[5]]["step"]) == 1 and float(opt_c.state[c[0]]["step"]) == 2 and len(opt_c.state[c[2]]) == 0
    alone = [p0[5].to(dev)]
    alone[0].grad = g0[5].to(dev)
    DeviceAdam(alone, **HYPER, weight_decay=0.01).step()
    assert torch.equal(alone[0], c[5])


def test_refusals_leave_parameters_and_state_unchanged(dev):
    p0, g0 = OS.parameters()[:3], OS.gradients()[:3]

    def fresh(**kw):
        ps = [p.to(dev) for p in p0]
        opt = DeviceAdam(ps, **HYPER, **kw)
        for p, g in zip(ps, g0):
            p.grad = g.to(dev)
        opt.step()
        return ps, opt

    def unchanged(ps, opt, snap):
        now = [t.clone() for p in ps for t in (p, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"], opt.state[p]["step"])]
        return all(torch.equal(a.cpu(), b.cpu()) for a, b in zip(now, snap))

    snap_of = lambda ps, opt: [t.clone() for p in ps for t in (p, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"], opt.state[p]["step"])]
    ps, opt = fresh()
    snap = snap_of(ps, opt)
    with pytest.raises(NotImplementedError):
        opt.step(lambda: 0.0)
    for flag in ("amsgrad", "maximize", "differentiable"):
        opt.param_groups[0][flag] = True
        with pytest.raises(NotImplementedError):
            opt.step()
        opt.param_groups[0][flag] = False
    opt.param_groups[0]["lr"] = torch.tensor(1e-3)
    with pytest.raises(NotImplementedError):
        opt.step()
    opt.param_groups[0]["lr"] = 1e-3
    opt.param_groups[0]["betas"] = (torch.tensor(0.9), 0.999)
    with pytest.raises(NotImplementedError):
        opt.step()
    opt.param_groups[0]["betas"] = HYPER["betas"]
    ps[2].grad = g0[2].to(dev).to_sparse()                                   # the LAST tensor: the first two must not have been stepped
    with pytest.raises(_capi.HpsError):
        opt.step()
    ps[2].grad = g0[2].to(dev)
    assert unchanged(ps, opt, snap)
    half = [p.to(dev).half() for p in p0[:1]] + [p0[1].to(dev)]
    opt_h = DeviceAdam(half, **HYPER)
    half[0].grad, half[1].grad = g0[0].to(dev).half(), g0[1].to(dev)
    with pytest.raises(_capi.HpsError):
        opt_h.step()
    assert torch.equal(half[1].cpu(), p0[1]) and len(opt_h.state[half[1]]) == 0
    cpu = [p0[0].to(dev), p0[1].clone()]
    opt_c = DeviceAdam(cpu, **HYPER)
    cpu[0].grad, cpu[1].grad = g0[0].to(dev), g0[1].clone()
    with pytest.raises(_capi.HpsError):
        opt_c.step()
    assert torch.equal(cpu[0].cpu(), p0[0]) and torch.equal(cpu[1], p0[1]) and len(opt_c.state[cpu[0]]) == 0
    # accepted and ignored
    for kw in (dict(foreach=True), dict(foreach=False), dict(capturable=True), dict(fused=True)):
        try:
            got, _ = fresh(**kw)
        except (RuntimeError, ValueError) as e:                               # torch's own constructor may refuse a combination
            print("torch refuses %s: %s" % (kw, e))
            continue
        assert all(torch.equal(a, b) for a, b in zip(got, ps)), kw
    opt.step()                                                               # and the optimiser still works
    assert not unchanged(ps, opt, snap)


def test_copies_device_counters_and_empty_parameters(dev):
    """A deepcopied / unpickled DeviceAdam steps (with no module registered); a state dict whose ``step`` lives on the device
    (torch.optim.Adam(capturable=True)) is continued with the counters back on the host; a zero-element parameter gets its state and
    its step as torch gives them; a launch that is refused leaves the counters where they were; fused=True does not claim the
    GradScaler's grad_scale / found_inf route."""
    import pickle
    p0, g0 = OS.parameters()[:4], OS.gradients()[:4]
    ps = [p.to(dev) for p in p0] + [torch.zeros(0, device=dev)]
    opt = DeviceAdam(ps, **HYPER, fused=True)
    assert not getattr(opt, "_step_supports_amp_scaling", False)
    for p, g in zip(ps, g0 + [torch.zeros(0)]):
        p.grad = g.to(dev)
    opt.step()
    assert float(opt.state[ps[4]]["step"]) == 1 and opt.state[ps[4]]["exp_avg"].numel() == 0
    want = [p.clone() for p in ps]
    twin = [p.clone() for p in ps]
    for clone in (copy.deepcopy(opt), pickle.loads(pickle.dumps(opt))):
        qs = [q for g in clone.param_groups for q in g["params"]]
        assert clone._refresh == [] and all(torch.equal(a, b) for a, b in zip(qs, want))
        for q, p in zip(qs, ps):
            q.grad = p.grad.clone()
        clone.step()
        assert all(float(clone.state[q]["step"]) == 2 for q in qs)
        twin = qs
    opt.step()
    assert all(torch.equal(a, b) for a, b in zip(ps, twin))                   # the copy continued exactly as the original does
    # counters on the device
    rs = [p.to(dev) for p in p0]
    cap = torch.optim.Adam(rs, **HYPER, capturable=True)
    for r, g in zip(rs, g0):
        r.grad = g.to(dev)
    cap.step()
    assert cap.state[rs[0]]["step"].is_cuda
    mine = DeviceAdam(rs, **HYPER)
    sd = cap.state_dict()
    sd["param_groups"][0]["capturable"] = False
    mine.load_state_dict(sd)
    mine.step()
    assert all(float(mine.state[r]["step"]) == 2 and not mine.state[r]["step"].is_cuda for r in rs)
    for r, p in zip(rs, ps):
        assert float((r - p).abs().max()) <= 4 * OS.EPS32 * float(p.abs().max())  # two steps either way
    # a refused launch
    real = _capi.call
    try:
        def refuse(name, *a):
            raise _capi.HpsError(name)
        _capi.call = refuse
        with pytest.raises(_capi.HpsError):
            mine.step()
    finally:
        _capi.call = real
    assert all(float(mine.state[r]["step"]) == 2 for r in rs)


# ---- the refresh against a fresh build ----
def configure(net, bn_mode, winograd):
    net.image_encoder.set_winograd(winograd)
    if bn_mode == "train":
        net.set_batchnorm_training(True)
        net.train()
        net.image_encoder.bn1.eval()                 # the stem and layer1 frozen: eval layers beside training layers
        net.image_encoder.layer1.eval()
    return net


def train_steps(net, smpl, x, opt, steps):
    for _ in range(steps):
        net.zero_grad(set_to_none=True)
        loss = chain_loss(net, smpl, x)
        loss.backward()
        opt.step()
    return loss


def scenario(dev, smpl, bn_mode, winograd, steps):
    """(a net of its own for the calling test after ``steps`` registered steps on the loss chain, its optimiser)."""
    x = ES.case("sq64")[0].to(dev)
    net = configure(chain_net(dev), bn_mode, winograd)
    opt = DeviceAdam(net.parameters(), lr=1e-4, refresh=(net,))
    train_steps(net, smpl, x, opt, steps)
    return net, opt


def fresh_like(net, dev, bn_mode, winograd):
    fresh = configure(chain_net(dev), bn_mode, winograd)
    fresh.load_state_dict(net.state_dict())
    return fresh


def outputs_equal(a, b):
    for u, v in zip(a, b):
        if isinstance(u, torch.Tensor):
            assert torch.equal(u, v)
        else:
            assert torch.equal(u.loc, v.loc) and torch.equal(u.scale, v.scale)


@pytest.mark.parametrize("steps", [1, 2])
@pytest.mark.parametrize("winograd", [True, False], ids=["default", "no_winograd"])
@pytest.mark.parametrize("bn_mode", ["eval", "train"])
def test_refreshed_state_equals_a_fresh_build(dev, smpl_gpu, bn_mode, winograd, steps):
    x = ES.case("sq64")[0].to(dev)
    net, opt = scenario(dev, smpl_gpu, bn_mode, winograd, steps)
    enc = net.image_encoder
    assert "refresh" in enc.device_state() and "refresh" in net.device_state()
    fresh = fresh_like(net, dev, bn_mode, winograd)
    chain_loss(fresh, smpl_gpu, x).backward()                                # prepared the same way: its backward entries exist
    got, want = OS.derived_tensors(net), OS.derived_tensors(fresh)
    assert len([k for k in want if ".bwd." in k]) >= 20
    print("%s %s %d step(s): %s" % (bn_mode, winograd, steps, OS.compare_states(got, want)))
    # by name: a derived tensor is an op's destination, a parameter / buffer itself, or does not depend on a parameter
    covered = enc.device_state()["refresh"].covered | net.device_state()["refresh"].covered
    own = {t.data_ptr() for t in list(net.parameters()) + list(net.buffers())}
    static = ("ident", "zeros", "sgc_add", "anc_ptr", "anc_idx", "levels", "level_joints", "level_sizes_host", "desc_ptr", "desc_joint",
              "desc_pos", "in_off")
    for name, t in got.items():
        if t.data_ptr() in covered or t.data_ptr() in own or name.endswith("_ptrs"):
            continue
        assert any(part in static for part in name.split(".")), "%s is derived from a parameter and has no refresh op" % name
    # the next forward: stepped net against a net built from its state dict
    # (the comparison of the states above ran a backward on ``fresh``, which under .train() moved its buffers: a new one)
    stepped, state = net, net.device_state()
    fresh = fresh_like(net, dev, bn_mode, winograd)
    with torch.no_grad():
        a, b = stepped(x), fresh(x)
    c, d = stepped(x), fresh(x)
    if not winograd:
        outputs_equal(a, b)
        outputs_equal(c, d)
        for (k, u), (_, v) in zip(stepped.named_buffers(), fresh.named_buffers()):
            assert torch.equal(u, v), k
    else:
        fa, fb = stepped.image_encoder(x).detach(), fresh.image_encoder(x).detach()
        assert float((fa - fb).abs().max()) <= 1e-4 * float(fb.abs().max())
    assert net.device_state() is state


def test_refreshed_layers_give_a_fresh_build_s_bits_on_the_same_input(dev, smpl_gpu):
    """Default kernels: every non-stem layer of the stepped net against the same layer of the fresh build on one input frame.  First
    the precondition of the bit-equal wino_u check on THESE weights, after two Adam steps (tests/test_optim_host.py shows it for the
    seeded ones): every float64 sum of G g G^T is exact -- two summation orders give equal bits -- and is what the refresh wrote."""
    net, _ = scenario(dev, smpl_gpu, "eval", True, 2)
    convs = [c for blk in net.image_encoder._prepared["blocks"] for c in blk if c is not None]
    checked = 0
    for (name, conv, _), cb in zip(net.image_encoder._enc_layers()[1:], convs):
        if cb.wino_u is not None:
            a, b = OS.wino_u_flat(conv.weight.detach(), 0), OS.wino_u_flat(conv.weight.detach(), 1)
            assert torch.equal(a, b) and torch.equal(a, cb.wino_u.reshape(-1)), name
            checked += 1
    assert checked >= 10
    fresh = fresh_like(net, dev, "eval", True)
    fresh.image_encoder.prepare()
    gen = torch.Generator().manual_seed(2)
    mine, theirs = net.image_encoder._prepared["blocks"], fresh.image_encoder._prepared["blocks"]
    h = 16
    for (a1, a2, ad), (b1, b2, bd) in zip(mine, theirs):
        for ca, cb in ((a1, b1), (a2, b2), (ad, bd)):
            if ca is None:
                continue
            hin = h if ca is not a2 else ca_out
            xp = torch.zeros(3, hin + 2, hin + 2, ca.cin_p, device=dev)
            xp[:, 1:-1, 1:-1] = torch.randn(3, hin, hin, ca.cin_p, generator=gen).to(dev)
            ho, _ = ca.out_hw(hin, hin)
            outs = []
            for c in (ca, cb):
                out = torch.zeros(3, ho + 2, ho + 2, c.cout, device=dev)
                outs.append(c.padded(xp, 1, out, 1))
            assert torch.equal(outs[0], outs[1]) and float(outs[0].abs().max()) > 0
            if ca is a1:
                ca_out = ho
        h = ca_out


def state_pointers(obj, out=None):
    """Addresses of every tensor, launch-list array and op under a device state."""
    out = [] if out is None else out
    if isinstance(obj, torch.Tensor):
        out.append(obj.data_ptr())
    elif isinstance(obj, (ctypes.Array, ctypes.Structure)):
        out.append(ctypes.addressof(obj))
    elif isinstance(obj, dict):
        for k in sorted(obj, key=repr):
            state_pointers(obj[k], out)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            state_pointers(v, out)
    elif isinstance(obj, _ConvBN):
        state_pointers(vars(obj), out)
    elif isinstance(obj, RefreshList):
        state_pointers(obj.array, out)
    return out


@pytest.mark.parametrize("bn_mode", ["eval", "train"])
def test_nothing_is_rebuilt_over_registered_steps(dev, smpl_gpu, bn_mode):
    x = ES.case("sq64")[0].to(dev)
    net = configure(chain_net(dev), bn_mode, True)
    enc = net.image_encoder
    opt = DeviceAdam(net.parameters(), lr=1e-4, refresh=(net,))
    train_steps(net, smpl_gpu, x, opt, 1)
    prep, head_prep, enc_state, head_state = enc._prepared, net._prepared, enc.device_state(), net.device_state()
    pointers = state_pointers(enc_state) + state_pointers(head_state)
    assert len(pointers) > 300
    allocated = []
    for _ in range(2):
        train_steps(net, smpl_gpu, x, opt, 1)
        allocated.append(torch.cuda.memory_allocated())
        assert enc._prepared is prep and net._prepared is head_prep and enc.device_state() is enc_state and net.device_state() is head_state
        assert state_pointers(enc_state) + state_pointers(head_state) == pointers
    assert allocated[0] == allocated[1], allocated
    with torch.no_grad():
        net(x)
    assert enc._prepared is prep and net._prepared is head_prep
    # the fallback still works, and this test tells the two apart: torch's Adam drops the prepared state at the next forward
    other = configure(chain_net(dev), bn_mode, True)
    topt = torch.optim.Adam(other.parameters(), lr=1e-4)
    train_steps(other, smpl_gpu, x, topt, 1)
    prep = other.image_encoder._prepared
    train_steps(other, smpl_gpu, x, topt, 1)
    assert other.image_encoder._prepared is not prep


def test_fallbacks(dev, smpl_gpu):
    x = ES.case("sq64")[0].to(dev)
    # unregistered: the version path sees the step; the same bits as the registered run on the direct kernels
    reg, _ = scenario(dev, smpl_gpu, "eval", False, 2)
    plain = configure(chain_net(dev), "eval", False)
    opt = DeviceAdam(plain.parameters(), lr=1e-4)
    prep = None
    for _ in range(2):
        train_steps(plain, smpl_gpu, x, opt, 1)
        assert plain.image_encoder._prepared is not prep                      # rebuilt behind every step
        prep = plain.image_encoder._prepared
    for (k, u), (_, v) in zip(reg.named_parameters(), plain.named_parameters()):
        assert torch.equal(u, v), k
    with torch.no_grad():
        outputs_equal(reg(x), plain(x))
    assert plain.image_encoder._prepared is not prep
    # a torch in-place edit after a registered step still invalidates
    net = copy.deepcopy(reg)
    opt = DeviceAdam(net.parameters(), lr=1e-4, refresh=(net,))
    train_steps(net, smpl_gpu, x, opt, 1)
    state, head_state = net.image_encoder.device_state(), net.device_state()
    with torch.no_grad():
        net(x)
        assert net.image_encoder.device_state() is state
        net.image_encoder.layer2[0].conv1.weight.mul_(1.5)
        net.fc1.bias.add_(0.25)
        got = net(x)
    assert net.image_encoder.device_state() is not state and net.device_state() is not head_state
    with torch.no_grad():
        outputs_equal(got, fresh_like(net, dev, "eval", False)(x))
    # after load_state_dict a registered step works on the new state
    net.load_state_dict(reg.state_dict())
    assert net.image_encoder._prepared is None and net._prepared is None
    opt.step()                                                               # no prepared state: nothing to refresh, nothing fails
    train_steps(net, smpl_gpu, x, opt, 1)
    with torch.no_grad():
        outputs_equal(net(x), fresh_like(net, dev, "eval", False)(x))
    # deepcopy drops the refresh list with the rest of the device state
    assert "refresh" in net.image_encoder.device_state()
    clone = copy.deepcopy(net)
    assert clone.image_encoder.device_state() == {} and clone.device_state() == {}


def test_stage2_chain_two_registered_steps(dev, smpl_gpu):
    """tests/test_gpu_stage2.py's training step at B = 3 under a registered DeviceAdam: every parameter moves, the loss stays finite."""
    import head_grad_scenario as HS
    from hierarchicalprobabilistic3dhuman_amd import configs
    from hierarchicalprobabilistic3dhuman_amd.matrix_fisher_loss import PoseMFShapeGaussianLoss
    from test_gpu_stage2 import outputs, stage2_loss, stage2_targets
    net = HS.make_net("spread")
    ES.randomize_bn(net.image_encoder)
    net = net.to(dev)
    net.set_differentiable_factors(True)
    net.set_batchnorm_training(True)
    net.train()
    x = ES.case("sq64")[0].to(dev)
    criterion = PoseMFShapeGaussianLoss(loss_config=configs.get_cfg_defaults().LOSS.STAGE2, img_wh=256)
    target = stage2_targets(x.shape[0], dev)
    opt = DeviceAdam(net.parameters(), lr=1e-4, refresh=(net,))
    prep = None
    for step in range(2):
        before = {k: p.detach().clone() for k, p in net.named_parameters()}
        net.zero_grad(set_to_none=True)
        loss, _, _ = stage2_loss(net, smpl_gpu, outputs(net(x)), target, criterion, False, 17 + step, 23 + step)
        loss.backward()
        opt.step()
        assert bool(torch.isfinite(loss))
        assert all(not torch.equal(p, before[k]) and bool(torch.isfinite(p).all()) for k, p in net.named_parameters())
        assert prep is None or net.image_encoder._prepared is prep
        prep = net.image_encoder._prepared
