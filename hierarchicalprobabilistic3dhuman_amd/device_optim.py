"""The optimiser step on the device (run_train.py:97: ``optim.Adam(pose_shape_model.parameters(), lr=1e-4)``;
train/train_poseMF_shapeGaussian_net.py:346-349) and the refresh of the kernel-side weights behind it (csrc/optim.hip).

    opt = DeviceAdam(net.parameters(), lr=1e-4, refresh=(net,))
    loss.backward(); opt.step()          # ONE launch for every parameter, then the registered modules' refresh lists

``DeviceAdam`` is ``torch.optim.Adam`` with the same constructor, ``param_groups`` and per-parameter state (``step`` a CPU float32
scalar, ``exp_avg``, ``exp_avg_sq``): its ``state_dict()`` loads into ``torch.optim.Adam`` and back.  ``step()`` builds one table
entry per parameter with a gradient and the workgroup map in a page-locked block, copies it with one asynchronous copy and calls
hps_adam_step.  It bumps the stepped parameters' version counters (host only), so autograd's saved-tensor checks stay truthful and a
module that was NOT registered notices the step on its next forward and rebuilds its device state as after any in-place edit.  A
registered module (``refresh=`` / ``register``) instead runs its refresh list (``refresh_weights()``): every tensor ``prepare()``
derives from a trainable parameter is written again in place; frames, launch lists and pointer tables survive.

Between steps the optimiser keeps the table of the last parameter selection (pointers, hyper-parameters, the workgroup map) and
patches only the gradients' addresses and the bias corrections; a changed selection, hyper-parameter, storage or state rebuilds it.
The counters move after the launch has been queued, so a step that raises leaves them where they were.

There is no CPU path: CPU tensors, non-fp32 parameters and sparse gradients are refused (HpsError) before any launch, as are the
variants that are not implemented (NotImplementedError: amsgrad, maximize, differentiable, a closure, tensor-valued lr / betas).
``foreach``, ``fused`` and ``capturable`` only select torch's implementation and are accepted and ignored.
"""
import ctypes

import numpy as np
import torch

from . import _capi

_ENTRY = np.dtype([(n, "<u8") for n in ("param", "grad", "exp_avg", "exp_avg_sq")] + [("numel", "<i8")] + [
    (n, "<f8") for n in ("lr", "beta1", "beta2", "eps", "weight_decay", "bias_correction1", "bias_correction2_sqrt")] + [
    ("decoupled", "<i4"), ("reserved", "<i4")])
assert _ENTRY.itemsize == ctypes.sizeof(_capi.AdamEntry)


class DeviceAdam(torch.optim.Adam):
    """All parameters live on ONE device, the current one at every ``step()`` (the launch goes to the current device's current
    stream, the table to the current device's memory); anything else is refused.  A copy (deepcopy / pickle) carries
    ``param_groups`` and the state as any torch optimiser does, and no registered module: register the copy's own."""

    def __init__(self, params, *args, refresh=(), **kwargs):
        super().__init__(params, *args, **kwargs)
        self._init_device_side()
        for module in refresh:
            self.register(module)

    def _init_device_side(self):
        self._refresh = []
        self._slots = [None, None]       # (page-locked block, device block, event behind the copy), used alternately
        self._turn = 0
        self._forget()
        # torch sets this with fused=True and GradScaler.step() then passes grad_scale / found_inf INSTEAD of unscaling; this step has
        # no such arguments, so the scaler takes its ordinary route: unscale, check, step()
        self._step_supports_amp_scaling = False

    def _forget(self):
        """Drop what step() keeps between calls (the table of the last parameter selection, the home of the step counters)."""
        self._plan = None
        self._flat = None
        self._step_buf = None

    def __setstate__(self, state):
        refresh = self.__dict__.get("_refresh")
        super().__setstate__(state)
        if refresh is None:                                   # a copy / an unpickled optimiser: Optimizer's state carries none of this
            self._init_device_side()
        else:                                                 # load_state_dict: new state tensors, the same modules
            self._forget()

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        if "_refresh" in self.__dict__:
            self._forget()

    def register(self, module):
        """``module.refresh_weights()`` runs after every step (ResNet, PoseMFShapeGaussianNet)."""
        if not callable(getattr(module, "refresh_weights", None)):
            raise TypeError("%s has no refresh_weights()" % type(module).__name__)
        if not any(m is module for m in self._refresh):
            self._refresh.append(module)
        return module

    # ---- what is refused, before anything is touched ----
    @staticmethod
    def _check_group(group):
        for flag in ("amsgrad", "maximize", "differentiable"):
            if group.get(flag):
                raise NotImplementedError("DeviceAdam: %s=True is not implemented on the device" % flag)
        if isinstance(group["lr"], torch.Tensor) or any(isinstance(b, torch.Tensor) for b in group["betas"]):
            raise NotImplementedError("DeviceAdam: tensor-valued lr / betas are not implemented on the device")

    @staticmethod
    def _check_tensor(t, what, like=None):
        if t.is_sparse:
            raise _capi.HpsError("DeviceAdam: sparse %s; the device step takes dense gradients only" % what)
        if not t.is_cuda:
            raise _capi.HpsError("DeviceAdam: %s lives on the CPU; this package has no CPU path" % what)
        if t.dtype != torch.float32:
            raise _capi.HpsError("DeviceAdam: %s is %s; the device step is fp32" % (what, t.dtype))
        if like is not None and (t.shape != like.shape or t.device != like.device):
            raise _capi.HpsError("DeviceAdam: %s does not match its parameter" % what)

    def _block(self, nbytes):
        """The next (page-locked block, device block) of at least ``nbytes``; waits for the copy that last read the block."""
        self._turn ^= 1
        slot = self._slots[self._turn]
        if slot is not None:
            slot[2].synchronize()
        if slot is None or slot[0].numel() < nbytes:
            size = max(1 << 16, 2 * nbytes)
            slot = (torch.empty(size, dtype=torch.uint8, pin_memory=True), torch.empty(size, dtype=torch.uint8, device="cuda"),
                    torch.cuda.Event())
            self._slots[self._turn] = slot
        return slot

    def _parameters(self):
        """[(group index, parameter)] in param_groups order, and the one CPU float32 buffer whose elements are the ``step`` scalars
        (state[p]["step"] is a 0-dim view of its element: torch's layout, and the host advances all of them with one addition)."""
        if self._flat is None or len(self._flat) != sum(len(g["params"]) for g in self.param_groups):
            self._flat = [(gi, p) for gi, g in enumerate(self.param_groups) for p in g["params"]]
            self._step_buf = torch.zeros(len(self._flat), dtype=torch.float32)
            self._plan = None
        return self._flat

    def _build_plan(self, key, sel):
        """Everything about a selection of parameters that does not change from step to step: the checked parameters and state,
        the table with its pointer and hyper-parameter columns, the workgroup map.  State is created here (first step with a
        gradient) and ``step`` is moved into the counter buffer (a loaded state dict may hold it anywhere, also on the device)."""
        flat = self._flat
        chosen = [flat[i] for i in sel]
        for _, p in chosen:                                   # every refusal before anything is created or moved
            self._check_tensor(p, "parameter")
            if not p.is_contiguous():
                raise _capi.HpsError("DeviceAdam: parameters must be contiguous")
            _capi.require_device(p, "parameter")
            state = self.state.get(p)
            if state:
                self._check_tensor(state["exp_avg"], "exp_avg", p)
                self._check_tensor(state["exp_avg_sq"], "exp_avg_sq", p)
        n = len(chosen)
        table = np.zeros(n, dtype=_ENTRY)
        states = []
        for k, (i, (gi, p)) in enumerate(zip(sel, chosen)):
            group, state = self.param_groups[gi], self.state[p]
            if len(state) == 0:
                state["step"] = torch.tensor(0.0, dtype=torch.float32)
                state["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            for name in ("exp_avg", "exp_avg_sq"):
                if not state[name].is_contiguous():
                    state[name] = state[name].contiguous()
            home = self._step_buf[i]
            if state["step"].data_ptr() != home.data_ptr():
                home.copy_(state["step"].detach().reshape(()).to("cpu", torch.float32))
                state["step"] = home
            beta1, beta2 = (float(b) for b in group["betas"])
            table[k] = (p.data_ptr(), 0, state["exp_avg"].data_ptr(), state["exp_avg_sq"].data_ptr(), p.numel(), float(group["lr"]), beta1,
                        beta2, float(group["eps"]), float(group["weight_decay"]), 0.0, 0.0, 1 if group.get("decoupled_weight_decay") else 0, 0)
            states.append(state)
        chunks = (table["numel"] + _capi.ADAM_CHUNK - 1) // _capi.ADAM_CHUNK
        n_blocks = int(chunks.sum())
        block_map = np.empty((n_blocks, 2), dtype=np.int32)
        block_map[:, 0] = np.repeat(np.arange(n, dtype=np.int32), chunks)
        block_map[:, 1] = np.arange(n_blocks, dtype=np.int64) - np.repeat(np.cumsum(chunks) - chunks, chunks)
        pointers = [x for st, (_, p) in zip(states, chosen) for x in (p.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr())]
        groups = sorted({gi for gi, _ in chosen})
        rows = {gi: np.array([k for k, (g, _) in enumerate(chosen) if g == gi]) for gi in groups}
        self._plan = dict(key=key, table=table, map_bytes=block_map.reshape(-1).view(np.uint8), n_blocks=n_blocks, states=states,
                          params=[p for _, p in chosen], pointers=pointers, index=np.array(sel), rows=rows)
        return self._plan

    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None:
            raise NotImplementedError("DeviceAdam: a closure is not implemented (evaluate the loss before step())")
        hyper = []
        for group in self.param_groups:
            self._check_group(group)
            hyper.append((group["lr"], group["betas"], group["eps"], group["weight_decay"], group.get("decoupled_weight_decay")))
        f32, strided = torch.float32, torch.strided
        sel, grads, grad_ptrs = [], [], []
        for i, (_, p) in enumerate(self._parameters()):
            g = p.grad
            if g is None:
                continue                                      # skipped with its state untouched, as torch does
            if not (g.is_cuda and g.dtype is f32 and g.layout is strided and g.is_contiguous()):
                self._check_tensor(g, "gradient")
                g = g.contiguous()                            # made contiguous on the host side of the call
                grads.append(g)                               # its owner until the launch is queued
            sel.append(i)
            grad_ptrs.append(g.data_ptr())
        if not sel:
            return None
        key = (tuple(sel), tuple(hyper))
        plan = self._plan
        if plan is not None and plan["key"] == key:
            now = [x for st, p in zip(plan["states"], plan["params"]) for x in (p.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr())]
            if now != plan["pointers"] or any(self.state.get(p) is not st for st, p in zip(plan["states"], plan["params"])):
                plan = None                                   # a parameter's storage or a state tensor was replaced by hand
        else:
            plan = None
        if plan is None:
            plan = self._build_plan(key, sel)
        # what does change: the gradients' addresses and the two bias corrections, as torch computes them (Python floats)
        table, counters = plan["table"], self._step_buf.numpy()
        steps = counters[plan["index"]] + np.float32(1.0)
        table["grad"] = grad_ptrs
        for gi, rows in plan["rows"].items():
            beta1, beta2 = (float(b) for b in self.param_groups[gi]["betas"])
            mine = steps[rows]
            for t in np.unique(mine):
                t = float(t)
                at = rows[mine == t]
                table["bias_correction1"][at] = 1 - beta1 ** t
                table["bias_correction2_sqrt"][at] = (1 - beta2 ** t) ** 0.5
        n, n_blocks = len(sel), plan["n_blocks"]
        table_bytes, map_bytes = n * _ENTRY.itemsize, n_blocks * 8
        host, dev, event = self._block(table_bytes + map_bytes)
        raw = host.numpy()
        raw[:table_bytes] = table.view(np.uint8)
        raw[table_bytes:table_bytes + map_bytes] = plan["map_bytes"]
        dev[:table_bytes + map_bytes].copy_(host[:table_bytes + map_bytes], non_blocking=True)
        event.record(torch.cuda.current_stream())
        _capi.call("hps_adam_step", _capi._P(dev.data_ptr()), n, _capi._P(dev.data_ptr() + table_bytes), n_blocks, _capi.stream())
        counters[plan["index"]] = steps                       # the launch is queued: now the counters move, all at once
        del grads                                             # the allocator is stream-ordered
        torch.autograd.graph.increment_version(plan["params"])
        for module in self._refresh:
            module.refresh_weights()
        return None


# ---- refresh lists (hps_weights_refresh): the builders ResNet.refresh_weights / PoseMFShapeGaussianNet.refresh_weights share ----
def plain(t):
    """``t`` is what the refresh ops can address in place: fp32 and contiguous."""
    return t.dtype == torch.float32 and t.is_contiguous()


class RefreshList:
    """The ops of one prepared state.  ``covered``: data_ptr() of every destination tensor; ``token``: what must be unchanged for the
    list to stay valid (the parameters' storage, the set of backward filters)."""

    def __init__(self, token):
        self.token, self.ops, self.covered, self.array = token, [], set(), None

    def _span(self, n, stride):
        return sum((a - 1) * s for a, s in zip(n, stride))

    def permute(self, src, dst, n, sstride, dstride, offset=0, scale=None, scale_dim=0):
        """dst.flatten()[offset + sum i_k dstride[k]] = src.flatten()[sum i_k sstride[k]] (times scale[i_scale_dim])."""
        scale_dim += 4 - len(n)
        n, sstride, dstride = ([1] * (4 - len(v)) + list(v) for v in (n, sstride, dstride))
        assert plain(src) and plain(dst) and min(n) > 0
        assert self._span(n, sstride) < src.numel() and offset + self._span(n, dstride) < dst.numel()
        assert scale is None or (plain(scale) and scale.numel() == n[scale_dim])
        op = _capi.RefreshOp(kind=_capi.REFRESH_PERMUTE, scale_dim=scale_dim, src=src.data_ptr(), dst=dst.data_ptr() + 4 * offset,
                             aux0=scale.data_ptr() if scale is not None else None)
        op.n[:], op.sstride[:], op.dstride[:] = n, sstride, dstride
        self._add(op, dst)

    def copy(self, src, dst, offset=0):
        """dst.flatten()[offset:offset + src.numel()] = src; nothing when dst IS src (prepare() aliases contiguous fp32 parameters)."""
        if dst.data_ptr() == src.data_ptr() and offset == 0:
            return
        self.permute(src, dst, (src.numel(),), (1,), (1,), offset)

    def transpose(self, src, dst, offset=0, ld=None):
        """dst (cols, ld)[:, offset:offset + rows] = src (rows, cols) transposed."""
        rows, cols = src.shape
        self.permute(src, dst, (cols, rows), (1, cols), (ld or rows, 1), offset)

    def fold(self, bn, scale, shift):
        c = scale.numel()
        ts = (bn.weight, bn.bias, bn.running_mean, bn.running_var, scale, shift)
        assert all(plain(t) and t.numel() == c for t in ts)
        op = _capi.RefreshOp(kind=_capi.REFRESH_FOLD, src=bn.weight.data_ptr(), aux0=bn.bias.data_ptr(), aux1=bn.running_mean.data_ptr(),
                             aux2=bn.running_var.data_ptr(), dst=scale.data_ptr(), dst2=shift.data_ptr(), eps=float(bn.eps))
        op.n[:] = [c, 1, 1, 1]
        self._add(op, scale)
        self.covered.add(shift.data_ptr())

    def winograd(self, w, dst, stem=False):
        cout, cin, kh, kw = w.shape
        assert plain(w) and plain(dst)
        assert (dst.numel() == 81 * 1152 + 256 and (cout, cin, kh, kw) == (64, 18, 7, 7)) if stem else \
            (dst.numel() == 16 * cin * cout and kh == kw == 3 and cout % 64 == 0 and cin % 8 == 0)
        op = _capi.RefreshOp(kind=_capi.REFRESH_STEM_U if stem else _capi.REFRESH_WINO_U, src=w.data_ptr(), dst=dst.data_ptr())
        op.n[:] = [cout, cin, kh, kw]
        self._add(op, dst)

    def _add(self, op, dst):
        self.ops.append(op)
        self.covered.add(dst.data_ptr())
        self.array = None

    def run(self):
        """On the current stream; the tensors are the module's own and live on its device."""
        if self.array is None:
            self.array = (_capi.RefreshOp * max(1, len(self.ops)))(*self.ops)
        _capi.call("hps_weights_refresh", self.array, len(self.ops), _capi.stream())
