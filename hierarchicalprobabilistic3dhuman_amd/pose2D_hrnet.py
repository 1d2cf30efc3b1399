"""HRNet 2D keypoint detector (inference forward) with the module tree and state-dict keys of the reference's
models/pose2D_hrnet.py, executed on the gfx950 fp32 matrix cores: every convolution is a problem of the grouped 16-channel kernel
(csrc/conv_c16.hip), every fuse step one launch of csrc/hrnet.hip.

The ``nn.Conv2d`` / ``nn.BatchNorm2d`` children only hold parameters, so that ``load_state_dict`` of the released
``pose_hrnet_w48_384x288.pth`` (strict) and default initialisation behave as in the reference; their own forward is never used.
Eval mode only: BatchNorm is folded once into the convolution epilogue's scale / shift (float64 arithmetic, rounded once); the final
layer, a convolution with a bias and no BatchNorm, runs with scale = 1 and shift = bias.  There is no backward: the output never
carries an autograd graph, and an input that requires grad is refused.

One plan per input shape.  ``PoseHighResolutionNet._plan`` walks the network once for a (B, H, W) and leaves the halo-padded NHWC
activation frames (zeroed once; only interiors are ever written) and the ordered launch list, an array of ``_capi.HrnetOp`` that goes
to the device as ONE ``hps_hrnet_run`` call per forward.  Convolutions that do not depend on each other share a launch, up to four per
launch: the branches of a HighResolutionModule at the same block depth, a bottleneck's first convolution and its down-sample, the
first steps of all fuse paths of a module, the first steps of a transition.  Every output has the bits it has when its convolution
is launched alone (include/hps.h: the summation order depends on the layer only).  HRNet-W48 at 384 x 288 is 131 launches (1 pack,
106 holding 293 convolutions, 23 fuse, 1 unpack).

The fuse step y_i = relu(sum_j term_ij) adds the terms in j order, as the reference does; a lower branch's 1x1 + BN output stays at
its own resolution and is read at (y >> s, x >> s): no up-sampled tensor exists.

The 3-channel stem reads what ``forward`` receives: ``hps_hrnet_pack_input`` writes the NCHW image into a 16-channel frame (13 zero
channels, part of the zero padding) and conv1 is a 16-channel problem like the rest.
"""
import torch
from torch import nn

from . import _capi
from .device_state import DeviceStateModule


def _conv(cin, cout, k, stride=1, bias=False):
    return nn.Conv2d(cin, cout, kernel_size=k, stride=stride, padding=k // 2, bias=bias)


class BasicBlock(nn.Module):
    """Two 3x3 convolutions and the identity (parameter container; executed as steps of PoseHighResolutionNet._plan)."""
    expansion = 1
    STEPS = (("conv1", "bn1"), ("conv2", "bn2"))

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1, self.bn1 = _conv(inplanes, planes, 3, stride), nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2, self.bn2 = _conv(planes, planes, 3), nn.BatchNorm2d(planes)
        self.downsample = downsample
        self.stride = stride


class Bottleneck(nn.Module):
    """1x1 reduce, 3x3, 1x1 expand (x 4) and the identity (parameter container)."""
    expansion = 4
    STEPS = (("conv1", "bn1"), ("conv2", "bn2"), ("conv3", "bn3"))

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1, self.bn1 = _conv(inplanes, planes, 1), nn.BatchNorm2d(planes)
        self.conv2, self.bn2 = _conv(planes, planes, 3, stride), nn.BatchNorm2d(planes)
        self.conv3, self.bn3 = _conv(planes, planes * 4, 1), nn.BatchNorm2d(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride


_BLOCKS = {"BASIC": BasicBlock, "BOTTLENECK": Bottleneck}


def _stack(block, inplanes, planes, count):
    """``count`` blocks, the first with a 1x1 + BN down-sample when the width changes; returns (nn.Sequential, output width)."""
    out = planes * block.expansion
    down = nn.Sequential(_conv(inplanes, out, 1), nn.BatchNorm2d(out)) if inplanes != out else None
    blocks = [block(inplanes, planes, 1, down)] + [block(out, planes) for _ in range(count - 1)]
    return nn.Sequential(*blocks), out


def _down_chain(cin, cout, steps, last_relu):
    """``steps`` 3x3 / 2 convolutions + BN; all but the last keep ``cin`` channels and carry a ReLU, the last one as ``last_relu``."""
    chain = []
    for k in range(steps):
        last = k == steps - 1
        width = cout if last else cin
        layers = [_conv(cin, width, 3, 2), nn.BatchNorm2d(width)]
        if not last or last_relu:
            layers.append(nn.ReLU(inplace=True))
        chain.append(nn.Sequential(*layers))
    return nn.Sequential(*chain)


class HighResolutionModule(nn.Module):
    """Parallel branches of blocks, then the exchange between the resolutions (parameter container)."""

    def __init__(self, num_branches, block, num_blocks, num_inchannels, num_channels, fuse_method, multi_scale_output=True):
        super().__init__()
        if not (num_branches == len(num_blocks) == len(num_channels) == len(num_inchannels)):
            raise ValueError("NUM_BRANCHES (%d) must equal the lengths of NUM_BLOCKS (%d), NUM_CHANNELS (%d) and the incoming widths (%d)"
                             % (num_branches, len(num_blocks), len(num_channels), len(num_inchannels)))
        self.num_branches, self.fuse_method, self.multi_scale_output = num_branches, fuse_method, multi_scale_output
        branches, widths = [], []
        for i in range(num_branches):
            seq, w = _stack(block, num_inchannels[i], num_channels[i], num_blocks[i])
            branches.append(seq)
            widths.append(w)
        self.num_inchannels = widths
        self.branches = nn.ModuleList(branches)
        self.fuse_layers = None
        if num_branches > 1:
            rows = []
            for i in range(num_branches if multi_scale_output else 1):
                row = []
                for j in range(num_branches):
                    if j > i:
                        row.append(nn.Sequential(_conv(widths[j], widths[i], 1), nn.BatchNorm2d(widths[i]),
                                                 nn.Upsample(scale_factor=2 ** (j - i), mode="nearest")))
                    elif j == i:
                        row.append(None)
                    else:
                        row.append(_down_chain(widths[j], widths[i], i - j, last_relu=False))
                rows.append(nn.ModuleList(row))
            self.fuse_layers = nn.ModuleList(rows)
        self.relu = nn.ReLU(True)

    def get_num_inchannels(self):
        return self.num_inchannels


class _Layer:
    """Kernel-side form of one convolution (+ eval BatchNorm or bias): the filter as hps_conv2d_bn_act_c16 reads it,
    (K * K, ceil16(Cout), ceil16(Cin)) tap-major with zero rows / channels in the padding, and the epilogue's scale / shift."""

    def __init__(self, conv, bn):
        w = conv.weight.detach().float()
        cout, cin, k, k2 = w.shape
        if k != k2 or k not in (1, 3) or conv.stride[0] not in (1, 2) or conv.padding[0] != k // 2 or conv.groups != 1:
            raise _capi.HpsError("pose2D_hrnet: only 1x1 and 3x3 convolutions with stride 1 or 2 and padding k // 2 run on the device")
        self.cin, self.cout, self.k, self.stride = cin, cout, k, conv.stride[0]
        self.cin_p, coutp = (cin + 15) // 16 * 16, (cout + 15) // 16 * 16
        wk = torch.zeros(k, k, coutp, self.cin_p, device=w.device, dtype=torch.float32)
        wk[:, :, :cout, :cin] = w.permute(2, 3, 0, 1)
        self.w = wk.reshape(k * k, coutp, self.cin_p).contiguous()
        if bn is not None:
            inv_std = torch.rsqrt(bn.running_var.detach().double() + bn.eps)
            scale = bn.weight.detach().double() * inv_std
            shift = bn.bias.detach().double() - bn.running_mean.detach().double() * scale
            if conv.bias is not None:
                shift = shift + conv.bias.detach().double() * scale
        else:
            scale = torch.ones(cout, device=w.device, dtype=torch.float64)
            shift = conv.bias.detach().double() if conv.bias is not None else torch.zeros(cout, device=w.device, dtype=torch.float64)
        # 16-byte aligned whatever Cout is: each in a buffer of its own
        self.scale, self.shift = scale.float().contiguous(), shift.float().contiguous()

    def out_hw(self, h, w):
        p = self.k // 2
        return (h + 2 * p - self.k) // self.stride + 1, (w + 2 * p - self.k) // self.stride + 1


class _Frame:
    """A halo-padded NHWC activation frame (B, h + 2 pad, w + 2 pad, c)."""
    __slots__ = ("t", "h", "w", "c", "pad")

    def __init__(self, t, h, w, c, pad):
        self.t, self.h, self.w, self.c, self.pad = t, h, w, c, pad


class _Planner:
    """Frames (a pool: a frame nothing reads any more is handed out again to a later layer of the same shape -- launches run in
    stream order, and only interiors are ever written, so the zero halo holds) and the launch list of one (B, H, W)."""

    def __init__(self, B, device):
        self.B, self.device = B, device
        self.free, self.frames, self.ops = {}, [], []

    def frame(self, h, w, c, pad=1):
        key = (h, w, c, pad)
        if self.free.get(key):
            return self.free[key].pop()
        f = _Frame(torch.zeros(self.B, h + 2 * pad, w + 2 * pad, c, device=self.device, dtype=torch.float32), h, w, c, pad)
        self.frames.append(f)
        return f

    def release(self, *frames):
        for f in frames:
            if f is not None:
                bucket = self.free.setdefault((f.h, f.w, f.c, f.pad), [])
                if not any(g is f for g in bucket):
                    bucket.append(f)

    def convs(self, jobs):
        """``jobs``: independent convolutions (layer, input frame, residual frame or None, relu[, output halo]) -> their output frames;
        up to four share a launch."""
        outs, problems = [], []
        for job in jobs:
            layer, x, res, relu = job[:4]
            opad = job[4] if len(job) > 4 else 1
            assert x.c == layer.cin_p, (x.c, layer.cin_p)
            ho, wo = layer.out_hw(x.h, x.w)
            y = self.frame(ho, wo, layer.cout, opad)
            assert res is None or (res.h, res.w, res.c, res.pad) == (ho, wo, layer.cout, opad)
            P = _capi.ptr
            problems.append(_capi.C16Problem(x=P(x.t), w=P(layer.w), scale=P(layer.scale), shift=P(layer.shift),
                                             residual=P(res.t) if res is not None else None, y=P(y.t), B=self.B, H=x.h, W=x.w, ipad=x.pad,
                                             Cin=x.c, Cout=layer.cout, K=layer.k, stride=layer.stride, opad=opad, relu=1 if relu else 0))
            outs.append(y)
        for i in range(0, len(problems), _capi.C16_MAX_PROBLEMS):
            group = problems[i:i + _capi.C16_MAX_PROBLEMS]
            op = _capi.HrnetOp(kind=_capi.HRNET_CONV, n_problems=len(group))
            for k, p in enumerate(group):
                op.conv[k] = p
            self.ops.append(op)
        return outs

    def fuse(self, terms, h, w, c):
        """``terms``: (frame, shift) in the reference's j order -> relu(sum) as a new frame."""
        y = self.frame(h, w, c)
        a = _capi.HrnetFuseArgs(n_terms=len(terms), y=_capi.ptr(y.t), opad=y.pad, B=self.B, H=h, W=w, C=c, relu=1)
        for k, (f, s) in enumerate(terms):
            assert (f.h << s, f.w << s, f.c) == (h, w, c)
            a.term[k], a.shift[k], a.pad[k] = f.t.data_ptr(), s, f.pad
        self.ops.append(_capi.HrnetOp(kind=_capi.HRNET_FUSE, fuse=a))
        return y


class PoseHighResolutionNet(DeviceStateModule):
    """models/pose2D_hrnet.py:275-461 for BASIC / BOTTLENECK blocks and FUSE_METHOD 'SUM': (B, 3, H, W) -> (B, NUM_JOINTS, H/4, W/4)."""

    def __init__(self, cfg, **kwargs):
        super().__init__()
        extra = cfg["MODEL"]["EXTRA"]
        for name in ("STAGE2", "STAGE3", "STAGE4"):
            st = extra[name]
            if st["FUSE_METHOD"] != "SUM":
                raise _capi.HpsError("pose2D_hrnet: %s.FUSE_METHOD = %r; only 'SUM' runs on the device" % (name, st["FUSE_METHOD"]))
            if st["BLOCK"] not in _BLOCKS:
                raise _capi.HpsError("pose2D_hrnet: %s.BLOCK = %r; only BASIC and BOTTLENECK run on the device" % (name, st["BLOCK"]))
            if not 1 <= st["NUM_BRANCHES"] <= _capi.HRNET_MAX_TERMS:
                raise _capi.HpsError("pose2D_hrnet: %s.NUM_BRANCHES = %r; the fuse kernel adds 1 to 4 terms" % (name, st["NUM_BRANCHES"]))
        if extra["FINAL_CONV_KERNEL"] not in (1, 3):
            raise _capi.HpsError("pose2D_hrnet: FINAL_CONV_KERNEL = %r; only 1 and 3 run on the device" % (extra["FINAL_CONV_KERNEL"],))
        self.conv1, self.bn1 = _conv(3, 64, 3, 2), nn.BatchNorm2d(64)
        self.conv2, self.bn2 = _conv(64, 64, 3, 2), nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.layer1, width = _stack(Bottleneck, 64, 64, 4)
        pre = [width]
        for n in (2, 3, 4):
            st = extra["STAGE%d" % n]
            setattr(self, "stage%d_cfg" % n, st)
            block = _BLOCKS[st["BLOCK"]]
            cur = [c * block.expansion for c in st["NUM_CHANNELS"]]
            if len(pre) > 1 and any(c != p for c, p in zip(cur, pre)):
                # the reference feeds EVERY transition layer from the last branch (:446, :454), so a layer that only changes an existing
                # branch's width receives a map of another width and resolution there: such a config does not run in the reference
                raise _capi.HpsError("pose2D_hrnet: STAGE%d.NUM_CHANNELS %r changes the width of an existing branch (%r); the reference "
                                     "feeds that transition layer from the last branch and cannot run such a config" % (n, list(cur), list(pre)))
            setattr(self, "transition%d" % (n - 1), self._transition(pre, cur))
            modules, widths = [], cur
            for m in range(st["NUM_MODULES"]):
                multi = not (n == 4 and m == st["NUM_MODULES"] - 1)        # the last module of all keeps the top resolution only
                modules.append(HighResolutionModule(st["NUM_BRANCHES"], block, st["NUM_BLOCKS"], widths, st["NUM_CHANNELS"],
                                                    st["FUSE_METHOD"], multi))
                widths = modules[-1].get_num_inchannels()
            setattr(self, "stage%d" % n, nn.Sequential(*modules))
            pre = widths
        k = extra["FINAL_CONV_KERNEL"]
        self.final_layer = _conv(pre[0], cfg["MODEL"]["NUM_JOINTS"], k, 1, bias=True)
        self.pretrained_layers = extra["PRETRAINED_LAYERS"]

    @staticmethod
    def _transition(pre, cur):
        layers = []
        for i, width in enumerate(cur):
            if i < len(pre):
                layers.append(nn.Sequential(_conv(pre[i], width, 3), nn.BatchNorm2d(width), nn.ReLU(inplace=True)) if width != pre[i] else None)
            else:
                layers.append(_down_chain(pre[-1], width, i + 1 - len(pre), last_relu=True))
        return nn.ModuleList(layers)

    def init_weights(self, pretrained=""):
        """models/pose2D_hrnet.py:463-493: N(0, 0.001) filters, zero biases, unit BatchNorm, then the named layers of ``pretrained``."""
        import os
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.normal_(m.weight, std=0.001)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        if os.path.isfile(pretrained):
            sd = torch.load(pretrained, map_location="cpu")
            keep = {k: v for k, v in sd.items() if k.split(".")[0] in self.pretrained_layers or self.pretrained_layers[0] == "*"}
            self.load_state_dict(keep, strict=False)
        elif pretrained:
            raise ValueError("{} is not exist!".format(pretrained))
        self.invalidate()

    # ---- weight preparation: redone after .to() / load_state_dict / in copies (DeviceStateModule) ----
    def prepare(self):
        """{id(conv): _Layer} for every convolution of the network, BatchNorm folded."""
        prep = {}

        def pair(conv, bn):
            prep[id(conv)] = _Layer(conv, bn)

        def seq(s):                         # Sequential(conv, bn[, relu | upsample])
            pair(s[0], s[1])

        def blocks(stack):
            for blk in stack:
                for cname, bname in blk.STEPS:
                    pair(getattr(blk, cname), getattr(blk, bname))
                if blk.downsample is not None:
                    seq(blk.downsample)

        with torch.no_grad():
            pair(self.conv1, self.bn1)
            pair(self.conv2, self.bn2)
            blocks(self.layer1)
            for n in (2, 3, 4):
                for t in getattr(self, "transition%d" % (n - 1)):
                    if t is None:
                        continue
                    if isinstance(t[0], nn.Conv2d):
                        seq(t)
                    else:
                        for step in t:
                            seq(step)
                for mod in getattr(self, "stage%d" % n):
                    for br in mod.branches:
                        blocks(br)
                    for row in (mod.fuse_layers or []):
                        for cell in row:
                            if cell is None:
                                continue
                            if isinstance(cell[0], nn.Conv2d):
                                seq(cell)
                            else:
                                for step in cell:
                                    seq(step)
            pair(self.final_layer, None)
        self._prepared = prep
        return prep

    # ---- the one walk over the network ----
    def _plan(self, prep, B, H, W, device):
        pl = _Planner(B, device)
        L = lambda conv: prep[id(conv)]

        def run_stacks(stacks, xs):
            """Block stacks side by side (the branches of a module; layer1 alone): step by step, the same step of every stack in one
            wave of launches.  Consumes xs."""
            xs = list(xs)
            depth = max(len(s) for s in stacks)
            for d in range(depth):
                live = [i for i, s in enumerate(stacks) if d < len(s)]
                blks = {i: stacks[i][d] for i in live}
                cur = {i: xs[i] for i in live}
                ident = dict(cur)
                nsteps = len(next(iter(blks.values())).STEPS)
                for s in range(nsteps):
                    last = s == nsteps - 1
                    jobs, owners = [], []
                    for i in live:
                        conv = getattr(blks[i], blks[i].STEPS[s][0])
                        jobs.append((L(conv), cur[i], ident[i] if last else None, True))
                        owners.append((i, "main"))
                        if s == 0 and blks[i].downsample is not None:
                            jobs.append((L(blks[i].downsample[0]), xs[i], None, False))
                            owners.append((i, "down"))
                    outs = pl.convs(jobs)
                    for (i, what), y in zip(owners, outs):
                        if what == "down":
                            ident[i] = y
                        else:
                            if cur[i] is not xs[i]:
                                pl.release(cur[i])
                            cur[i] = y
                for i in live:
                    if ident[i] is not xs[i]:
                        pl.release(ident[i])
                    pl.release(xs[i])
                    xs[i] = cur[i]
            return xs

        def chain(steps, x):
            """([(layer, relu), ...], x): the convolutions of ``steps`` to run one after the other from frame x (run_chains)."""
            return [(L(s[0]), isinstance(s[-1], nn.ReLU)) for s in steps], x

        def run_chains(chains):
            """Chains of convolutions side by side, step k of every chain in one wave; returns the last frame of each.  The chains'
            inputs are not consumed."""
            state = [x for _, x in chains]
            depth = max(len(st) for st, _ in chains) if chains else 0
            for k in range(depth):
                idx = [c for c, (st, _) in enumerate(chains) if k < len(st)]
                outs = pl.convs([(chains[c][0][k][0], state[c], None, chains[c][0][k][1]) for c in idx])
                for c, y in zip(idx, outs):
                    if state[c] is not chains[c][1]:
                        pl.release(state[c])
                    state[c] = y
            return state

        # stem
        x_in = pl.frame(H, W, 16)
        pl.ops.append(_capi.HrnetOp(kind=_capi.HRNET_PACK, x=None, y=_capi.ptr(x_in.t), B=B, H=H, W=W, C=16, P=1))
        s1, = pl.convs([(L(self.conv1), x_in, None, True)])
        s2, = pl.convs([(L(self.conv2), s1, None, True)])
        pl.release(s1)
        ys = run_stacks([list(self.layer1)], [s2])
        for n in (2, 3, 4):
            trans = getattr(self, "transition%d" % (n - 1))
            chains, slots = [], []
            for i, t in enumerate(trans):
                if t is None:
                    continue
                src = ys[-1]                      # every transition layer reads the last branch (models/pose2D_hrnet.py:438, :446, :454)
                chains.append(chain([t] if isinstance(t[0], nn.Conv2d) else list(t), src))
                slots.append(i)
            made = dict(zip(slots, run_chains(chains)))
            xs = [made[i] if i in made else ys[i] for i in range(len(trans))]
            pl.release(*[y for y in ys if not any(y is x for x in xs)])
            for mod in getattr(self, "stage%d" % n):
                xs = run_stacks([list(br) for br in mod.branches], xs)
                if mod.fuse_layers is None:
                    continue
                chains, where = [], []
                for i, row in enumerate(mod.fuse_layers):
                    for j, cell in enumerate(row):
                        if cell is None:
                            continue
                        chains.append(chain([cell] if isinstance(cell[0], nn.Conv2d) else list(cell), xs[j]))
                        where.append((i, j))
                terms = dict(zip(where, run_chains(chains)))
                fused = []
                for i, row in enumerate(mod.fuse_layers):
                    tl = [(xs[j], 0) if j == i else (terms[(i, j)], max(j - i, 0)) for j in range(len(row))]
                    fused.append(pl.fuse(tl, xs[i].h, xs[i].w, xs[i].c))
                pl.release(*terms.values())
                pl.release(*xs)
                xs = fused
            ys = xs
        heat, = pl.convs([(L(self.final_layer), ys[0], None, False, 0)])
        pl.ops.append(_capi.HrnetOp(kind=_capi.HRNET_UNPACK, x=_capi.ptr(heat.t), y=None, B=B, H=heat.h, W=heat.w, C=heat.c, P=0))
        ops = (_capi.HrnetOp * len(pl.ops))(*pl.ops)
        return {"frames": pl.frames, "ops": ops, "out": (B, heat.c, heat.h, heat.w)}

    def launches_per_forward(self, B, H, W, device):
        """The number of kernel launches of one forward on a (B, 3, H, W) input."""
        return len(self._frame_set(self._prepared or self.prepare(), B, H, W, device)["ops"])

    def _frame_set(self, prep, B, H, W, device):
        key = (B, H, W, _capi.stream().value)
        return self._derived("frames", key, lambda: self._plan(prep, B, H, W, device), limit=4)

    def forward(self, x):
        if self.training:
            raise RuntimeError("the MI355X HRNet path runs eval-mode BatchNorm only (running statistics); call .eval() -- "
                               "training-mode BatchNorm and the backward pass are not implemented for pose2D_hrnet")
        if isinstance(x, torch.Tensor) and x.requires_grad:
            raise RuntimeError("pose2D_hrnet has no backward pass on the device: the input requires grad; detach it")
        _capi.require_device(x, "HRNet input")
        if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] % 32 != 0 or x.shape[3] % 32 != 0 or x.shape[2] == 0 or x.shape[3] == 0:
            raise _capi.HpsError("HRNet input must be (B, 3, H, W) with H and W multiples of 32, got %s" % (tuple(x.shape),))
        x = _capi.f32c(x.detach())
        B, _, H, W = x.shape
        prep = self._prepared or self.prepare()
        fs = self._frame_set(prep, B, H, W, x.device)
        out = torch.empty(fs["out"], device=x.device, dtype=torch.float32)
        if B == 0:
            return out
        ops = fs["ops"]
        ops[0].x = x.data_ptr()
        ops[len(ops) - 1].y = out.data_ptr()
        _capi.call("hps_hrnet_run", ops, len(ops), _capi.stream())
        return out


def get_pose_net(cfg, is_train, **kwargs):
    """models/pose2D_hrnet.py:496-502."""
    model = PoseHighResolutionNet(cfg, **kwargs)
    if is_train and cfg["MODEL"].get("INIT_WEIGHTS", False):
        model.init_weights(cfg["MODEL"]["PRETRAINED"])
    return model
