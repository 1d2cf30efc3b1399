"""ResNet-18 / ResNet-50 image encoder (final FC removed) with the module tree and state-dict keys of the reference's
models/resnet.py, executed as implicit-GEMM convolutions on the gfx950 fp32 matrix cores.

The ``nn.Conv2d`` / ``nn.BatchNorm2d`` children only hold parameters (so that
``load_state_dict(checkpoint['best_model_state_dict'])`` and default initialisation behave exactly as in
the reference); their own forward is never used.  By default BatchNorm uses running statistics
(the reference runs the encoder under ``model.eval()``, predict/...:55) and is fused, together with the
residual add and ReLU, into the convolution epilogue; ``.train()`` is refused unless ``set_batchnorm_training(True)`` opted in.

One plan for every forward.  ``ResNet._plan`` is the only walk over the network in the forward direction: for a frame set it returns
the ordered steps, each one launch as a ``_capi.EncOp`` (``_ConvBN.op`` is the only place that picks a convolution's kernel: Winograd
or direct, row mode, split K, tile) or, behind the convolution of a training-mode layer, a ``_BNStep``.  The eval list is the frame
set's ``ops`` array and goes to the device as one ``hps_encoder_run`` call, or -- ``composite = False``, the tests' cross-check of
csrc/composite.hip -- op by op through the public entry points (``_capi.run_enc_ops``); the training forward issues its cached list
step by step.  ``_ConvBN.padded`` / ``padded_with_down`` build the same op and issue it alone.

Fine-tuning with frozen statistics.  With grad mode on and the input or an encoder parameter requiring grad, ``ResNet.forward`` runs
inside a torch.autograd.Function: its forward issues exactly the launches of a no_grad call (same bits, in every kernel mode) and
saves only the input and the parameters.  The backward (csrc/conv_backward.hip) evaluates the encoder once more into a frame set of
its own -- the activation frames belong to the module and the next forward overwrites them, and the fused stem never writes the
full-resolution map the max pool's backward needs -- with the forward's kernel family per layer and only the bit-identical fusions
switched off, so the ReLU masks and pool winners are those of the function the caller evaluated.  This alone is NOT the reference's
``model.train()`` step.

Training-mode BatchNorm (``ResNet.set_batchnorm_training``, opt-in; csrc/bn_train.hip).  A BatchNorm whose own ``.training`` is set
runs as ``nn.BatchNorm2d`` does in training mode: its convolution writes the raw map, the batch mean and biased variance are reduced
in float64 in a fixed order, one fold launch turns them into the epilogue's scale / shift and updates running_mean / running_var /
num_batches_tracked on the device, and the epilogue runs as a pass of its own.  The autograd function saves each such layer's mean
and inverse standard deviation (two float64 vectors); the backward's recompute applies them and the backward goes through the
statistics.  Bitwise repeatable; a training layer's output depends on the whole batch, so the independence of an image's result from
the batch size holds for eval layers only.  From the first differentiable forward on
the module compares its parameters' ``_version`` counters with those recorded by ``prepare()`` and refolds the filters after an
optimiser step, as PoseMFShapeGaussianNet does for the head.

The Bottleneck (ResNet-50) encoder takes all of this after ``ResNet.set_differentiable(True)`` and nothing of it before: the backward
walks a block's convolutions from the last to the first (``_backward``), and the two gradients of its 1x1 layers run as LDS-tiled GEMMs
(csrc/conv1x1_backward.hip, ``gemm_backward``) where ``_gemm_dgrad`` / ``_gemm_wgrad`` send them.
"""
import collections

import torch
from torch import nn

from . import _capi
from .device_optim import RefreshList, plain
from .device_state import DeviceStateModule


class _ConvBN:
    """Kernel-side form of conv + eval BatchNorm: k-major filter (ceil16(KH*KW*Cin_p), Cout), scale, shift."""

    def __init__(self, conv, bn, cin_pad=None):
        w = conv.weight.detach().float()                      # (Cout, Cin, KH, KW)
        cout, cin, kh, kw = w.shape
        cin_p = cin if cin_pad is None else cin_pad
        wk = torch.zeros(kh, kw, cin_p, cout, device=w.device, dtype=torch.float32)
        wk[:, :, :cin, :] = w.permute(2, 3, 1, 0)
        k_real = kh * kw * cin_p
        k_pad = (k_real + 15) // 16 * 16
        flat = torch.zeros(k_pad, cout, device=w.device, dtype=torch.float32)
        flat[:k_real] = wk.reshape(k_real, cout)
        self.wk = flat.contiguous()
        self.scale, self.shift = self.fold(bn)
        # identity pair: a training-mode BatchNorm's convolution writes the exact accumulator (every epilogue is a scale + shift + res)
        self.ident = (torch.ones(cout, device=w.device, dtype=torch.float32), torch.zeros(cout, device=w.device, dtype=torch.float32))
        self.cin_p, self.cout, self.kh, self.kw = cin_p, cout, kh, kw
        self.stride, self.pad = conv.stride[0], conv.padding[0]
        # n-major filter (Cout, KH*KW*Cin) for the v2 kernel (Cin % 32 == 0: every conv after the stem)
        self.wn = wk.reshape(k_real, cout).t().contiguous() if cin_p % 32 == 0 else None
        # row-mode filter (Cout, KH * ceil32(KW*Cin)) for the halo-padded kernel when Cin % 32 != 0 (the stem): one
        # filter row of a window is KW*Cin contiguous NHWC floats, treated as one tap; the tail of each row is zero
        # Channels per pixel of a row-mode frame (row_c >= cin, the extra channels are zero = part of the zero padding): the
        # kernel's LDS-DMA windows start at multiples of stride * row_c floats and a window is ceil32(kw * row_c) floats long, so
        # row_c must be even (16-byte window starts on frames of even width) and the window's zero-weight tail must fit into
        # the one pixel of slack an even frame width leaves behind the last window.  18 (the proxy representation) qualifies as
        # it is; any other count rounds up to a multiple of 4, which always does.
        self.cin = cin
        self.wrow = None
        self.row_c = cin
        if cin % 32 != 0:
            fits = lambda c: c % 2 == 0 and (kw * c + 31) // 32 * 32 - kw * c <= c
            rc = cin if fits(cin) else (cin + 3) // 4 * 4
            self.row_c = rc
            ck = (kw * rc + 31) // 32 * 32
            wr = torch.zeros(cout, kh, kw, rc, device=w.device, dtype=torch.float32)
            wr[:, :, :, :cin] = w.permute(0, 2, 3, 1)
            wrow = torch.zeros(cout, kh, ck, device=w.device, dtype=torch.float32)
            wrow[:, :, :kw * rc] = wr.reshape(cout, kh, kw * rc)
            self.wrow = wrow.reshape(cout, kh * ck).contiguous()
        # Winograd F(2x2, 3x3) form of a stride-1 3x3 layer (csrc/conv_wino.hip): U = G g G^T in the kernel's layout
        #   [cin / 8][cout / 64][position 4a + b][(cin % 8) / 4][cout % 64][cin % 4]
        self.wino_u = None
        if kh == 3 and kw == 3 and self.stride == 1 and self.pad == 1 and cin % 8 == 0 and cout % 64 == 0:
            G = torch.tensor([[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]], dtype=torch.float64, device=w.device)
            U = torch.einsum("ai,ocij,bj->abco", G, w.double(), G)                       # (4,4,cin,cout)
            U = U.reshape(16, cin // 8, 2, 4, cout // 64, 64)                            # p, chunk, kq, j, ct, n
            self.wino_u = U.permute(1, 4, 0, 2, 5, 3).contiguous().float()              # chunk, ct, p, kq, n, j
        # Winograd form of the stem (csrc/stem_wino.hip): the 7x7 / 2 correlation as four stride-1 phase correlations, each
        # F(2x2, r x s); U = G_y g G_x^T per phase in the kernel's layout (include/hps.h: hps_stem_winograd)
        self.stem_u = None
        if kh == 7 and kw == 7 and self.stride == 2 and self.pad == 3 and cin == 18 and cout == 64:
            self.stem_u = _stem_winograd_filters(w).to(w.device).contiguous()
        self.use_winograd = True
        self.latency = False      # ResNet.set_latency_mode: direct kernels with many K slices (see _auto_ksplit)
        self.variant = 0          # tile choice of the v2 / v3 kernels (0 = automatic)
        self.ksplit = 0           # split-K slices of the v3 kernel (0 = automatic, 1 = off)
        self.zeros = torch.zeros(64, device=w.device, dtype=torch.float32)

    @staticmethod
    def fold(bn):
        """Eval-mode BatchNorm as fp32 (scale, shift): float64 arithmetic on the running statistics, rounded once."""
        inv_std = torch.rsqrt(bn.running_var.detach().double() + bn.eps)
        scale = bn.weight.detach().double() * inv_std
        return scale.float().contiguous(), (bn.bias.detach().double() - bn.running_mean.detach().double() * scale).float().contiguous()

    def refold(self, bn):
        """The fold again IN PLACE (the launch lists keep pointing at these tensors): after a training forward moved the statistics."""
        scale, shift = self.fold(bn)
        self.scale.copy_(scale)
        self.shift.copy_(shift)

    def _auto_ksplit(self, pixels_per_image):
        """Split K (4 slices) for the late layers whose 128x128 output tiles cannot fill 256 CUs at the benchmark batch
        (8x8 outputs: layer4).  The rule depends on the layer only, never on the batch size: the summation order of a
        pixel must not change with B, otherwise per-image results (and, through accept decisions that sit on rounding
        ties, whole sample streams) would depend on how images are batched or sharded over GPUs."""
        chunks = self.kh * self.kw * self.cin_p // 32
        if self.latency:
            # latency mode (ResNet.set_latency_mode): a single image leaves the 3x3 layers of layer2-4 with 4-16 output tiles, each a
            # serial walk over 36-144 K chunks; 12-18 slices of 3-8 chunks put 50-300 workgroups on the chip instead (batch 1,
            # tools/latency_sweep.py: layer2 27 -> 18 us, layer3 50 -> 20, layer4 97 -> 27 including the slice-sum pass).  Still a
            # rule on the layer alone.
            if self.kh * self.kw == 1 or pixels_per_image > 1024 or chunks < 36:
                return 1
            for ks in (18, 12, 9, 8, 6, 4, 3, 2):
                if chunks % ks == 0 and chunks // ks >= 3:
                    return ks
            return 1
        if self.variant == 0 and self.cout % 128 == 0 and self.kh * self.kw > 1 and pixels_per_image <= 64 \
                and chunks % 4 == 0 and chunks // 4 >= 18:
            return 4
        return 1

    def _tile_variant(self, ksplit):
        """Tile choice handed to hps_conv2d_bn_act_pad.  Latency mode: 64 x 64 tiles with a four-stage K loop for every layer (variant
        5), split-K layers included -- a single image's maps leave 128-row tiles half empty and a quarter as many workgroups on the
        chip; an output's summation order does not depend on the tile shape, so the mode's bits are those of the 128-row tiles."""
        if self.latency and self.variant == 0:
            return 5
        return self.variant if ksplit <= 1 else 0

    def winograd_ok(self, H, W, ipad):
        """Winograd F(2x2, 3x3) applies: a 3x3 / 1 / 1 layer on a map that splits into 16 x 16-pixel blocks (8 x 8 tiles, one
        work item of csrc/conv_wino.hip) or on 8 x 8 maps (layer4: four images per item, K in slices) -- a rule on the layer
        and the image size only, never on the batch size (the summation order of a pixel, and with it the last bit of every
        feature, must not depend on how images are batched or sharded)."""
        return self.use_winograd and self.wino_u is not None and ipad >= 1 and \
            ((H % 16 == 0 and W % 16 == 0) or (H == 8 and W == 8))

    def stem_winograd_ok(self, C, H, W):
        """The Winograd form of the stem (csrc/stem_wino.hip) applies: the released model's conv1 (7x7 / 2 / 3, 18 -> 64) on maps
        that split into 32 x 32-pixel input blocks -- a rule on the layer and the image size only (see winograd_ok)."""
        return self.use_winograd and self.stem_u is not None and C == 18 and H % 32 == 0 and W % 32 == 0

    def wino_workspace_bytes(self, B, H, W, ipad=1):
        """Bytes of the K-slice buffer hps_conv3x3_winograd needs for this layer on (H, W) maps (0: none / not Winograd)."""
        if not self.winograd_ok(H, W, ipad):
            return 0
        return int(_capi.load(dev=_capi._use_dev).hps_conv3x3_winograd_workspace(B, H, W, self.cin_p, self.cout))

    def _route(self, B, H, W, ipad, down=None):
        """(op kind, split-K slices, scratch bytes) of this layer's launch on (B, H, W) maps with an ``ipad`` halo, ``down`` riding in it:
        Winograd or the direct kernel, row mode, the K slices.  The one place that decides; op() and the frame sets' scratch follow it."""
        if down is not None:
            assert self.folds_down(down, H, W, ipad)
        elif self.winograd_ok(H, W, ipad):
            return _capi.ENC_CONV_WINOGRAD, 1, self.wino_workspace_bytes(B, H, W, ipad)
        Ho, Wo = self.out_hw(H, W)
        ksplit = 1 if self.wn is None else (self.ksplit if self.ksplit > 0 else self._auto_ksplit(Ho * Wo))
        return (_capi.ENC_CONV if down is None else _capi.ENC_CONV_DOWN, ksplit,
                _capi.query_workspace(_capi.WS_CONV_SPLITK, ksplit, B * Ho * Wo, self.cout))

    def workspace_bytes(self, B, H, W, ipad=1, down=None):
        """Bytes of scratch this layer's launch needs on (B, H, W) maps: split-K slices or the Winograd kernel's K-slice buffer (0: none)."""
        return self._route(B, H, W, ipad, down)[2]

    def op(self, xp, ipad, out, opad, residual=None, relu=True, ws=None, ident=False, down=None, out_down=None, ident_down=False):
        """This layer on these frames as ONE hps_enc_op; nothing is launched.  Halo-padded generation (csrc/conv_pad.hip, conv_wino.hip):
        xp (B, H+2*ipad, W+2*ipad, Cin) with a zero halo; the launch writes the interior of ``out`` (B, Ho+2*opad, Wo+2*opad, Cout) --
        the caller owns the halo (zeroed once); ``residual`` has out's frame; ``ws`` holds workspace_bytes().  ``ident``: identity
        scale / shift instead of the folded BatchNorm (the raw map of a training-mode layer).  ``down`` (see folds_down): the block's
        1x1 down-sample writes ``out_down`` (no ReLU) in the same launch, ``ident_down`` as ident; identical bits."""
        B, Hp, Wp, C = xp.shape
        H, W = Hp - 2 * ipad, Wp - 2 * ipad
        kind, ksplit, need = self._route(B, H, W, ipad, down)
        wino, row_mode = kind == _capi.ENC_CONV_WINOGRAD, self.wn is None
        Ho, Wo = self.out_hw(H, W)
        assert C == (self.row_c if row_mode else self.cin_p) and tuple(out.shape) == (B, Ho + 2 * opad, Wo + 2 * opad, self.cout)
        assert need == 0 or (ws is not None and ws.numel() * 4 >= need)
        P = _capi.ptr
        scale, shift = self.ident if ident else (self.scale, self.shift)
        op = _capi.EncOp(kind=kind, x=P(xp), w=P(self.wino_u if wino else self.wrow if row_mode else self.wn), scale=P(scale), shift=P(shift),
                         residual=P(residual), y=P(out), splitk_ws=P(ws) if need else None, B=B, H=H, W=W, ipad=ipad, Cin=C, Cout=self.cout,
                         KH=self.kh, KW=self.kw, stride=self.stride, pad=self.pad, opad=opad, relu=1 if relu else 0,
                         row_mode=1 if row_mode else 0, variant=0 if wino else self._tile_variant(ksplit), ksplit=ksplit)
        if down is not None:
            assert residual is None and out_down.shape == out.shape
            scale, shift = down.ident if ident_down else (down.scale, down.shift)
            op.w_down, op.scale_down, op.shift_down, op.y_down = P(down.wn), P(scale), P(shift), P(out_down)
        return op

    def _scratch(self, xp, ipad, ws, down=None):
        """``ws`` where it holds what the launch on ``xp`` needs, else a buffer of its own (None: none needed)."""
        need = self.workspace_bytes(xp.shape[0], xp.shape[1] - 2 * ipad, xp.shape[2] - 2 * ipad, ipad, down)
        if need == 0 or (ws is not None and ws.numel() * 4 >= need):
            return ws
        return torch.empty(need // 4, device=xp.device, dtype=torch.float32)

    def padded(self, xp, ipad, out, opad, residual=None, relu=True, ws=None, ident=False):
        """Launch op(...) through its own entry point, with scratch of its own when the caller gave none (or too little)."""
        _capi.issue_enc_op(self.op(xp, ipad, out, opad, residual, relu, self._scratch(xp, ipad, ws), ident))
        return out

    def folds_down(self, down, H, W, ipad):
        """This (a block's first convolution) can carry the block's 1x1 down-sample ``down`` in its own launch
        (hps_conv2d_bn_act_pad_down): direct kernel, odd square filter with pad = k // 2 (its centre tap is the 1x1 / stride / 0
        window), same stride and output channels -- a rule on the layer only."""
        return (down is not None and self.wn is not None and down.wn is not None and not self.winograd_ok(H, W, ipad)
                and self.kh == self.kw and self.kh % 2 == 1 and self.pad == self.kh // 2 and down.kh == down.kw == 1 and down.pad == 0
                and down.stride == self.stride and down.cout == self.cout and down.cin_p == self.cin_p and self.cout >= 128)

    def padded_with_down(self, xp, ipad, out, opad, down, out_down, ws=None, relu=True, ident=(False, False)):
        """padded(xp -> out, relu) and down.padded(xp -> out_down, no relu) in ONE launch (see folds_down); identical bits.
        ``ident``: identity scale / shift for (this convolution, the down-sample) -- see op."""
        _capi.issue_enc_op(self.op(xp, ipad, out, opad, None, relu, self._scratch(xp, ipad, ws, down), ident[0], down, out_down, ident[1]))
        return out, out_down

    def expands_with(self, down, B, H, W):
        """This (a Bottleneck's conv3: 1x1 / 1) can take the block's down-sample ``down`` (1x1 / s on the block's (H, W) input) into its
        own launch (hps_bottleneck_expand_down): two direct 1x1 / pad 0 layers with the same output channels, neither split over K --
        a rule on the layers only."""
        if down is None or self.wn is None or down.wn is None or down.cout != self.cout:
            return False
        if not (self.kh == self.kw == down.kh == down.kw == 1 and self.pad == down.pad == 0 and self.stride == 1 and down.stride in (1, 2)):
            return False
        Ho, Wo = down.out_hw(H, W)
        return self._route(B, Ho, Wo, 1)[1] == 1 and down._route(B, H, W, 1)[1] == 1

    def expand_down_op(self, t, tpad, x, xpad, down, out, opad):
        """relu(this layer on ``t`` + ``down`` on the block's input ``x``) as ONE hps_enc_op (see expands_with); the bits of down.op(x -> d,
        no ReLU) followed by self.op(t -> out, residual = d, ReLU).  Nothing is launched."""
        B, Hp, Wp, C = x.shape
        H, W = Hp - 2 * xpad, Wp - 2 * xpad
        Ho, Wo = down.out_hw(H, W)
        assert self.expands_with(down, B, H, W) and C == down.cin_p
        assert tuple(t.shape) == (B, Ho + 2 * tpad, Wo + 2 * tpad, self.cin_p) and tuple(out.shape) == (B, Ho + 2 * opad, Wo + 2 * opad, self.cout)
        P = _capi.ptr
        return _capi.EncOp(kind=_capi.ENC_EXPAND_DOWN, x=P(t), w=P(self.wn), scale=P(self.scale), shift=P(self.shift), y=P(out),
                           x_down=P(x), w_down=P(down.wn), scale_down=P(down.scale), shift_down=P(down.shift), B=B, H=H, W=W,
                           stride=down.stride, ipad=tpad, ipad_down=xpad, opad=opad, Cin=self.cin_p, Cin_down=C, Cout=self.cout, KH=1, KW=1,
                           relu=1, variant=self._tile_variant(1), ksplit=1)

    def out_hw(self, H, W):
        return (H + 2 * self.pad - self.kh) // self.stride + 1, (W + 2 * self.pad - self.kw) // self.stride + 1


_STEM_G4 = [[0.5, 0, 0, 0], [-0.5, -0.5, -0.5, -0.5], [-1 / 6, 1 / 6, -1 / 6, 1 / 6], [1 / 6, 1 / 3, 2 / 3, 4 / 3], [0, 0, 0, 1]]
_STEM_G3 = [[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]]


def _stem_winograd_filters(w):
    """w (64, 18, 7, 7) -> the 81 transformed filter positions of csrc/stem_wino.hip, fp64 arithmetic rounded once to fp32.
    Phase (ry, rx) holds the taps w[:, :, ry::2, rx::2] (4 or 3 per axis); positions are ordered phase 2 ry + rx, row i, column j;
    one position is 1152 floats: [co / 32][k-block (c % 16) / 8][c % 2][co % 32][(c % 8) / 2] for c < 16, then c = 16, 17 as
    [c - 16][co % 32] behind them.  256 floats of slack follow (the last DMA piece of a row of positions over-reads)."""
    w = w.detach().double().cpu()
    pos = []
    for ry in (0, 1):
        for rx in (0, 1):
            gy = torch.tensor(_STEM_G4 if ry == 0 else _STEM_G3, dtype=torch.float64)
            gx = torch.tensor(_STEM_G4 if rx == 0 else _STEM_G3, dtype=torch.float64)
            u = torch.einsum("ia,ocab,jb->ijco", gy, w[:, :, ry::2, rx::2], gx)          # (ny, nx, 18, 64)
            pos.append(u.reshape(-1, 18, 64))
    u = torch.cat(pos, 0)                                                                # (81, c, co)
    lo = u[:, :16].reshape(81, 2, 4, 2, 2, 32)                                           # p, kblock, e, parity, co half, co % 32   (c = 8 kb + 2 e + parity)
    lo = lo.permute(0, 4, 1, 3, 5, 2).reshape(81, 2, 512)                                # p, half, [kb][parity][co % 32][e]
    hi = u[:, 16:].reshape(81, 2, 2, 32).permute(0, 2, 1, 3).reshape(81, 2, 64)          # p, half, [c - 16][co % 32]
    packed = torch.cat([lo, hi], 2).reshape(-1)
    return torch.cat([packed, torch.zeros(256, dtype=torch.float64)]).float()


# A training-mode BatchNorm behind its layer's convolution (ResNet._plan): the raw frame -> batch statistics -> fold -> out = act(raw
# scale + shift [+ residual]) on (h, w) maps inside a ``pad`` halo (csrc/bn_train.hip)
_BNStep = collections.namedtuple("_BNStep", "name channels raw out residual relu h w pad")


class FilledStemFrames:
    """Marker returned by ResNet.stem_frames(): the encoder's own phase frames for a (B, C, H, W) input on the current stream have
    been (or are about to be, on that stream) filled by the caller -- hps_proxy_rep_phase_frames -- instead of by
    hps_stem_phase_split from an NCHW tensor.  ``ResNet.forward(filled)`` then starts at the stem convolution."""

    def __init__(self, frames, shape, device, fill=None, owner=None, generation=0):
        self.frames, self.shape, self.device = frames, tuple(shape), device
        self.is_cuda = True
        # the frame buffer is ONE per (shape, stream) and belongs to the encoder: this object is good for exactly one forward, the next
        # stem_frames() / phase split on the same buffer bumps the owner's generation and forward() refuses a stale object
        self.owner, self.generation = owner, generation
        # ``fill``: the launch that writes the frames, deferred to forward() -- issued right in front of the stem convolution, where
        # hps_stem_phase_split would have run: the stem then reads frames that were just written (L2 / Infinity Cache), not frames
        # written before the previous batch's mesh kernel streamed 540 MB through the caches (measured: filling them early made the
        # stem 0.2 ms slower and lost more than the skipped phase split gained)
        self.fill = fill

    def run_fill(self):
        if self.fill is not None:
            fill, self.fill = self.fill, None
            fill()

    def record_stream(self, stream):            # the frames belong to the encoder (allocated once per shape and stream)
        pass


class _EncoderFunction(torch.autograd.Function):
    """ResNet.forward for autograd: forward = the module's own launches (the bits of a no_grad call), saving only the input and the
    parameters; backward = the recompute and the device backward kernels (ResNet._backward), without the kernels whose result
    ``ctx.needs_input_grad`` does not ask for.  Inputs after ``x``: the parameters in the order of ``ResNet._enc_params()``."""

    @staticmethod
    def forward(ctx, net, prep, gate, flags, x, *params):
        xc = _capi.f32c(x.detach())
        ctx.flags, saved = flags, []
        if flags is not None:                                            # some BatchNorm runs on batch statistics
            B, C, H, W = xc.shape
            feats, stats = net._forward_train(prep, xc, net._train_frames(prep, B, C, H, W, xc.device, flags), flags, update=True)
            ctx.stat_names = list(stats)
            saved = [t for name in ctx.stat_names for t in (stats[name][0], stats[name][2])]      # mean, invstd: (C,) float64 each
        else:
            feats = net._forward_padded(prep, xc, gate=gate)
        ctx.net, ctx.prep, ctx.x_dtype = net, prep, x.dtype             # prep owns the folded filters the recompute reads
        ctx.n_params = len(params)
        ctx.save_for_backward(xc, *params, *saved)
        return feats

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_feats):
        x = ctx.saved_tensors[0]
        need = ctx.needs_input_grad
        saved = None
        if ctx.flags is not None:
            st = ctx.saved_tensors[1 + ctx.n_params:]
            saved = {name: (st[2 * i], st[2 * i + 1]) for i, name in enumerate(ctx.stat_names)}
        g_x, g_params = ctx.net._backward(ctx.prep, x, g_feats, list(need[4:]), flags=ctx.flags, saved=saved)
        if g_x is not None and g_x.dtype != ctx.x_dtype:
            g_x = g_x.to(ctx.x_dtype)
        return (None, None, None, None, g_x) + tuple(g_params)


class BasicBlock(nn.Module):
    """models/resnet.py:40-78 (parameter container; executed as the steps of ResNet._plan)."""
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, kernel_size=3, stride=stride, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, stride=1, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = downsample
        self.stride = stride


class Bottleneck(nn.Module):
    """models/resnet.py:81-122 (parameter container; executed as the steps of ResNet._plan).  The 3x3 convolution carries the block's
    stride (:91-97)."""
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, kernel_size=1, stride=1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * self.expansion, kernel_size=1, stride=1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * self.expansion)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride


def _block_convs(blk):
    """[(suffix, conv, bn)] of a block's main branch in execution order: c1, c2 (BasicBlock) or c1, c2, c3 (Bottleneck)."""
    n = 3 if isinstance(blk, Bottleneck) else 2
    return [("c%d" % i, getattr(blk, "conv%d" % i), getattr(blk, "bn%d" % i)) for i in range(1, n + 1)]


class _Block(tuple):
    """A residual block on the kernel side: the tuple (c1, c2, down) of a BasicBlock or (c1, c2, c3, down) of a Bottleneck -- ``convs``,
    the main branch's _ConvBN in execution order, then ``down``, the down-sample on the block's input or None."""

    def __new__(cls, convs, down):
        return super().__new__(cls, tuple(convs) + (down,))

    convs = property(lambda self: list(self[:-1]))
    down = property(lambda self: self[-1])


class ResNet(DeviceStateModule):
    """models/resnet.py:125-217 for BasicBlock and Bottleneck stacks.  A freshly built Bottleneck encoder runs forward only (eval-mode
    BatchNorm, no_grad): a differentiable forward, training-mode BatchNorm and the in-place weight refresh are refused, never computed
    wrongly.  ``set_differentiable(True)`` opts such an encoder in to what the ResNet-18 encoder does: the differentiable forward
    (_EncoderFunction, the block walk of _backward, the 1x1 GEMM kernels of csrc/conv1x1_backward.hip), set_batchnorm_training(True)
    and then ``.train()``, refresh_weights() in place, the training loop.  A BasicBlock encoder is always differentiable."""

    SWITCHES = ("_winograd", "_latency", "composite", "fused_pool", "fold_downsample", "stem_reads_nchw", "_bn_training")
    # (``_differentiable`` and ``gemm_backward`` change no forward launch and nothing the device state holds: no SWITCHES entry)

    def __init__(self, layers, in_channels, block=BasicBlock):
        super().__init__()
        self.block = block
        self.inplanes = 64
        self.conv1 = nn.Conv2d(in_channels, 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.layer1 = self._make_layer(64, layers[0])
        self.layer2 = self._make_layer(128, layers[1], stride=2)
        self.layer3 = self._make_layer(256, layers[2], stride=2)
        self.layer4 = self._make_layer(512, layers[3], stride=2)
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        # same initialisation, in the same module order, as models/resnet.py:161-166
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        # kernel-selection modes are properties of the MODEL (set_winograd / set_latency_mode) and survive .to() / load_state_dict:
        # prepare() re-applies them to the rebuilt _ConvBN objects
        self._winograd = True
        self._latency = False
        self._bn_training = False      # set_batchnorm_training: BatchNorm layers whose own .training is set run on batch statistics
        self.composite = True     # padded layout: issue the launch list through hps_encoder_run (one call) instead of one by one
        # Winograd stem: form the max pool in the stem kernel's epilogue (hps_stem_winograd_pooled: the full-resolution stem output is never
        # written; identical values).  False: hps_stem_winograd + hps_maxpool3x3s2_pad (the cross-check of the tests)
        self.fused_pool = True
        # the 1x1 / 2 down-sample of layer2-4's first block rides in the launch of the block's 3x3 / 2 convolution (hps_conv2d_bn_act_pad_down:
        # three launches of 16-26 us at 0.24-0.32 MFMA-busy disappear; identical bits).  False: two launches per block (the cross-check of the tests)
        # Bottleneck entry blocks (layer1-4): the 1x1 / s down-sample is formed inside the launch of the block's expand convolution, whose
        # epilogue is its only reader (hps_bottleneck_expand_down: the identity's frame is neither written nor read; identical bits)
        self.fold_downsample = True
        # ... and gather its phase windows from the NCHW input itself (hps_stem_winograd_pooled_nchw: no hps_stem_phase_split, no phase frames;
        # identical values; needs fused_pool): phase split 0.118 + frame-fed stem 0.61 -> 0.67 ms.  The default since round 6.  In round 5
        # it was off: the persistent stem as the encoder's first kernel raced the previous batch's joint / uncertainty kernels on the
        # caller's stream for the CUs, and lost or won 3-7 % of the step with the bench's event records; InferencePipeline.inline_side now
        # queues those kernels in stream order behind the mesh kernel (no race: the rate is the same with and without the markers,
        # profiles/r06_ab.txt).  False = phase split + frame-fed kernel (the cross-check of the tests; callers that fill the frames
        # themselves -- stem_frames -- use the frame-fed kernel either way).
        self.stem_reads_nchw = True
        self._track_versions = False   # set by the first differentiable forward: parameters may now change in place (optimiser steps)
        self._differentiable = block is BasicBlock      # set_differentiable: a Bottleneck encoder opts in
        # the backward's 1x1 / pad 0 layers on the LDS-tiled GEMM kernels (hps_conv1x1_dgrad: the bits of hps_conv_dgrad; hps_conv1x1_wgrad:
        # another slice length, other last bits) where _gemm_dgrad / _gemm_wgrad -- rules on the layer's shape alone -- say so.  False:
        # every layer on hps_conv_dgrad / hps_conv_wgrad (the cross-check of the tests)
        self.gemm_backward = True

    def _make_layer(self, planes, blocks, stride=1):
        """models/resnet.py:178-200 for either block."""
        block, downsample = self.block, None
        if stride != 1 or self.inplanes != planes * block.expansion:
            downsample = nn.Sequential(nn.Conv2d(self.inplanes, planes * block.expansion, kernel_size=1, stride=stride, bias=False),
                                       nn.BatchNorm2d(planes * block.expansion))
        blks = [block(self.inplanes, planes, stride, downsample)]
        self.inplanes = planes * block.expansion
        for _ in range(1, blocks):
            blks.append(block(self.inplanes, planes))
        return nn.Sequential(*blks)

    @property
    def _forward_only(self):
        """A Bottleneck encoder that has not opted in (set_differentiable): forward under no_grad with eval-mode BatchNorm only."""
        return self.block is not BasicBlock and not self.__dict__.get("_differentiable", False)

    def set_differentiable(self, on=True):
        """Opt a Bottleneck (ResNet-50) encoder in to the backward: with it on, a forward under grad mode runs through
        _EncoderFunction as the ResNet-18 encoder's does (the launches and bits of a no_grad forward), set_batchnorm_training(True) and
        then .train() are accepted (every BatchNorm by its own flag, as for ResNet-18), and refresh_weights() rewrites the kernel-side
        weights in place.  Off (the default for Bottleneck): the refusals of a forward-only encoder.  A BasicBlock encoder is always
        differentiable: True is a no-op, False a ValueError.  The call allocates nothing and changes no forward launch; like
        set_winograd a property of the model: it survives .to(), load_state_dict, deepcopy and pickling."""
        if self.block is BasicBlock:
            if not on:
                raise ValueError("the BasicBlock (ResNet-18) encoder is always differentiable")
            return
        self._differentiable = bool(on)

    def train(self, mode=True):
        if mode and self._forward_only:
            raise NotImplementedError("training-mode BatchNorm is not implemented for the Bottleneck (ResNet-50) encoder: it runs in "
                                      ".eval() mode only")
        return super().train(mode)

    # ---- weight preparation (BN folding, k-major filters); redone after .to() / load_state_dict / a switch ----
    def set_winograd(self, on):
        """Product default True: the stride-1 3x3 layers of layer1-3 run as Winograd F(2x2, 3x3) (csrc/conv_wino.hip); False runs
        every layer on the direct implicit-GEMM kernel (csrc/conv_pad.hip) -- the cross-check of the tests."""
        self._winograd = bool(on)
        self._prepared or self.prepare()

    def set_latency_mode(self, on=True):
        """Per-model switch for latency-bound deployments (the reference's own operating point is ONE image per call,
        predict/predict_poseMF_shapeGaussian_net.py:58-104).  The default kernels are built for throughput: a Winograd work item is
        a serial walk of one workgroup over all input channels, and a single image has 4-64 of them for 256 CUs.  In latency mode
        every layer runs the direct implicit-GEMM kernel (the stem in row mode) and the 3x3 layers of layer2-4 split K over
        12-18 workgroups per output tile (+ the slice-sum pass): encoder 0.80 -> 0.42 ms at batch 1; at batch 64 it is ~1.5x
        SLOWER than the default.  Like set_winograd it is a property of the model, never of the batch: per-image results do not
        depend on the batch size within a mode; between the modes they differ in the last bits (another summation order, same
        1e-4 feature tolerance against the reference -- tests/test_gpu_net.py)."""
        self._latency = bool(on)              # switching it off restores whatever set_winograd selected before
        self._prepared or self.prepare()

    def set_batchnorm_training(self, on=True):
        """Opt-in training-mode BatchNorm (models/resnet.py under ``model.train()``, train/train_poseMF_shapeGaussian_net.py:114).
        Off (the default): nothing changes, a forward with ``self.training`` set is refused -- an inference caller who forgot
        ``.eval()`` must not silently normalise a batch-1 predict loop by its own statistics.  On: every convolution's BatchNorm
        decides by ITS OWN ``bn.training`` flag.  A training layer's convolution writes its raw map (identity scale / shift), then
        csrc/bn_train.hip: batch statistics (float64, deterministic), one fold launch that also updates running_mean / running_var
        (unbiased variance, the layer's momentum) and num_batches_tracked on the device, and the epilogue as a pass of its own; an
        eval layer (``enc.layer1.eval()`` after ``enc.train()`` freezes layer1) runs the folded path and the existing backward.  With
        no layer training the call issues exactly the eval launches.  The buffers are updated once per forward (also under no_grad),
        never by the backward's recompute (it applies the statistics the forward saved) and never by training_activations.  Results
        are bitwise repeatable; a training layer's output of course depends on the whole batch, so the independence of an image's
        result from the batch size holds for eval layers only.  Like set_winograd a property of the model: it survives .to(),
        load_state_dict and deepcopy.  FilledStemFrames inputs and ``_gate`` belong to the inference pipeline and are refused while
        a layer is training."""
        if on and self._forward_only:
            raise NotImplementedError("training-mode BatchNorm is not implemented for the Bottleneck (ResNet-50) encoder")
        self._bn_training = bool(on)

    def prepare(self):
        cin = self.conv1.in_channels
        self._cin_pad = (cin + 3) // 4 * 4
        prep = {"stem": _ConvBN(self.conv1, self.bn1, cin_pad=self._cin_pad), "blocks": []}
        for layer in (self.layer1, self.layer2, self.layer3, self.layer4):
            for blk in layer:
                down = _ConvBN(blk.downsample[0], blk.downsample[1]) if blk.downsample is not None else None
                prep["blocks"].append(_Block([_ConvBN(conv, bn) for _, conv, bn in _block_convs(blk)], down))
        for c in self._convs(prep):
            c.latency = self._latency
            c.use_winograd = self._winograd and not self._latency      # latency mode runs every layer on the direct kernel
        if self._track_versions:
            prep["versions"] = self._enc_versions()
        self._prepared = prep
        return prep

    @property
    def _frames(self):
        """The activation frame sets of the current device state, by (batch shape, stream) key."""
        return {key: entry[0] for key, entry in self.device_state().get("frames", {}).items()}

    # ---- halo-padded activation frames: owned by the module, zeroed once, only interiors are ever written ----
    def _frame_set(self, prep, B, C, H, W, device, frames=False):
        """``frames``: the caller fills the stem's phase frames itself (stem_frames / FilledStemFrames): the frame-fed stem kernel."""
        stem = prep["stem"]
        stem_wino = stem.stem_winograd_ok(C, H, W)
        fused_pool = bool(stem_wino and self.fused_pool)
        from_nchw = bool(fused_pool and self.stem_reads_nchw and not frames)
        # (switches and layer modes: one device state each; layer fields edited by hand on a prepared layer: a frame set of their own)
        key = (B, C, H, W, _capi.stream().value, from_nchw, self._variant_state(prep))
        return self._derived("frames", key, lambda: self._new_frame_set(prep, B, C, H, W, device, stem_wino, fused_pool, from_nchw),
                             limit=6)                # a handful of batch shapes / streams at most

    def _new_frame_set(self, prep, B, C, H, W, device, stem_wino, fused_pool, from_nchw, train=False):
        """``train``: a frame set for training flags (_train_frames, _backward_frames with flags): it owns the identity's frame of a
        Bottleneck entry block too -- with the down-sample's or conv3's BatchNorm training, _plan takes the block apart."""
        stem = prep["stem"]
        z = lambda *shape: torch.zeros(*shape, device=device, dtype=torch.float32)
        # input frame of the direct stem: channels as the stem's filters expect them (row mode: row_c; Cin % 32 == 0: cin_p), an even
        # number of columns; zero channels / a zero column are part of the convolution's zero padding
        cf = stem.row_c if stem.wn is None else stem.cin_p
        wf = W + (W & 1)
        generic = cf != C or wf != W or C not in (4, 18, 64)
        if from_nchw:      # the stem reads the NCHW input itself
            fs = {"in": None}
        elif stem_wino:    # four phase frames per image (hps_stem_phase_split), out-of-image pixels zeroed here once
            fs = {"in": z(int(_capi.load(dev=_capi._use_dev).hps_stem_phase_frames_bytes(B, H, W)) // 4)}
        else:
            fs = {"in": z(B, H + 6, wf + 6, cf)}
        fs["stem_wino"], fs["generic_in"] = stem_wino, (C, cf, W, wf) if generic else None
        h, w = stem.out_hw(H, W)
        fs["fused_pool"], fs["from_nchw"] = fused_pool, from_nchw
        if fused_pool:       # the stem's full-resolution output is never materialised; scratch for the items' border contributions
            fs["stem"] = None
            fs["side"] = torch.empty(int(_capi.load(dev=_capi._use_dev).hps_stem_pool_side_bytes(B, H, W)) // 4, device=device, dtype=torch.float32)
        else:
            fs["stem"] = torch.empty(B, h, w, stem.cout, device=device, dtype=torch.float32)
        h, w = (h + 2 - 3) // 2 + 1, (w + 2 - 3) // 2 + 1
        fs["pool"] = z(B, h + 2, w + 2, stem.cout)
        fs["blocks"] = []
        for blk in prep["blocks"]:
            convs, down = blk.convs, blk.down
            hin, win = h, w
            folded = self.fold_downsample and convs[0].folds_down(down, hin, win, 1)
            ent, ws_bytes = {}, down.workspace_bytes(B, hin, win) if down is not None else 0
            for i, c in enumerate(convs):          # one frame per convolution of the main branch: "c1", "c2", ...
                ws_bytes = max(ws_bytes, c.workspace_bytes(B, h, w, 1, down if folded and i == 0 else None))
                h, w = c.out_hw(h, w)
                ent["c%d" % (i + 1)] = z(B, h + 2, w + 2, c.cout)
            # (a Bottleneck entry block whose down-sample rides in conv3's launch never writes the identity's frame)
            ent["down"] = z(B, h + 2, w + 2, down.cout) if down is not None and (train or not self._expands(blk, B, hin, win)) else None
            ent["out"] = ent["c%d" % len(convs)]         # the block's output frame
            ent["ws"] = torch.empty(ws_bytes // 4, device=device, dtype=torch.float32) if ws_bytes else None
            fs["blocks"].append(ent)
        fs["hw"] = (h, w)
        # the launch list of hps_encoder_run: every pointer but the input image and the feature output is fixed
        ops = self._plan(prep, fs, (B, C, H, W))
        fs["ops"] = (_capi.EncOp * len(ops))(*ops)
        return fs

    def _plan(self, prep, fs, shape, flags=None):
        """The forward on the frame set ``fs`` as the ordered list of its steps -- THE walk over the network (models/resnet.py:202-217,
        BasicBlock.forward :62-78): stem, max pool, blocks, average pool.  A step is one launch (a _capi.EncOp; the first one's input and
        the last one's output pointer are the caller's, set per forward) or, with ``flags`` (_train_flags()) naming a layer's BatchNorm as
        training, the _BNStep behind that layer's convolution, which then writes the raw frame: identity scale / shift, no ReLU, no
        residual.  Order within a block: the down-sample (its own launch or riding in c1's), c1, the BatchNorm of .down, of .c1, then
        every further convolution of the main branch with its BatchNorm behind it -- c2 (BasicBlock), c2 and c3 (Bottleneck.forward
        :102-122: c1 1x1, c2 3x3 with the block's stride, c3 1x1) -- the last one with the residual and the block's ReLU."""
        B, C, H, W = shape
        E, P = _capi.EncOp, _capi.ptr
        stem, steps = prep["stem"], []
        train = lambda name: flags is not None and flags[name]
        assert flags is None or not fs["fused_pool"]              # the statistics are needed between the convolution and the pool
        target = lambda name, frame: fs["raw"][name] if train(name) else frame       # where a layer's convolution writes

        def bn(name, cb, out, pad, residual, relu):
            if train(name):
                steps.append(_BNStep(name, cb.cout, fs["raw"][name], out, residual, relu, out.shape[1] - 2 * pad, out.shape[2] - 2 * pad, pad))

        ts = train("stem")
        if fs["stem_wino"]:
            fused = fs["fused_pool"]
            kind = _capi.ENC_STEM_WINOGRAD_POOLED_NCHW if fs["from_nchw"] else _capi.ENC_STEM_WINOGRAD_POOLED if fused else _capi.ENC_STEM_WINOGRAD
            if not fs["from_nchw"]:
                steps.append(E(kind=_capi.ENC_STEM_SPLIT, x=None, y=P(fs["in"]), B=B, Cin=C, H=H, W=W))
            scale, shift = stem.ident if ts else (stem.scale, stem.shift)
            steps.append(E(kind=kind, x=P(fs["in"]), w=P(stem.stem_u), scale=P(scale), shift=P(shift),
                           y=P(fs["pool"] if fused else target("stem", fs["stem"])), splitk_ws=P(fs["side"]) if fused else None, B=B, H=H, W=W,
                           Cin=C, Cout=stem.cout, KH=7, KW=7, stride=2, pad=3, opad=1 if fused else 0, relu=0 if ts else 1))
        else:
            if fs["generic_in"] is not None:
                _, cf, _, wf = fs["generic_in"]
                steps.append(E(kind=_capi.ENC_RELAYOUT_GENERIC, x=None, y=P(fs["in"]), B=B, Cin=C, Cout=cf, H=H, W=W, KW=wf, opad=3))
            else:
                steps.append(E(kind=_capi.ENC_RELAYOUT, x=None, y=P(fs["in"]), B=B, Cin=C, H=H, W=W, opad=3))
            steps.append(stem.op(fs["in"], 3, target("stem", fs["stem"]), 0, relu=not ts, ident=ts))         # conv1 + bn1 + relu
        if not fs["fused_pool"]:
            y = fs["stem"]
            bn("stem", stem, y, 0, None, True)
            steps.append(E(kind=_capi.ENC_MAXPOOL, x=P(y), y=P(fs["pool"]), B=B, H=y.shape[1], W=y.shape[2], Cin=stem.cout, opad=1))
        y = fs["pool"]
        for name, blk, ent in zip(self._block_names(), prep["blocks"], fs["blocks"]):
            convs, down = blk.convs, blk.down
            c1, n1, nd = convs[0], name + ".c1", name + ".down"
            t1, td = train(n1), down is not None and train(nd)
            identity = y if down is None else ent["down"]
            folded = self.fold_downsample and c1.folds_down(down, y.shape[1] - 2, y.shape[2] - 2, 1)
            # Bottleneck entry: the down-sample inside the expand convolution's launch (hps_bottleneck_expand_down), where no BatchNorm
            # of the two is training
            expand = self._expands(blk, B, y.shape[1] - 2, y.shape[2] - 2) and not (td or train("%s.c%d" % (name, len(convs))))
            x_in = y
            assert expand or down is None or ent["down"] is not None
            if down is not None and not folded and not expand:
                steps.append(down.op(y, 1, target(nd, ent["down"]), 1, relu=False, ws=ent["ws"], ident=td))
            steps.append(c1.op(y, 1, target(n1, ent["c1"]), 1, relu=not t1, ws=ent["ws"], ident=t1,
                               down=down if folded else None, out_down=target(nd, ent["down"]) if folded else None, ident_down=td))
            if down is not None:
                bn(nd, down, ent["down"], 1, None, False)
            bn(n1, c1, ent["c1"], 1, None, True)
            y = ent["c1"]
            for i, c in enumerate(convs[1:], 2):
                n, out = "%s.c%d" % (name, i), ent["c%d" % i]
                t, res = train(n), identity if i == len(convs) else None              # the last one closes the block
                if expand and i == len(convs):
                    steps.append(c.expand_down_op(y, 1, x_in, 1, down, out, 1))
                    y = out
                    break
                steps.append(c.op(y, 1, target(n, out), 1, residual=None if t else res, relu=not t, ws=ent["ws"], ident=t))
                bn(n, c, out, 1, res, True)
                y = out
        h, w = fs["hw"]
        steps.append(E(kind=_capi.ENC_AVGPOOL, x=P(y), y=None, B=B, H=h, W=w, Cin=y.shape[3], ipad=1))
        return steps

    def _expands(self, blk, B, H, W):
        """``fold_downsample`` for a Bottleneck entry block ``blk`` on (H, W) input maps: its down-sample rides in conv3's launch."""
        return bool(self.fold_downsample and len(blk.convs) == 3 and blk.convs[-1].expands_with(blk.down, B, H, W))

    @staticmethod
    def _convs(prep):
        """Every _ConvBN in the order of _enc_layers(): the stem, then per block the main branch and the down-sample."""
        return [prep["stem"]] + [c for blk in prep["blocks"] for c in blk if c is not None]

    @staticmethod
    def _variant_state(prep):
        convs = ResNet._convs(prep)
        return tuple((c.variant, c.ksplit, c.use_winograd, c.latency) for c in convs)

    def stem_frames(self, B, C, H, W, device):
        """The phase-frame buffer the Winograd stem will read for a (B, C, H, W) input on the CURRENT stream, wrapped as a
        FilledStemFrames for the caller to fill (hps_proxy_rep_phase_frames) and hand to forward(); None when this shape does not
        take the Winograd stem (then build the NCHW tensor as usual)."""
        prep = self._prepared or self.prepare()
        if not prep["stem"].stem_winograd_ok(C, H, W):
            return None
        fs = self._frame_set(prep, B, C, H, W, device, frames=True)
        if not fs["stem_wino"]:
            return None
        fs["generation"] = fs.get("generation", 0) + 1
        return FilledStemFrames(fs["in"], (B, C, H, W), device, owner=fs, generation=fs["generation"])

    def _forward_padded(self, prep, x, gate=None, fs=None):
        """``gate``: optional callable invoked after the input relayout has been enqueued and before the first convolution
        (InferencePipeline: the HBM-bound relayout may run beside the previous batch's MFMA-bound mesh kernel; the
        convolutions wait).  ``fs``: run on this frame set instead of the module's own for the shape (the backward's recompute)."""
        filled = isinstance(x, FilledStemFrames)
        B, C, H, W = x.shape
        if fs is None:
            fs = self._frame_set(prep, B, C, H, W, x.device, frames=filled)
        if filled and (not fs["stem_wino"] or fs["in"].data_ptr() != x.frames.data_ptr()):
            raise _capi.HpsError("FilledStemFrames belong to another stream / shape / kernel selection than this forward (fill the "
                                 "frames stem_frames() returned on the stream the encoder runs on)")
        if filled:
            if x.owner is not fs or x.generation != fs.get("generation", 0):
                raise _capi.HpsError("stale FilledStemFrames: the encoder's frame buffer has been handed out again (or consumed by a forward) "
                                     "since stem_frames() returned this object; call stem_frames() once per forward")
            fs["generation"] += 1                        # consumed: a second forward with the same object would read whatever the frames hold then
        elif fs.get("in") is not None and fs["stem_wino"]:
            fs["generation"] = fs.get("generation", 0) + 1      # the phase split below overwrites the frames
        # the frame set's launch list (_plan): one call across the C ABI for the whole encoder (csrc/composite.hip), two when it is
        # gated; ``composite`` False: the same list launch by launch through the public entry points (the cross-check of the tests)
        feats = torch.empty(B, fs["blocks"][-1]["out"].shape[3], device=x.device, dtype=torch.float32)
        ops = fs["ops"]
        n = len(ops)
        ops[n - 1].y = feats.data_ptr()
        if filled:                                       # the caller fills the phase frames: the list starts at the stem convolution
            first = 1
        else:
            ops[0].x = x.data_ptr()
            # op 0 is the input relayout / phase split in front of the gate -- unless the stem reads the NCHW input itself: the whole list waits
            first = 0 if gate is None or fs["from_nchw"] else 1
            if first:
                _capi.run_enc_ops(ops, 0, 1, self.composite)
        if gate is not None:
            gate()
        if filled:
            x.run_fill()
        _capi.run_enc_ops(ops, first, n - first, self.composite)
        return feats

    def forward(self, x, _gate=None):
        """models/resnet.py:202-217: (B,C,H,W) NCHW fp32 -> (B, 512 * block.expansion)."""
        flags = self._train_flags()
        filled = isinstance(x, FilledStemFrames)
        if flags is not None:
            if filled or _gate is not None:
                raise RuntimeError("FilledStemFrames inputs and _gate are the inference pipeline's paths; not with a BatchNorm in training mode")
            self._check_training(flags, x.shape)                  # before any launch, before any buffer is touched
            _capi.require_device(x, "encoder input")
        differentiable = torch.is_grad_enabled() and not filled and (
            (isinstance(x, torch.Tensor) and x.requires_grad) or any(w.requires_grad for w in self._enc_params()))
        if differentiable and self._forward_only:
            raise NotImplementedError("the backward of the Bottleneck (ResNet-50) encoder is not implemented: run it under torch.no_grad() "
                                      "(or with no input / encoder parameter requiring grad)")
        if differentiable:
            self._track_versions = True
        prep = self._current_prep()
        if filled:
            return self._forward_padded(prep, x, gate=_gate)
        _capi.require_device(x, "encoder input")
        if differentiable:
            return _EncoderFunction.apply(self, prep, _gate, flags, x, *self._enc_params())
        if flags is not None:
            xc = _capi.f32c(x)
            B, C, H, W = xc.shape
            return self._forward_train(prep, xc, self._train_frames(prep, B, C, H, W, xc.device, flags), flags, update=True)[0]
        # every (C, H, W) runs on the product kernels: shapes the stem's fast paths do not take get a channel-padded, even-width input
        # frame (hps_nchw_to_padded_nhwc_generic) in front of the row-mode / direct stem
        return self._forward_padded(prep, _capi.f32c(x), gate=_gate)

    def stage_taps(self, shape, device, x=None, fill=None):
        """The outputs of layer1..4 (C2..C5 of a feature pyramid, strides 4, 8, 16, 32) for a (B, C, H, W) input: the existing launch
        plan of ``forward`` without its closing average pool, handed back as the four block-output frames themselves -- halo-padded NHWC
        (B, h + 2, w + 2, c), zero halo -- which belong to the module: read them, never write them, and copy what must outlive the
        next forward of this shape on this stream.  Read-only: no launch is added for any other caller and ``forward`` keeps its bits.
        ``x``: the NCHW input; or ``fill(frame)``, a callable that writes the interior of the direct stem's input frame
        (B, H + 6, W + 6, row channels; channels past C and the halo stay zero) in the input relayout's place -- for shapes whose stem
        reads such a frame (not the Winograd stem of the 18-channel model).  Eval-mode BatchNorm, no autograd."""
        if self._train_flags() is not None:
            raise RuntimeError("stage_taps runs eval-mode BatchNorm only")
        B, C, H, W = shape
        prep = self._current_prep()
        fs = self._frame_set(prep, B, C, H, W, device)
        ops = fs["ops"]
        n = len(ops) - 1                                   # the average pool closes the list: not run
        if x is not None:
            _capi.require_device(x, "encoder input")
            xc = _capi.f32c(x.detach())
            if tuple(xc.shape) != tuple(shape):
                raise _capi.HpsError("stage_taps: the input is %s, not %s" % (tuple(xc.shape), tuple(shape)))
            ops[0].x = xc.data_ptr()
            _capi.run_enc_ops(ops, 0, n, self.composite)
        else:
            if fill is None or fs["stem_wino"] or fs.get("in") is None:
                raise _capi.HpsError("stage_taps: give the input, or fill() for a shape whose stem reads a padded NHWC frame")
            fill(fs["in"])
            _capi.run_enc_ops(ops, 1, n - 1, self.composite)
        last, taps = -1, []
        for layer in (self.layer1, self.layer2, self.layer3, self.layer4):
            last += len(layer)
            taps.append(fs["blocks"][last]["out"])
        return taps

    # ---- training-mode BatchNorm (csrc/bn_train.hip) ----
    def _train_flags(self):
        """None when every BatchNorm runs on running statistics, else {layer name: its BatchNorm is training} over _enc_layers().
        Switch off: a module in training mode is refused."""
        if not self._bn_training:
            if self.training:
                raise RuntimeError("the MI355X encoder path runs eval-mode BatchNorm only (running statistics, also when fine-tuning); "
                                   "call .eval(), or opt in to batch statistics with set_batchnorm_training(True)")
            return None
        flags = {name: bool(bn.training) for name, _, bn in self._enc_layers()}
        return flags if any(flags.values()) else None

    def _layer_maps(self, H, W):
        """{layer name: (Ho, Wo)} of every convolution's output for an (H, W) input."""
        hw = lambda h, w, k, s, p: ((h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1)
        out = {"stem": hw(H, W, 7, 2, 3)}
        h, w = hw(*out["stem"], 3, 2, 1)
        for name, conv, _ in self._enc_layers()[1:]:
            if not name.endswith(".down"):          # the down-sample's map is its block's output map
                h, w = hw(h, w, conv.kernel_size[0], conv.stride[0], conv.padding[0])
            out[name] = (h, w)
        return out

    def _check_training(self, flags, shape):
        """torch's own refusals for the training layers, raised before any launch and before any buffer is touched."""
        B, _, H, W = shape
        maps = self._layer_maps(H, W)
        for name, _, bn in self._enc_layers():
            if not flags[name]:
                continue
            if bn.momentum is None:
                raise NotImplementedError("%s: momentum=None (cumulative moving average) is not implemented on the device" % name)
            if not bn.track_running_stats or bn.running_mean is None:
                raise NotImplementedError("%s: track_running_stats=False is not implemented on the device" % name)
            if not bn.affine:
                raise NotImplementedError("%s: affine=False is not implemented on the device" % name)
            h, w = maps[name]
            if B * h * w == 1:
                raise ValueError("Expected more than 1 value per channel when training, got input size %s (%s)"
                                 % (torch.Size((B, bn.num_features, h, w)), name))

    def _current_prep(self):
        """The kernel-side weights for the parameters and statistics as they are now: rebuilt after an optimiser step (version
        counters, from the first differentiable forward on), eval-mode folds redone in place for the layers whose running statistics
        a training forward has moved since (the fold kernel writes through data_ptr(): no version counter sees it)."""
        if self._track_versions and self._prepared is not None and self._prepared.get("versions") != self._enc_versions():
            self.invalidate()                                     # an optimiser step (or any in-place edit) since prepare()
        prep = self._prepared or self.prepare()
        stale = prep.get("stale_bn")
        if stale:
            convs = self._convs(prep)
            with torch.no_grad():
                for (name, _, bn), cb in zip(self._enc_layers(), convs):
                    if name in stale:
                        cb.refold(bn)
                        prep.get("bwd", {}).pop(name, None)       # the data gradient's scaled filter
            stale.clear()
        return prep

    # ---- after an optimiser step that says so (device_optim.DeviceAdam): the derived weights again, in place ----
    def _refresh_token(self, prep):
        tensors = [t for _, conv, bn in self._enc_layers() for t in (conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var)]
        if not all(t.is_cuda and plain(t) for t in tensors):
            return None
        return tuple(t.data_ptr() for t in tensors), frozenset(prep.get("bwd", {}))

    def _refresh_list(self, prep, token):
        """One hps_refresh_op per tensor _ConvBN.__init__ / _dgrad_filter derive from a parameter, in their layouts; the folds first
        (the scaled data-gradient filters read them)."""
        ref = RefreshList(token)
        bwd = prep.get("bwd", {})
        convs = self._convs(prep)
        layers = list(zip(self._enc_layers(), convs))
        for (_, _, bn), cb in layers:
            ref.fold(bn, cb.scale, cb.shift)
        for (name, conv, _), cb in layers:
            w = conv.weight
            cout, cin, kh, kw = w.shape
            s_o, s_c, s_i, s_j = cin * kh * kw, kh * kw, kw, 1
            ref.permute(w, cb.wk, (kh, kw, cin, cout), (s_i, s_j, s_c, s_o), (kw * cb.cin_p * cout, cb.cin_p * cout, cout, 1))
            if cb.wn is not None:
                ref.permute(w, cb.wn, (cout, kh, kw, cin), (s_o, s_i, s_j, s_c), (kh * kw * cb.cin_p, kw * cb.cin_p, cb.cin_p, 1))
            if cb.wrow is not None:
                ck = cb.wrow.shape[1] // kh
                ref.permute(w, cb.wrow, (cout, kh, kw, cin), (s_o, s_i, s_j, s_c), (kh * ck, ck, cb.row_c, 1))
            if cb.wino_u is not None:
                ref.winograd(w, cb.wino_u)
            if cb.stem_u is not None:
                ref.winograd(w, cb.stem_u, stem=True)
            for key, scale in ((name + ".raw", None), (name, cb.scale)):
                if key in bwd:
                    ref.permute(w, bwd[key], (kh, kw, cout, cin), (s_i, s_j, s_o, s_c), (kw * cout * cin, cout * cin, cin, 1),
                                scale=scale, scale_dim=2)
        return ref

    def refresh_weights(self):
        """Write every kernel-side tensor of the prepared state again, in place, from the parameters and running statistics as they
        are now (hps_weights_refresh), and record the parameters' version counters: the next forward keeps the state -- frames,
        launch lists, captured graphs -- where the version check would have dropped it.  The eval-mode folds of the layers a training
        forward marked stale are redone by this very pass (the same float64 arithmetic, the same bits as _ConvBN.refold).  Without a
        prepared state: nothing to do.  Parameters the kernels cannot read in place (another dtype, a replaced storage): the state
        is dropped instead, as after any other edit."""
        prep = self._prepared
        if prep is None:
            return
        if self._forward_only:          # a Bottleneck encoder that has not opted in (set_differentiable): drop the state, which is always correct
            self.invalidate()
            return
        token = self._refresh_token(prep)
        ref = self._device_state.get("refresh")
        if token is None or (ref is not None and ref.token[0] != token[0]):
            self.invalidate()
            return
        if ref is None or ref.token != token:
            ref = self._device_state["refresh"] = self._refresh_list(prep, token)
        ref.run()
        prep.get("stale_bn", set()).clear()
        prep["versions"] = self._enc_versions()

    def _train_frames(self, prep, B, C, H, W, device, flags):
        """The training forward's frame set for a batch shape on the current stream: as the backward's activation set (unfused stem
        and pool: the statistics are needed between the convolution and the pool) plus one raw frame per training layer."""
        key = (B, C, H, W, _capi.stream().value, tuple(flags.values()), self._variant_state(prep))
        return self._derived("train_frames", key, lambda: self._add_raw_frames(
            prep, self._new_frame_set(prep, B, C, H, W, device, prep["stem"].stem_winograd_ok(C, H, W), False, False, train=True), (B, C, H, W),
            flags), limit=4)

    def _add_raw_frames(self, prep, fs, shape, flags):
        """... and with them the training forward's steps, ``fs["plan"]`` (_plan with ``flags``: every pointer in it is fixed)."""
        raw = {"stem": torch.empty_like(fs["stem"]) if flags["stem"] else None}
        for name, ent in zip(self._block_names(), fs["blocks"]):
            for k in [k for k in ("c1", "c2", "c3") if k in ent] + ["down"]:
                raw[name + "." + k] = torch.empty_like(ent[k]) if ent[k] is not None and flags[name + "." + k] else None
        fs["raw"] = raw
        fs["plan"] = self._plan(prep, fs, shape, flags)
        return fs

    def _forward_train(self, prep, x, fs, flags, saved=None, update=False):
        """The forward with batch statistics in the layers ``flags`` names, step by step over ``fs["plan"]`` (_add_raw_frames), one
        call across the C ABI per launch: (features, {name: (mean, biased var or None, invstd, n)}).  The convolution kernels and the
        rules that pick them are those of the eval forward.  ``saved`` {name: (mean, invstd)}: apply these statistics instead of reducing
        them (the backward's recompute).  ``update``: the fold launch also updates the layer's running buffers and counter."""
        B = x.shape[0]
        s, P = _capi.stream(), _capi.ptr
        D = lambda t: _capi.ptr(t, torch.float64)
        lib = _capi.load(dev=_capi._use_dev)
        dev, f64 = x.device, torch.float64
        bns = {name: bn for name, _, bn in self._enc_layers()}
        stats = {}

        def normalise(name, c, z, out, residual, relu, h, w, pad):
            """raw frame ``z`` of ``name`` -> statistics -> fold -> out = act(raw scale + shift [+ residual])"""
            bn = bns[name]
            scale, shift = torch.empty(c, device=dev), torch.empty(c, device=dev)
            gamma, beta = _capi.f32c(bn.weight.detach()), _capi.f32c(bn.bias.detach())
            n = B * h * w
            if saved is None:
                mean, var, invstd = (torch.empty(c, device=dev, dtype=f64) for _ in range(3))
                ws = torch.empty(max(1, int(lib.hps_bn_batch_stats_workspace(B, h, w, c)) // 8), device=dev, dtype=f64)
                _capi.call("hps_bn_batch_stats", P(z), D(ws), D(mean), D(var), B, h, w, c, pad, s)
                if update:
                    _capi.call("hps_bn_train_fold", D(mean), D(var), D(invstd), P(gamma), P(beta), float(bn.eps), float(bn.momentum), n,
                               P(scale), P(shift), P(bn.running_mean), P(bn.running_var),
                               _capi.ptr(bn.num_batches_tracked, torch.int64), c, s)
                else:
                    _capi.call("hps_bn_train_fold", D(mean), D(var), D(invstd), P(gamma), P(beta), float(bn.eps), 0.0, n, P(scale), P(shift),
                               None, None, None, c, s)
            else:
                (mean, invstd), var = saved[name], None
                _capi.call("hps_bn_train_fold", D(mean), None, D(invstd), P(gamma), P(beta), float(bn.eps), 0.0, n, P(scale), P(shift),
                           None, None, None, c, s)
            _capi.call("hps_bn_apply_act_pad", P(z), P(scale), P(shift), P(residual) if residual is not None else None, P(out), B, h, w, c,
                       pad, pad, 1 if relu else 0, s)
            stats[name] = (mean, var, invstd, n)

        plan = fs["plan"]
        feats = torch.empty(B, fs["blocks"][-1]["out"].shape[3], device=dev, dtype=torch.float32)
        plan[0].x, plan[-1].y = x.data_ptr(), feats.data_ptr()
        for step in plan:
            if isinstance(step, _BNStep):
                normalise(*step)
            else:
                _capi.issue_enc_op(step)
        if update:
            prep.setdefault("stale_bn", set()).update(stats)      # their eval-mode folds no longer match the running statistics
        return feats, stats

    # ---- backward (csrc/conv_backward.hip) ----
    def _enc_layers(self):
        """(name, conv, bn) of every convolution in the order of prepare(): the stem, then conv1 / conv2 [/ conv3] / downsample per block."""
        out = [("stem", self.conv1, self.bn1)]
        for li, layer in enumerate((self.layer1, self.layer2, self.layer3, self.layer4), 1):
            for bi, blk in enumerate(layer):
                out += [("layer%d.%d.%s" % (li, bi, k), conv, bn) for k, conv, bn in _block_convs(blk)]
                if blk.downsample is not None:
                    out.append(("layer%d.%d.down" % (li, bi), blk.downsample[0], blk.downsample[1]))
        return out

    def _enc_params(self):
        """The parameters in the order _EncoderFunction takes them and _backward returns their gradients: conv weight, BatchNorm
        weight, BatchNorm bias per convolution of _enc_layers()."""
        return [w for _, conv, bn in self._enc_layers() for w in (conv.weight, bn.weight, bn.bias)]

    def _enc_versions(self):
        return tuple(t._version for _, conv, bn in self._enc_layers()
                     for t in (conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var))

    def _block_names(self):
        return ["layer%d.%d" % (li, bi) for li, layer in enumerate((self.layer1, self.layer2, self.layer3, self.layer4), 1)
                for bi in range(len(layer))]

    def _backward_frames(self, prep, B, C, H, W, device, flags=None):
        """The backward's own frames for a batch shape on the current stream: an activation set for the recompute (stem output
        written out, max pool as a launch of its own; phase split + frame-fed kernel where the forward took the Winograd stem -- the
        same values as the fused launches) and one cotangent frame per activation frame, halos zeroed once."""
        # the launch list points at ``prep``'s filters: a backward that outlives a kernel-mode switch keeps its own set
        key = (B, C, H, W, _capi.stream().value, id(prep), tuple(flags.values()) if flags else None, self._variant_state(prep))

        def build():
            stem = prep["stem"]
            fs = self._new_frame_set(prep, B, C, H, W, device, stem.stem_winograd_ok(C, H, W), False, False, train=bool(flags))
            z = lambda *shape: torch.zeros(*shape, device=device, dtype=torch.float32)
            g = {"xin": z(B, H + 6, W + 6, C), "stem": torch.empty_like(fs["stem"]), "pool": torch.zeros_like(fs["pool"]), "blocks": []}
            y = fs["pool"]
            for blk, ent in zip(prep["blocks"], fs["blocks"]):
                # one cotangent frame per convolution of the main branch ("c1", "c2" [, "c3"]); "out": the block's output cotangent
                ge = {"c%d" % i: torch.zeros_like(ent["c%d" % i]) for i in range(1, len(blk.convs) + 1)}
                ge["out"] = ge["c%d" % len(blk.convs)]
                ge["tmp"] = torch.zeros_like(y) if blk.down is not None else None
                g["blocks"].append(ge)
                y = ent["out"]
            if flags:        # raw maps of the training layers; their dz frames (out of place: the gated cotangent has other readers)
                self._add_raw_frames(prep, fs, (B, C, H, W), flags)
                g["dz_stem"] = torch.empty_like(fs["stem"]) if flags["stem"] else None
                for name, ent, ge in zip(self._block_names(), fs["blocks"], g["blocks"]):
                    by_shape = {}          # one dz frame per map shape of the block: a convolution's dz is consumed before the next is written
                    for k in [k for k in ("c1", "c2", "c3") if k in ent]:
                        if flags[name + "." + k]:
                            if tuple(ent[k].shape) not in by_shape:
                                by_shape[tuple(ent[k].shape)] = torch.zeros_like(ent[k])
                            ge["dz_" + k] = by_shape[tuple(ent[k].shape)]
                    ge["dzd"] = torch.zeros_like(ent["out"]) if ent["down"] is not None and flags[name + ".down"] else None
            return fs, g, prep
        return self._derived("backward_frames", key, build, limit=6)[:2]

    def _recompute(self, prep, x):
        """The forward again on the backward's frame set: (features, activation frames, cotangent frames)."""
        B, C, H, W = x.shape
        fs, g = self._backward_frames(prep, B, C, H, W, x.device)
        return self._forward_padded(prep, x, fs=fs), fs, g

    def activations(self, x):
        """(features, {name: NCHW clone}) of the recompute the backward differentiates -- the very code path: 'stem' (conv1 + bn1 +
        relu), 'pool', and per block 'layerL.j.c1' (after its ReLU), 'layerL.j.c2' (the block's output) and 'layerL.j.down'.  The
        ReLU masks (map > 0) and the pool winners of the device's function are read off these maps (the tests pin their float64
        restatement to them).  A Bottleneck: 'layerL.j.c1' and '.c2' after their ReLUs, 'layerL.j.c3' the block's output; no
        '.down' where the down-sample rides in conv3's launch (fold_downsample: its frame is never written, and no ReLU reads it)."""
        if self._train_flags() is not None:
            raise RuntimeError("a BatchNorm is in training mode: use training_activations()")
        _capi.require_device(x, "encoder input")
        with torch.no_grad():
            feats, fs, _ = self._recompute(self._current_prep(), _capi.f32c(x))
            return feats, self._maps_of(fs)

    def _maps_of(self, fs):
        nchw = lambda t, p: (t[:, p:t.shape[1] - p, p:t.shape[2] - p] if p else t).permute(0, 3, 1, 2).clone()
        maps = {"stem": nchw(fs["stem"], 0), "pool": nchw(fs["pool"], 1)}
        for name, ent in zip(self._block_names(), fs["blocks"]):
            for k in ("c1", "c2", "c3"):
                if k in ent:
                    maps[name + "." + k] = nchw(ent[k], 1)
            if ent["down"] is not None:
                maps[name + ".down"] = nchw(ent["down"], 1)
        return maps

    def training_activations(self, x):
        """(features, maps, stats) of the training-mode function the backward differentiates -- the very code path (the recompute's
        frames and launches, statistics reduced instead of taken from a forward), WITHOUT any running-buffer update.  ``maps`` as
        activations() names them; ``stats[name] = (mean float64 (C,), biased variance float64 (C,), n)`` for every layer whose
        BatchNorm is training, ``name`` as in _enc_layers().  Needs set_batchnorm_training(True)."""
        flags = self._train_flags()
        _capi.require_device(x, "encoder input")
        if flags is not None:
            self._check_training(flags, x.shape)
        with torch.no_grad():
            prep = self._current_prep()
            xc = _capi.f32c(x)
            if flags is None:
                feats, fs, _ = self._recompute(prep, xc)
                return feats, self._maps_of(fs), {}
            B, C, H, W = xc.shape
            fs, _ = self._backward_frames(prep, B, C, H, W, xc.device, flags)
            feats, stats = self._forward_train(prep, xc, fs, flags, update=False)
            return feats, self._maps_of(fs), {name: (mean.clone(), var.clone(), n) for name, (mean, var, _, n) in stats.items()}

    @staticmethod
    def _prepare_backward(prep):
        """What only the backward needs, built at the first backward of a prepared state: per convolution the filter as
        (KH, KW, Cout, Cin) with the folded BatchNorm scale of the output channel multiplied in (float64, rounded once) -- the B
        operand of hps_conv_dgrad."""
        q = prep.get("bwd")
        if q is None:
            q = prep["bwd"] = {}
        return q

    def _dgrad_filter(self, prep, name, conv, cb, raw=False):
        """``raw``: the unscaled filter (a training layer: hps_bn_train_backward_dz has the scale in dz)."""
        q = self._prepare_backward(prep)
        key = name + ".raw" if raw else name
        if key not in q:
            w = conv.weight.detach().double()
            if not raw:
                w = w * cb.scale.double()[:, None, None, None]
            q[key] = w.permute(2, 3, 0, 1).float().contiguous()
        return q[key]

    def _gemm_dgrad(self, cb):
        """This layer's data gradient runs on hps_conv1x1_dgrad: every 1x1 / pad 0 layer the kernel takes (identical bits, so the rule
        is one of speed alone)."""
        return bool(self.gemm_backward and cb.kh == cb.kw == 1 and cb.pad == 0 and cb.stride in (1, 2) and cb.cout % 8 == 0)

    def _gemm_wgrad(self, cb):
        """This layer's weight gradient runs on hps_conv1x1_wgrad (other last bits than hps_conv_wgrad): the 1x1 / pad 0 layers with
        Cin Cout >= 16384 (at 64 -> 64 the two kernels' quartiles overlap, tools/resnet50_backward_time.py) and stride 1, or stride 2
        from 1024 output channels on -- a rule on the layer alone that leaves the ResNet-18 encoder's three down-samples (1x1 / 2, up
        to 512 channels) on hps_conv_wgrad, whose bits its tests pin; the price is layer2's 256 -> 512 / 2 down-sample of the
        Bottleneck encoder, the same layer shape, which stays there too (0.63 against 0.32 ms at B = 72)."""
        return bool(self._gemm_dgrad(cb) and cb.cin * cb.cout >= 16384 and (cb.stride == 1 or cb.cout >= 1024))

    def _backward(self, prep, x, g_feats, needs, flags=None, saved=None):
        """(input gradient or None, parameter gradients in _enc_params() order, None where ``needs`` does not ask) for the cotangent
        ``g_feats`` (B, 512 * block.expansion). ``flags`` / ``saved``: the layers that ran on batch statistics and the (mean, invstd) the forward saved --
        the recompute applies them (no reduction, no running-buffer update) and writes the raw maps; such a layer's backward is
        hps_bn_train_backward_sums (with the ReLU gate in the same sweep where the block allows it) and hps_bn_train_backward_dz, then
        the weight gradient of dz IS dW and the data gradient takes the unscaled filter.  ``needs``: [input] + one flag per parameter.  Kernels whose result nobody wants are not launched: no
        weight gradient for a frozen convolution, no data gradient below the lowest layer that wants one, the stem's data
        gradient only for an input that requires grad."""
        P, s = _capi.ptr, _capi.stream()
        lib = _capi.load(dev=_capi._use_dev)
        B, C, H, W = x.shape
        dev = x.device
        flags = flags or {}
        if flags:
            fs, gf = self._backward_frames(prep, B, C, H, W, dev, flags)
            self._forward_train(prep, x, fs, flags, saved=saved, update=False)
        else:
            _, fs, gf = self._recompute(prep, x)
        D = lambda t: _capi.ptr(t, torch.float64)
        trains = lambda name: bool(flags.get(name))
        layers = self._enc_layers()
        want = {name: needs[1 + 3 * i:4 + 3 * i] for i, (name, _, _) in enumerate(layers)}
        mods = {name: (conv, bn) for name, conv, bn in layers}
        grads = {}
        ws_cache = {}

        def scratch(nbytes, dtype):
            n = max(1, nbytes // (8 if dtype == torch.float64 else 4))
            t = ws_cache.get(dtype)
            if t is None or t.numel() < n:
                t = ws_cache[dtype] = torch.empty(n, device=dev, dtype=dtype)
            return t

        def gate(g, y, Bh, h, w, c, gpad, ypad, want_sums):
            """g <- g * (y > 0) in place; the per-channel sums of the gated cotangent when a shift / scale gradient wants them."""
            sums = torch.empty(c, device=dev, dtype=torch.float32) if want_sums else None
            ws = scratch(int(lib.hps_relu_gate_workspace(Bh, h, w, c)), torch.float64) if want_sums else None
            _capi.call("hps_relu_gate_pad", P(g), P(y), _capi.ptr(ws, torch.float64) if want_sums else None, P(sums), Bh, h, w, c, gpad, ypad, s)
            return sums

        def train_sums(name, cb, g, gpad, y, ypad, h, w):
            """(d beta, d gamma) float64 (2 C,) of a training layer from the cotangent frame ``g``; with ``y`` the ReLU gate is applied to
            g in the same sweep."""
            mean, invstd = saved[name]
            ws = scratch(int(lib.hps_bn_train_backward_sums_workspace(B, h, w, cb.cout)), torch.float64)
            sums = torch.empty(2 * cb.cout, device=dev, dtype=torch.float64)
            _capi.call("hps_bn_train_backward_sums", P(g), P(fs["raw"][name]), P(y) if y is not None else None, D(mean), D(invstd), D(ws),
                       D(sums), B, h, w, cb.cout, gpad, ypad, ypad, s)
            return sums

        def train_dz(name, cb, g, gpad, sums, dz, h, w):
            mean, invstd = saved[name]
            _capi.call("hps_bn_train_backward_dz", P(g), P(fs["raw"][name]), D(mean), D(invstd), P(_capi.f32c(mods[name][1].weight.detach())),
                       D(sums), P(dz), B, h, w, cb.cout, gpad, gpad, gpad, s)
            return dz

        def wgrad(cb, xf, ipad, cx, cin, hin, win, g, gpad):
            """G (Cout, KH, KW, Cin) = corr(xf, g): hps_conv1x1_wgrad where _gemm_wgrad sends the layer, else hps_conv_wgrad."""
            G = torch.empty(cb.cout, cb.kh, cb.kw, cin, device=dev, dtype=torch.float32)
            if self._gemm_wgrad(cb):
                ws = scratch(int(lib.hps_conv1x1_wgrad_workspace(B, hin, win, cin, cb.cout, cb.stride)), torch.float32)
                _capi.call("hps_conv1x1_wgrad", P(xf), P(g), P(G), P(ws), B, hin, win, ipad, cx, cin, cb.cout, cb.stride, gpad, s)
            else:
                ws = scratch(int(lib.hps_conv_wgrad_workspace(B, hin, win, cin, cb.cout, cb.kh, cb.kw, cb.stride, cb.pad)), torch.float32)
                _capi.call("hps_conv_wgrad", P(xf), P(g), P(G), P(ws), B, hin, win, ipad, cx, cin, cb.cout, cb.kh, cb.kw, cb.stride, cb.pad,
                           gpad, s)
            return G

        def train_params(name, cb, xf, ipad, cx, cin, hin, win, dz, gpad, sums):
            """Gradients of a training layer: dW = corr(x, dz), d gamma and d beta are the sums themselves."""
            conv, bn = mods[name]
            w_w, w_g, w_b = want[name]
            dW = None
            if w_w:
                dW = wgrad(cb, xf, ipad, cx, cin, hin, win, dz, gpad).permute(0, 3, 1, 2).to(conv.weight.dtype).contiguous()
            if w_w or w_g or w_b:
                grads[name] = (dW, sums[cb.cout:].to(bn.weight.dtype) if w_g else None, sums[:cb.cout].to(bn.bias.dtype) if w_b else None)

        def params(name, cb, xf, ipad, cx, cin, hin, win, g, gpad, sums):
            """Gradients of one convolution's weight and BatchNorm affine from its gated cotangent frame ``g`` and input frame ``xf``."""
            conv, bn = mods[name]
            w_w, w_g, w_b = want[name]
            if not (w_w or w_g or w_b):
                return
            d = torch.float64
            inv_std = torch.rsqrt(bn.running_var.detach().to(d) + bn.eps)
            dW = dscale = None
            if w_w or w_g:
                Gd = wgrad(cb, xf, ipad, cx, cin, hin, win, g, gpad).permute(0, 3, 1, 2).to(d)      # (Cout, Cin, KH, KW), the weight's layout
                if w_w:
                    dW = (Gd * cb.scale.to(d)[:, None, None, None]).to(conv.weight.dtype).contiguous()
                if w_g:
                    dscale = (Gd * conv.weight.detach().to(d)).sum((1, 2, 3))
            dg = (inv_std * (dscale - bn.running_mean.detach().to(d) * sums.to(d))).to(bn.weight.dtype) if w_g else None
            db = sums.to(bn.bias.dtype) if w_b else None
            grads[name] = (dW, dg, db)

        def dgrad(name, cb, g, gpad, other, dx, dpad, cdx, cin, hin, win):
            conv, _ = mods[name]
            wt = self._dgrad_filter(prep, name, conv, cb, trains(name))
            if self._gemm_dgrad(cb):               # the same bits (hps_conv1x1_dgrad keeps hps_conv_dgrad's summation order)
                _capi.call("hps_conv1x1_dgrad", P(g), P(wt), P(other), P(dx), B, hin, win, cin, cb.cout, cb.stride, gpad, dpad, cdx, s)
            else:
                _capi.call("hps_conv_dgrad", P(g), P(wt), P(other), P(dx), B, hin, win, cin, cb.cout, cb.kh, cb.kw, cb.stride, cb.pad, gpad, dpad,
                           cdx, s)

        # which blocks still have somebody below them asking for a gradient
        names = self._block_names()
        conv_names = lambda name, blk: [name + ".c%d" % i for i in range(1, len(blk.convs) + 1)]
        below = [needs[0] or any(want["stem"])]
        for name, blk in zip(names, prep["blocks"]):
            here = any(any(want[n]) for n in conv_names(name, blk)) or (blk.down is not None and any(want[name + ".down"]))
            below.append(below[-1] or here)
        h, w = fs["hw"]
        last = fs["blocks"][-1]["out"]
        _capi.call("hps_global_avgpool_backward", P(_capi.f32c(g_feats)), P(gf["blocks"][-1]["out"]), B, h, w, last.shape[3], 1, s)
        # Per block (BasicBlock.forward models/resnet.py:62-78, Bottleneck.forward :102-122), last convolution first: the block's ReLU gate
        # on the last convolution's output frame, then per convolution its parameter gradients, the data gradient into the previous
        # convolution's cotangent frame and that frame's gate; the first one's data gradient takes the identity branch as ``other``.
        for k in range(len(names) - 1, -1, -1):
            name, blk, ent, ge = names[k], prep["blocks"][k], fs["blocks"][k], gf["blocks"][k]
            convs, down, n = blk.convs, blk.down, len(blk.convs)
            cn, nd = conv_names(name, blk), name + ".down"
            y_in = fs["blocks"][k - 1]["out"] if k else fs["pool"]
            g_in = gf["blocks"][k - 1]["out"] if k else gf["pool"]
            hin, win, cin = y_in.shape[1] - 2, y_in.shape[2] - 2, y_in.shape[3]
            out, g_out = ent["out"], ge["out"]
            ho, wo = out.shape[1] - 2, out.shape[2] - 2
            cl, nl = convs[-1], cn[-1]
            xl = ent["c%d" % (n - 1)]                                                            # the last convolution's input frame
            hl, wl = xl.shape[1] - 2, xl.shape[2] - 2
            tl, td = trains(nl), down is not None and trains(nd)
            asks = [below[k]]                      # asks[i]: somebody below convolution i + 1 wants something
            for i in range(1, n):
                asks.append(asks[-1] or any(want[cn[i - 1]]))
            more = asks[n - 1]
            sums_d = want[nl][1] or want[nl][2] or (down is not None and (want[nd][1] or want[nd][2]))
            gl = gd = g_out
            if tl and (td or down is None):        # the block's ReLU, both branches -- in the sweep of the last convolution's sums
                sl = train_sums(nl, cl, g_out, 1, out, 1, ho, wo)
                sums_l = None
            else:
                sums_l = gate(g_out, out, B, ho, wo, cl.cout, 1, 1, sums_d)
                sl = train_sums(nl, cl, g_out, 1, None, 1, ho, wo) if tl else None
            if tl:
                if more or want[nl][0]:
                    gl = train_dz(nl, cl, g_out, 1, sl, ge["dz_c%d" % n], ho, wo)
                train_params(nl, cl, xl, 1, cl.cin_p, cl.cin_p, hl, wl, gl, 1, sl)
            else:
                params(nl, cl, xl, 1, cl.cin_p, cl.cin_p, hl, wl, g_out, 1, sums_l)
            if td:
                if below[k] or any(want[nd]):
                    sd = train_sums(nd, down, g_out, 1, None, 1, ho, wo)
                    if below[k] or want[nd][0]:
                        gd = train_dz(nd, down, g_out, 1, sd, ge["dzd"], ho, wo)
                    train_params(nd, down, y_in, 1, cin, cin, hin, win, gd, 1, sd)
            elif down is not None:
                params(nd, down, y_in, 1, cin, cin, hin, win, g_out, 1, sums_l)
            stop, gprev = not more, gl                                                           # nobody below wants anything
            for i in range(n - 1, 0, -1):          # convolution i: its cotangent frame <- the data gradient of convolution i + 1
                if stop:
                    break
                ci, ni, ei, gi = convs[i - 1], cn[i - 1], ent["c%d" % i], ge["c%d" % i]
                hi, wi = ei.shape[1] - 2, ei.shape[2] - 2
                dgrad(cn[i], convs[i], gprev, 1, None, gi, 1, convs[i].cin_p, convs[i].cin_p, hi, wi)
                xi = y_in if i == 1 else ent["c%d" % (i - 1)]
                hx, wx, cx = xi.shape[1] - 2, xi.shape[2] - 2, xi.shape[3]
                gprev = gi
                if trains(ni):
                    si = train_sums(ni, ci, gi, 1, ei, 1, hi, wi)
                    if asks[i - 1] or want[ni][0]:
                        gprev = train_dz(ni, ci, gi, 1, si, ge["dz_c%d" % i], hi, wi)            # the later dz has been consumed (stream order)
                    train_params(ni, ci, xi, 1, cx, cx, hx, wx, gprev, 1, si)
                else:
                    sums_i = gate(gi, ei, B, hi, wi, ci.cout, 1, 1, want[ni][1] or want[ni][2])
                    params(ni, ci, xi, 1, cx, cx, hx, wx, gi, 1, sums_i)
                stop = not asks[i - 1]
            if stop:
                break
            # the identity / down-sample branch's gradient first, the main branch's data gradient adds it in its epilogue (fixed order)
            if down is not None:
                dgrad(nd, down, gd, 1, None, ge["tmp"], 1, cin, cin, hin, win)
                other = ge["tmp"]
            else:
                other = g_out
            dgrad(cn[0], convs[0], gprev, 1, other, g_in, 1, cin, cin, hin, win)
        else:
            stem = prep["stem"]
            hs, wst = fs["stem"].shape[1], fs["stem"].shape[2]
            _capi.call("hps_maxpool3x3s2_backward", P(fs["stem"]), P(gf["pool"]), P(gf["stem"]), B, hs, wst, stem.cout, 1, s)
            g0 = gf["stem"]
            if trains("stem"):
                if needs[0] or any(want["stem"]):
                    s0 = train_sums("stem", stem, gf["stem"], 0, fs["stem"], 0, hs, wst)
                    if needs[0] or want["stem"][0]:
                        g0 = train_dz("stem", stem, gf["stem"], 0, s0, gf["dz_stem"], hs, wst)
                    if want["stem"][0]:
                        _capi.call("hps_nchw_to_padded_nhwc_generic", P(x), P(gf["xin"]), B, C, C, H, W, W, 3, s)
                    train_params("stem", stem, gf["xin"], 3, C, C, H, W, g0, 0, s0)
            else:
                sums0 = gate(gf["stem"], fs["stem"], B, hs, wst, stem.cout, 0, 0, want["stem"][1] or want["stem"][2])
                if want["stem"][0] or want["stem"][1]:
                    _capi.call("hps_nchw_to_padded_nhwc_generic", P(x), P(gf["xin"]), B, C, C, H, W, W, 3, s)
                params("stem", stem, gf["xin"], 3, C, C, H, W, gf["stem"], 0, sums0)
            if needs[0]:
                dx = torch.empty(B, H, W, C, device=dev, dtype=torch.float32)
                dgrad("stem", stem, g0, 0, None, dx, 0, C, C, H, W)
                grads["input"] = dx.permute(0, 3, 1, 2).contiguous()
        out = []
        for name, _, _ in layers:
            out += list(grads.get(name, (None, None, None)))
        return grads.get("input"), out


def resnet18(in_channels, pretrained=False, progress=True, **kwargs):
    """models/resnet.py:229-237 (pretrained ImageNet weights are never used by the reference's nets)."""
    if pretrained:
        raise NotImplementedError("no network access: pretrained weights are not available")
    return ResNet([2, 2, 2, 2], in_channels)


def resnet50(in_channels, pretrained=False, progress=True, **kwargs):
    """models/resnet.py:251-259 (Bottleneck, [3, 4, 6, 3], 2048 features); forward only until set_differentiable(True) opts in to the
    backward, training-mode BatchNorm and the in-place refresh (see ResNet)."""
    if pretrained:
        raise NotImplementedError("no network access: pretrained weights are not available")
    return ResNet([3, 4, 6, 3], in_channels, block=Bottleneck)
