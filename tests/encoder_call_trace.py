"""Records what the encoder asks libhps to launch, on a CPU-resident encoder and without a device: one row per launch with the entry
point's name, its scalar arguments and every pointer argument as ``p<k>``, k being the order in which that address first appeared
in the trace -- so a trace also says which buffer each launch reads and writes relative to the others.  The stream argument is
dropped.  An ``hps_encoder_run`` call is expanded into the rows of its ops by KIND_ENTRY below, which restates the switch of
csrc/composite.hip on purpose (it is NOT the package's table: a wrong table there must show up as a mismatch).  ``gate`` / ``fill``
rows mark where the pipeline's callbacks ran.

tests/golden/make_encoder_call_traces.py writes the traces of CONFIGS to tests/golden/encoder_call_traces.json;
tests/test_encoder_call_trace.py compares against that file."""
import contextlib
import ctypes

import torch

from hierarchicalprobabilistic3dhuman_amd import _capi
from hierarchicalprobabilistic3dhuman_amd.resnet import resnet18

# csrc/composite.hip, hps_encoder_run: op kind -> (entry point, the op's fields in the order of the entry's arguments)
KIND_ENTRY = {
    0: ("hps_nchw_to_padded_nhwc", "x y B Cin H W opad"),
    7: ("hps_nchw_to_padded_nhwc_generic", "x y B Cin Cout H W KW opad"),
    1: ("hps_conv2d_bn_act_pad", "x w scale shift residual y B H W ipad Cin Cout KH KW stride pad opad relu row_mode variant ksplit splitk_ws"),
    10: ("hps_conv2d_bn_act_pad_down", "x w scale shift y w_down scale_down shift_down y_down B H W ipad Cin Cout KH KW stride pad opad relu "
                                       "variant ksplit splitk_ws"),
    4: ("hps_conv3x3_winograd", "x w scale shift residual y B H W ipad Cin Cout opad relu splitk_ws"),
    5: ("hps_stem_phase_split", "x y B Cin H W"),
    6: ("hps_stem_winograd", "x w scale shift y B H W opad relu"),
    8: ("hps_stem_winograd_pooled", "x w scale shift y splitk_ws B H W opad relu"),
    9: ("hps_stem_winograd_pooled_nchw", "x w scale shift y splitk_ws B H W opad relu"),
    2: ("hps_maxpool3x3s2_pad", "x y B H W Cin opad"),
    3: ("hps_global_avgpool_pad", "x y B H W Cin ipad"),
}
POINTER_FIELDS = {"x", "w", "scale", "shift", "residual", "y", "splitk_ws", "w_down", "scale_down", "shift_down", "y_down"}


class _FakeStream:
    cuda_stream = 0

    def wait_event(self, event):
        pass


class _FakeEvent:
    def record(self, stream=None):
        pass


class Recorder:
    def __init__(self):
        self.rows, self.names, self.keep = [], {}, []

    def name(self, address):
        if isinstance(address, ctypes.c_void_p):
            address = address.value
        if not address:
            return None
        return self.names.setdefault(address, "p%d" % len(self.names))

    def ptr(self, t, dtype=torch.float32, what="tensor"):
        if t is None:
            return None
        assert t.dtype == dtype and t.is_contiguous(), what
        self.keep.append(t)                       # alive until the trace ends: no address is handed out twice
        return ctypes.c_void_p(t.data_ptr())

    def call(self, entry, *args):
        if entry == "hps_encoder_run":
            ops, n = args[0], args[1]
            for i in range(n):
                name, fields = KIND_ENTRY[ops[i].kind]
                self.rows.append([name] + [self.name(getattr(ops[i], f)) if f in POINTER_FIELDS else int(getattr(ops[i], f))
                                           for f in fields.split()])
            return
        types = _capi._PROTOTYPES[entry]          # the C signature: which arguments are pointers
        assert len(args) == len(types), entry
        row = [entry]
        for a, t in zip(args[:-1], types[:-1]):   # the last argument is the stream
            if t is ctypes.c_void_p:
                row.append(self.name(a))
            else:
                assert a is not None and not isinstance(a, ctypes.c_void_p), entry
                row.append(a)
        self.rows.append(row)

    def mark(self, what):
        return lambda: self.rows.append([what])


@contextlib.contextmanager
def recording(monkeypatch):
    """Inside the block the package's calls into libhps are recorded instead of made; host-side size queries still reach the library."""
    rec = Recorder()
    with monkeypatch.context() as m:
        m.setattr(_capi, "call", rec.call)
        m.setattr(_capi, "ptr", rec.ptr)
        m.setattr(_capi, "stream", lambda: ctypes.c_void_p(0))
        m.setattr(_capi, "require_device", lambda t, what="tensor": None)
        m.setattr(torch.cuda, "current_stream", lambda device=None: _FakeStream())
        m.setattr(torch.cuda, "Event", _FakeEvent)
        yield rec


# name -> (input shape, switches, how the encoder is driven)
EVAL_CONFIGS = {
    "default": ((2, 18, 256, 256), {}),
    "stem_from_frames": ((2, 18, 256, 256), {"stem_reads_nchw": False}),
    "stem_from_frames_unfused_pool": ((2, 18, 256, 256), {"stem_reads_nchw": False, "fused_pool": False}),
    "unfolded_downsample": ((2, 18, 256, 256), {"fold_downsample": False}),
    "no_winograd": ((2, 18, 256, 256), {"winograd": False}),
    "latency": ((2, 18, 256, 256), {"latency": True}),
    "winograd_stem_direct_layers": ((1, 18, 64, 96), {}),
    "generic_relayout_row_stem": ((2, 18, 130, 67), {}),
    "channel_padded": ((2, 3, 65, 47), {}),
    # the inference pipeline's hooks: where the gate and the caller's fill of the phase frames run among the launches
    "default_gated": ((2, 18, 256, 256), {"gate": True}),
    "stem_from_frames_gated": ((2, 18, 256, 256), {"stem_reads_nchw": False, "gate": True}),
    "generic_relayout_gated": ((2, 18, 130, 67), {"gate": True}),
    "filled_frames_gated": ((2, 18, 256, 256), {"gate": True, "filled": True}),
    "filled_frames": ((2, 18, 256, 256), {"filled": True}),
}
TRAIN_CONFIGS = {
    "train_all": {},
    "train_layer1_eval": {"layer1_eval": True},
    "train_unfolded_downsample": {"fold_downsample": False},
    "training_activations": {"activations": True},
}
TRAIN_SHAPE = (2, 18, 64, 96)


def _encoder(channels):
    torch.manual_seed(0)
    return resnet18(in_channels=channels).eval()


def eval_trace(monkeypatch, name, composite):
    shape, opt = EVAL_CONFIGS[name]
    enc = _encoder(shape[1])
    enc.composite = composite
    for switch in ("stem_reads_nchw", "fused_pool", "fold_downsample"):
        if switch in opt:
            setattr(enc, switch, opt[switch])
    if "winograd" in opt:
        enc.set_winograd(opt["winograd"])
    if "latency" in opt:
        enc.set_latency_mode(opt["latency"])
    x = torch.rand(*shape, generator=torch.Generator().manual_seed(1))
    with recording(monkeypatch) as rec, torch.no_grad():
        gate = rec.mark("gate") if opt.get("gate") else None
        if opt.get("filled"):
            x = enc.stem_frames(*shape, x.device)
            x.fill = rec.mark("fill")
        enc(x, _gate=gate)
    return rec.rows


def train_trace(monkeypatch, name):
    opt = TRAIN_CONFIGS[name]
    enc = _encoder(TRAIN_SHAPE[1])
    enc.fold_downsample = opt.get("fold_downsample", True)
    enc.set_batchnorm_training(True)
    enc.train()
    if opt.get("layer1_eval"):
        enc.layer1.eval()
    x = torch.rand(*TRAIN_SHAPE, generator=torch.Generator().manual_seed(1))
    with recording(monkeypatch) as rec, torch.no_grad():
        enc.training_activations(x) if opt.get("activations") else enc(x)
    return rec.rows
