"""One owner and one validity rule for the device data a module derives from its parameters and kernel switches."""
import torch
from torch import nn


class DeviceStateModule(nn.Module):
    """An nn.Module that keeps ALL device data derived from its parameters and kernel switches -- folded weights, pointer tables,
    activation frames, launch lists, index tables -- in ONE dict, ``device_state()``.  Entries are only ever added to that dict;
    every reset REPLACES it (invalidate()): after .to(), after a load_state_dict that reaches the module (directly or through a
    parent), when an attribute named in SWITCHES gets a new value, and in copies / pickles (they carry no device state).

    The dict is therefore the validity token of everything built from it: a recorded launch sequence (a hipGraph) is stale exactly
    when ``device_state()`` returns another object, and holding the old dict keeps every tensor the sequence points at alive."""

    SWITCHES = ()

    def __init__(self):
        super().__init__()
        self.invalidate()
        self.register_load_state_dict_post_hook(DeviceStateModule.invalidate)

    def device_state(self):
        return self._device_state

    def invalidate(self, *_):
        """Drop the derived device state; the next forward rebuilds it from the current parameters and switches.  Call it by hand
        after editing parameters in place (PoseMFShapeGaussianNet does it itself for its head parameters once it has run a
        differentiable forward: it compares their version counters on every forward).  (Also the load_state_dict post hook: nn.Module.load_state_dict recurses with
        _load_from_state_dict and never calls a child's load_state_dict, but it runs the children's post hooks.)"""
        self._device_state = {}

    @property
    def _prepared(self):
        """The kernel-side weights of the current device state (prepare()), None before they are built."""
        return self._device_state.get("prep")

    @_prepared.setter
    def _prepared(self, prep):
        if self._device_state:                # new weights: whatever the state holds points at the old ones
            self.invalidate()
        self._device_state["prep"] = prep

    def _derived(self, kind, key, build, limit=4):
        """Entry ``key`` of one ``kind``, built by ``build()`` on the current stream at first use.  A use on another stream waits for
        the build once (an event recorded behind it); later uses issue nothing.  At most ``limit`` entries per kind: one more starts a
        new state that keeps the other kinds (the old state stays intact for whoever holds it)."""
        entries = self._device_state.setdefault(kind, {})
        entry = entries.get(key)
        stream = torch.cuda.current_stream()
        if entry is None:
            if len(entries) >= limit:
                kept = {k: v for k, v in self._device_state.items() if k != kind}
                self.invalidate()
                self._device_state.update(kept)
                entries = self._device_state[kind] = {}
            value = build()
            built = torch.cuda.Event()
            built.record(stream)
            entry = entries[key] = (value, built, {stream.cuda_stream})
        elif stream.cuda_stream not in entry[2]:
            stream.wait_event(entry[1])
            entry[2].add(stream.cuda_stream)
        return entry[0]

    def __setattr__(self, name, value):
        if name in self.SWITCHES and name in self.__dict__ and self.__dict__[name] != value:
            self.invalidate()
        super().__setattr__(name, value)

    def _apply(self, fn, *args, **kwargs):
        self.invalidate()
        return super()._apply(fn, *args, **kwargs)

    def __getstate__(self):
        state = super().__getstate__()
        state["_device_state"] = {}
        return state
