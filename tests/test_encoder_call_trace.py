"""CPU: the encoder's forward issues the launches, arguments and buffers of tests/golden/encoder_call_traces.json -- recorded before
the forward was rebuilt around one plan (tests/golden/make_encoder_call_traces.py) -- in every kernel mode, as one hps_encoder_run
call and launch by launch through the public entry points, and with training-mode BatchNorm."""
import json
import os

import pytest

import encoder_call_trace as T

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encoder_call_traces.json")) as f:
    GOLDEN = json.load(f)


def check(rows, name):
    want = GOLDEN[name]
    rows = json.loads(json.dumps(rows))
    for i, (got, exp) in enumerate(zip(rows, want)):
        assert got == exp, "%s: launch %d" % (name, i)
    assert len(rows) == len(want), name


def test_golden_covers_the_configurations():
    assert set(GOLDEN) == set(T.EVAL_CONFIGS) | set(T.TRAIN_CONFIGS)


@pytest.mark.parametrize("composite", [True, False], ids=["one_call", "per_launch"])
@pytest.mark.parametrize("name", list(T.EVAL_CONFIGS))
def test_eval_forward_launches(monkeypatch, name, composite):
    check(T.eval_trace(monkeypatch, name, composite), name)


@pytest.mark.parametrize("name", list(T.TRAIN_CONFIGS))
def test_training_forward_launches(monkeypatch, name):
    check(T.train_trace(monkeypatch, name), name)


def test_per_launch_mode_calls_the_public_entry_points(monkeypatch):
    """composite = False must stay a check of csrc/composite.hip's argument mapping: it never goes through hps_encoder_run."""
    seen = []
    real = T.Recorder.call
    monkeypatch.setattr(T.Recorder, "call", lambda self, entry, *args: (seen.append(entry), real(self, entry, *args))[1])
    T.eval_trace(monkeypatch, "default", composite=False)
    assert "hps_encoder_run" not in seen and len(seen) == len(GOLDEN["default"])
    del seen[:]
    T.eval_trace(monkeypatch, "default", composite=True)
    assert seen == ["hps_encoder_run"]
