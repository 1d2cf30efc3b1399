"""Writes tests/golden/encoder_call_traces.json: the launches of the encoder's forward (tests/encoder_call_trace.py) for the
configurations tests/test_encoder_call_trace.py checks.  It drives the encoder through its public API only, so it runs at any
commit; the committed file was recorded at 3cee304, the commit before the forward's three walks over the network became one
plan, and is the statement of "same launches, same arguments, same order" -- do not regenerate it from the code under test.

    python tests/golden/make_encoder_call_traces.py
"""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import encoder_call_trace as T  # noqa: E402


def main():
    mp = pytest.MonkeyPatch()
    traces = {}
    for name in T.EVAL_CONFIGS:
        rows = T.eval_trace(mp, name, composite=True)
        assert rows == T.eval_trace(mp, name, composite=False), name       # one call or launch by launch: the same launches
        traces[name] = rows
    for name in T.TRAIN_CONFIGS:
        traces[name] = T.train_trace(mp, name)
    path = os.path.join(HERE, "encoder_call_traces.json")
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(
            '"%s": [\n%s\n]' % (name, ",\n".join(json.dumps(row, separators=(",", ":")) for row in rows)) for name, rows in traces.items()) + "\n}\n")
    for name, rows in traces.items():
        print("%-34s %3d rows" % (name, len(rows)))
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
