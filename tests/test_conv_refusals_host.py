"""What the nine convolution entry points refuse, and with which MAGNET_E_* code and message, is part of their contract: every case of
tests/golden/conv_refusals.json (348 refused argument sets recorded by tests/golden/make_conv_refusals.py from the library before the
entry points were routed through one launcher: every fail(...) site of conv_mfma_run, of the entry points and of their shared checks once
per entry point that reaches it, and 18 two-violation cases that pin the order where the codes differ) is replayed against the current
library.  No GPU needed, and none wanted: the argument sets hold fake pointers, so the test skips itself where a device is visible."""
import importlib.util
import json
import os

import pytest

from magnet_amd import lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _generator():
    spec = importlib.util.spec_from_file_location("make_conv_refusals", os.path.join(GOLDEN, "make_conv_refusals.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_recorded_refusal_is_refused_alike(hip_lib):
    L = hip_lib
    if L.magnet_device_count() != 0:
        pytest.skip("a GPU is visible: a wrongly accepted argument set would launch on fake pointers")
    gen = _generator()
    with open(os.path.join(GOLDEN, "conv_refusals.json")) as f:
        cases = json.load(f)["cases"]
    assert len(cases) == 348 and {c["entry"] for c in cases} == set(gen.BASES)
    bad = []
    for c in cases:
        assert 0 < c["code"] <= lib.E_SHAPE, f"{c['entry']} / {c['name']}: the file holds a call that is not a refusal"
        rc, msg = gen.replay(L, c["entry"], c["set"], c["call"])      # msg: what magnet_last_error() answers after the call
        code = -rc if c["entry"].endswith("_workspace") else rc
        what = f"{c['entry']} / {c['name']}"
        if code <= 0:
            bad.append(f"{what}: accepted, expected code {c['code']} ({c['message']!r})")
        elif code != c["code"]:
            bad.append(f"{what}: code {code} ({msg!r}), expected {c['code']} ({c['message']!r})")
        elif c["exact"] and msg != c["message"]:
            bad.append(f"{what}: message {msg!r}, expected {c['message']!r}")
        elif not c["exact"] and not (msg.startswith(c["who"] + ":") and c["word"] in msg):
            bad.append(f"{what}: message {msg!r} must begin with {c['who'] + ':'!r} and name {c['word']!r}")
    assert not bad, "\n".join(bad)
