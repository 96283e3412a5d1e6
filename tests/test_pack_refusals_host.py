"""What magnet_pack_features, magnet_pack_split and magnet_pack_f16 refuse, with which MAGNET_E_* code and which
message, is part of their contract: every case of tests/golden/pack_refusals.json (recorded by tests/golden/make_pack_refusals.py from
the library before the packs' checks were stated once: every fail(...) site of the three entry points, each of its conditions, and the
two-violation cases that pin the order of the checks) is replayed against the current library: equal codes, equal bytes.  No GPU
needed, and none wanted: the argument sets hold fake pointers, so the test skips itself where a device is visible."""
import importlib.util
import json
import os

import pytest

from magnet_amd import lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _generator():
    spec = importlib.util.spec_from_file_location("make_pack_refusals", os.path.join(GOLDEN, "make_pack_refusals.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_recorded_pack_refusal_is_refused_alike(hip_lib):
    L = hip_lib
    if L.magnet_device_count() != 0:
        pytest.skip("a GPU is visible: a wrongly accepted argument set would launch on fake pointers")
    gen = _generator()
    with open(os.path.join(GOLDEN, "pack_refusals.json")) as f:
        cases = json.load(f)["cases"]
    assert len(cases) == 60 and {c["entry"] for c in cases} == set(gen.BASES)
    recorded = {(c["entry"], c["name"]) for c in cases}
    for entry, own in gen.CASES.items():                              # the file is the generator's: every case that is not a "maybe" is in it
        assert all((entry, name) in recorded for name, _, *maybe in own if not maybe), entry
    bad = []
    for c in cases:
        assert 0 < c["code"] <= lib.E_SHAPE, f"{c['entry']} / {c['name']}: the file holds a call that is not a refusal"
        rc, msg = gen.replay(L, c["entry"], c["set"])                 # msg: the bytes magnet_last_error() answers after the call
        what = f"{c['entry']} / {c['name']}"
        if rc <= 0:
            bad.append(f"{what}: accepted, expected code {c['code']} ({c['message']!r})")
        elif rc != c["code"]:
            bad.append(f"{what}: code {rc} ({msg!r}), expected {c['code']} ({c['message']!r})")
        elif msg != c["message"].encode("latin-1"):
            bad.append(f"{what}: message {msg!r}, expected {c['message']!r}")
    assert not bad, "\n".join(bad)
