"""Record what the three layout-pack entry points answer to refused argument sets: tests/golden/pack_refusals.json.

    python tests/golden/make_pack_refusals.py LIBRARY [out.json]

LIBRARY is the libmagnet_hip.so whose behaviour is to be pinned: the one built in a checkout of the parent commit (python -m
magnet_amd.build there), on a machine without a GPU.  It is loaded in place of this tree's own, as tests/golden/make_conv_refusals.py
does and for its reason.  Every case is the valid base argument set of its entry point (fake 16-aligned pointers, small dimensions)
with the arguments of `set` replaced, so that one rule is violated: every fail(...) site of magnet_pack_features, magnet_pack_split
and magnet_pack_f16, each condition of a site once.  The cases named "two: ..." violate two rules and pin the order of
the checks.  Recorded per case: the MAGNET_E_* code and magnet_last_error(), which the replay compares byte for byte.  Only refusals are
written, since replaying an accepted call on a machine with a GPU would launch on fake pointers; a case marked MAYBE is one the
entry point may accept (magnet_pack_split takes a negative in_img_stride), tried and kept only if it is refused.
tests/test_pack_refusals_host.py replays the file against the current library."""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from magnet_amd import lib  # noqa: E402

P, ODD = 16, 24                                                        # a fake 16-aligned pointer, and one that is only 8-aligned
# entry point -> its arguments before the stream, in call order, with a valid value each
BASES = {
    "magnet_pack_features": dict(nchw=P, out_cl=P, N=2, F=16, h=4, w=6, out_dtype=lib.FEAT_F32, pad=0),
    "magnet_pack_split": dict(nchw=P, out_hi=P, out_lo=P, N=2, C=16, h=4, w=6, ctot=32, c_off=8, in_img_stride=0),
    "magnet_pack_f16": dict(nchw=P, out_f16=P, N=2, C=16, h=4, w=6, ctot=32, c_off=8, in_img_stride=0),
}
MAYBE = "maybe"
DIMS = [(f"{d} 0", {d: 0}) for d in "Nhw"] + [(f"{d} -1", {d: -1}) for d in "Nhw"]
SLICE = [                                                              # the channel slice of split and f16: granule 8, round-up lanes inside ctot
    ("C 0", {"C": 0}), ("C -8", {"C": -8}), ("c_off 4", {"c_off": 4}), ("c_off -8", {"c_off": -8}), ("ctot 36", {"ctot": 36}),
    ("c_off + C over ctot", {"c_off": 24}), ("round-up lanes over ctot", {"C": 17, "c_off": 16}),
]
CASES = {
    "magnet_pack_features": [
        ("nchw NULL", {"nchw": None}), ("out_cl NULL", {"out_cl": None}), *DIMS, ("F 0", {"F": 0}), ("F -8", {"F": -8}), ("F 12", {"F": 12}),
        ("out_dtype 7", {"out_dtype": 7}), ("out_dtype -1", {"out_dtype": -1}), ("pad 2", {"pad": 2}), ("pad -1", {"pad": -1}),
        ("out_cl misaligned", {"out_cl": ODD}),
        ("two: nchw NULL, N 0", {"nchw": None, "N": 0}), ("two: F 12, out_dtype 7", {"F": 12, "out_dtype": 7}),
        ("two: out_dtype 7, pad 2", {"out_dtype": 7, "pad": 2}), ("two: pad 2, out_cl misaligned", {"pad": 2, "out_cl": ODD}),
    ],
    "magnet_pack_split": [
        ("nchw NULL", {"nchw": None}), ("out_hi NULL", {"out_hi": None}), ("out_lo NULL", {"out_lo": None}), *DIMS, *SLICE,
        ("out_hi misaligned", {"out_hi": ODD}), ("out_lo misaligned", {"out_lo": ODD}),
        ("in_img_stride -4", {"in_img_stride": -4}, MAYBE), ("rows 2^31", {"N": 1 << 20, "h": 46, "w": 46}, MAYBE),
        ("two: out_lo NULL, c_off 4", {"out_lo": None, "c_off": 4}), ("two: ctot 36, out_hi misaligned", {"ctot": 36, "out_hi": ODD}),
    ],
    "magnet_pack_f16": [
        ("nchw NULL", {"nchw": None}), ("out_f16 NULL", {"out_f16": None}), *DIMS, *SLICE, ("in_img_stride -4", {"in_img_stride": -4}),
        ("rows 2^31", {"N": 1 << 20, "h": 46, "w": 46}), ("out_f16 misaligned", {"out_f16": ODD}),
        ("two: nchw NULL, c_off 4", {"nchw": None, "c_off": 4}), ("two: in_img_stride -4, out_f16 misaligned", {"in_img_stride": -4, "out_f16": ODD}),
    ],
}


def replay(L, entry, overrides):
    """Call `entry` of the loaded library L with its base arguments, `overrides` replaced, on the null stream.
    Returns (answer, the bytes of magnet_last_error())."""
    args = {**BASES[entry], **overrides}
    assert set(args) == set(BASES[entry]), (entry, overrides)
    rc = getattr(L, entry)(*args.values(), None)
    return int(rc), bytes(L.magnet_last_error())


def main(library, out):
    lib.LIB_PATH = os.path.abspath(library)                            # before the first load(): the library to record, not this tree's
    L = lib.load()
    assert L._name == lib.LIB_PATH, (L._name, lib.LIB_PATH)
    assert L.magnet_device_count() == 0, "run this on a machine without a GPU: the base argument sets hold fake pointers"
    cases = []
    for entry in BASES:                                                # the base sets are valid: accepted (then no device to launch on), and not recorded
        rc, msg = replay(L, entry, {})
        assert rc < 0, f"{entry}: the base set is refused: {rc} {msg!r}"
    for entry, own in CASES.items():
        for name, overrides, *maybe in own:
            rc, msg = replay(L, entry, overrides)
            if maybe and rc < 0:
                print(f"{entry} / {name}: accepted, not recorded")
                continue
            assert 0 < rc <= lib.E_SHAPE, f"{entry} / {name}: answered {rc} ({msg!r}): not a refusal"
            assert msg.startswith(entry.encode() + b":"), (entry, name, msg)
            cases.append({"entry": entry, "name": name, "set": overrides, "code": rc, "message": msg.decode("latin-1")})
    ids = [(c["entry"], c["name"]) for c in cases]
    assert len(ids) == len(set(ids))
    with open(out, "w") as f:
        f.write('{"cases": [\n' + ",\n".join(json.dumps(c, sort_keys=True) for c in cases) + "\n]}\n")      # one case per line
    print(f"{len(cases)} refusals of {lib.LIB_PATH} -> {out}")
    print({e: sum(c["entry"] == e for c in cases) for e in BASES})


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "pack_refusals.json"))
