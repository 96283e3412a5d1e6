"""Record what the nine convolution entry points answer to refused argument sets: tests/golden/conv_refusals.json.

    python tests/golden/make_conv_refusals.py LIBRARY [out.json]

LIBRARY is the libmagnet_hip.so whose behaviour is to be pinned: the one built in a checkout of the parent commit (python -m
magnet_amd.build there), on a machine without a GPU.  It is named on the command line and loaded in place of this tree's own, because
this script imports magnet_amd.lib (the ctypes mirrors and prototypes, which an unchanged ABI shares) from the tree it lies in, and
would otherwise record the code under test.  (After a change of MagnetConvArgs the mirrors no longer fit the parent's library: then this
tree's library is recorded and the new file compared with the old one case by case, as profiles/retire_mx/NOTES.md did.)  Besides that it needs ctypes only.  Every case is a valid base argument set of its entry point (fake 16-aligned pointers, small dimensions, as
tests/test_splitk_host.py builds its own) with the fields of `set` overridden and the call arguments of `call` replaced, so that one
rule is violated (two in the cases named "two: ...", which pin the order of checks whose codes differ).  Recorded per case: the
MAGNET_E_* code (the workspace queries answer its negative), magnet_last_error(), `exact` = the message comes from conv_mfma_run's
checks of the common fields and is pinned byte for byte; for the others `who` = the name the message begins with and `word` = what it
must keep naming.  Only refusals are written: an accepted call has no place in the file, since replaying it on a machine with a GPU would launch on fake pointers.
tests/test_conv_refusals_host.py replays the file against the current library."""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from magnet_amd import lib  # noqa: E402

P, BIG = 16, 1 << 30                                                   # a fake aligned pointer; a workspace size that is always enough
F16 = {"base.in_lo": None, "base.w_lo": None}
# entry point -> (overrides of the common base that make a valid call of it, its call arguments besides the struct and the stream)
BASES = {
    "magnet_conv_mfma": ({}, {}),
    "magnet_conv_mfma_ex": ({}, {}),
    "magnet_conv_mfma_f16": ({**F16, "base.cout_pad": 128}, {}),
    "magnet_conv_mfma_f16p": ({**F16, "base.cout_pad": 128}, {}),
    "magnet_conv_mfma_splitk_workspace": ({}, {"split_k": 2}),
    "magnet_conv_mfma_splitk": ({}, {"split_k": 2, "work": P, "work_bytes": BIG}),
    "magnet_conv_mfma_f16d": (F16, {}),
    "magnet_conv_mfma_f16d_splitk_workspace": (F16, {"split_k": 2}),
    "magnet_conv_mfma_f16d_splitk": (F16, {"split_k": 2, "work": P, "work_bytes": BIG}),
}
LAUNCHES = [e for e in BASES if not e.endswith("_workspace")]
TAIL = {"base.tail_w_hi": P, "base.tail_w_lo": P, "base.tail_bias": P, "base.cout_pad": 128}
GRID = {"base.rows": 510, "base.wp": 17, "base.up_B": 1, "base.up_h": 28, "base.up_w": 15}     # 1 x (28 + 2) x (15 + 2) = 510 rows

# the fail(...) sites of conv_mfma_run, in its order: (name, overrides); tried on every launch entry point and kept where the
# message is conv_mfma_run's (an entry point's own check may come first: those sites are in OWN below)
COMMON = [
    ("in_hi NULL", {"base.in_hi": None}),
    ("in_lo NULL", {"base.in_lo": None}),
    ("out_mode 5", {"base.out_mode": 5}),
    ("out_mode 0 (f16p)", {"base.out_mode": 0, "base.out_hi": P}),
    ("out_mode 5 behind a tail", {**TAIL, "base.tail_cout_pad": 16, "base.out_mode": 5}),
    ("tail without tail_w_lo", {**TAIL, "base.tail_cout_pad": 16, "base.tail_w_lo": None}),
    ("tail without any output", {**TAIL, "base.tail_cout_pad": 16, "base.out_f32": None}),
    ("tail at cout_pad 256", {**TAIL, "base.tail_cout_pad": 16, "base.cout_pad": 256}),
    ("tail_w_hi misaligned", {**TAIL, "base.tail_cout_pad": 16, "base.tail_w_hi": 24}),
    ("tail with border", {**TAIL, "base.tail_cout_pad": 16, "base.border_hp": 30, "base.border_pad": 1}),
    ("out_f32 NULL", {"base.out_f32": None}),
    ("rows 0", {"base.rows": 0}),
    ("cin 16", {"base.cin": 16}),
    ("taps 2", {"base.taps": 2}),
    ("taps 9 without wp", {"base.wp": 0}),
    ("cout_pad 48", {"base.cout_pad": 48}),
    ("in_hi misaligned", {"base.in_hi": 24}),
    ("out_f32 misaligned", {"base.out_f32": 24}),
    ("dil 9", {"base.dil": 9}),
    ("addend misaligned", {"base.addend": 24}),
    ("addend_ld 100", {"base.addend": P, "base.addend_ld": 100}),
    ("in_ld 100", {"base.in_ld": 100}),
    ("row window over 2 GiB", {"base.in_ld": 4000000}),
    ("out_ld 100", {"base.out_ld": 100}),
    ("add_hi without add_lo", {"base.add_hi": P}),
    ("add_hi misaligned", {"base.add_hi": 24, "base.add_lo": P}),
    ("add_hi misaligned (one plane)", {"base.add_hi": 24}),
    ("add_ld 100", {"base.add_hi": P, "base.add_lo": P, "base.add_ld": 100}),
    ("addend and add_hi", {"base.addend": P, "base.add_hi": P, "base.add_lo": P}),
    ("border_hp 7", {"base.border_hp": 7, "base.border_pad": 1}),
    ("border_hp * wp 2^24", {"base.border_hp": 1 << 20, "base.border_pad": 1, "base.rows": 17 << 20}),
    ("repad without border_hp", {"base.repad": 1}),
    ("up_out without up_depth", {"base.up_out": P}),
    ("upsampling without a tail", {"base.up_out": P, "base.up_depth": P}),
    ("upsampling with bad dims", {**TAIL, **GRID, "base.tail_cout_pad": 144, "base.up_out": P, "base.up_depth": P, "base.up_npred": 1, "base.up_h": 27}),
    ("up_out misaligned", {**TAIL, **GRID, "base.tail_cout_pad": 144, "base.up_out": 24, "base.up_depth": P, "base.up_npred": 1}),
    ("gu_out without gu_in", {"base.gu_out": P}),
    ("gu_in aliases gu_out", {"base.gu_in": P, "base.gu_out": P}),
    ("Gaussian update without a tail", {"base.gu_in": P, "base.gu_out": 32}),
    ("Gaussian update with bad dims", {**TAIL, **GRID, "base.tail_cout_pad": 16, "base.gu_in": P, "base.gu_out": 32, "base.up_w": 14}),
]

LEAKY = {"act": lib.ACT_LEAKY_RELU, "act_slope": 0.01}
PLANES = [(f, {"base." + f: P}, f) for f in ("in_lo", "w_lo")]
ACT = [("act 7", {"act": 7}, "act"), ("LeakyReLU with relu", {**LEAKY, "base.relu": 1}, "relu"), ("act_slope 1e38", {**LEAKY, "act_slope": 1e38}, "act_slope")]
FUSED = [("tail_w_hi", {"base.tail_w_hi": P}, "fused tail"), ("tail_w_lo", {"base.tail_w_lo": P}, "fused tail"), ("addend", {"base.addend": P}, "addend"),
         ("up_out", {"base.up_out": P}, "upsampling"), ("up_depth", {"base.up_depth": P}, "upsampling"), ("gu_in", {"base.gu_in": P}, "Gaussian update"),
         ("gu_out", {"base.gu_out": P}, "Gaussian update")]
SPLITK_FORM = [
    ("split_k 1", {}, {"split_k": 1}, "split_k"), ("split_k 9", {}, {"split_k": 9}, "split_k"), ("split_k -1", {}, {"split_k": -1}, "split_k"),
    *[(n, s, {}, w) for n, s, w in FUSED],
    ("add_hi", {"base.add_hi": P}, {}, "residual input"), ("add_lo", {"base.add_lo": P}, {}, "residual input"),
    ("tiling BM256", {"tiling": lib.TILING_BM256}, {}, "tiling"), ("tiling BM64", {"tiling": lib.TILING_BM64}, {}, "tiling"), ("tiling 8", {"tiling": 8}, {}, "tiling"),
    ("taps 4", {"base.taps": 4}, {}, "taps"), ("cout_pad 64", {"base.cout_pad": 64}, {}, "cout_pad"), ("cout_pad 144", {"base.cout_pad": 144}, {}, "cout_pad"),
    ("out_mode 2", {"base.out_mode": 2, "base.out_hi": P}, {}, "out_mode"), ("rows 0", {"base.rows": 0}, {}, "rows"), ("cin 176", {"base.cin": 176}, {}, "cin"),
    ("one chunk per split", {}, {"split_k": 3}, "chunks"), ("rows 2^31", {"base.rows": 1 << 31}, {}, "rows"),
]
SPLITK_CALL = [
    ("work NULL", {}, {"work": None}, "work"), ("work misaligned", {}, {"work": 24}, "work"), ("work_bytes short", {}, {"work_bytes": 2 * 510 * 256 * 4 - 1}, "work_bytes"),
    *[(n, s, {}, w) for n, s, w in ACT],
]
F16D_FORM = [
    *[(n, s, {}, w) for n, s, w in PLANES], ("add_hi", {"base.add_hi": P}, {}, "add_hi"), ("add_lo", {"base.add_lo": P}, {}, "add_lo"),
    *[(n, s, {}, w) for n, s, w in ACT], ("tiling BM256", {"tiling": lib.TILING_BM256}, {}, "tiling"), *[(n, s, {}, w) for n, s, w in FUSED],
    ("taps 4", {"base.taps": 4}, {}, "taps"), ("dil 2", {"base.dil": 2}, {}, "dil"), ("cout_pad 64", {"base.cout_pad": 64}, {}, "cout_pad"),
    ("out_mode 2", {"base.out_mode": 2, "base.out_hi": P}, {}, "out_mode"),
]
NULL_ARGS = ("args NULL", {}, {"args": None}, "args is NULL")
# the fail(...) sites of the entry points themselves: entry point -> [(name, overrides, call overrides, word)]
OWN = {
    "magnet_conv_mfma": [NULL_ARGS],
    "magnet_conv_mfma_ex": [
        NULL_ARGS, *[(n, s, {}, w) for n, s, w in ACT], ("LeakyReLU with a tail", {**LEAKY, **TAIL, "base.tail_cout_pad": 16}, {}, "tail"),
        ("tiling 8", {"tiling": 8}, {}, "tiling"), ("BM64 with BM256", {"tiling": lib.TILING_BM64 | lib.TILING_BM256}, {}, "MAGNET_TILING_BM256"),
        ("BM64 at taps 1", {"tiling": lib.TILING_BM64, "base.taps": 1}, {}, "taps"), ("BM64 at cout_pad 64", {"tiling": lib.TILING_BM64, "base.cout_pad": 64}, {}, "cout_pad"),
    ],
    "magnet_conv_mfma_f16": [
        NULL_ARGS, *[(n, s, {}, w) for n, s, w in PLANES], ("act LeakyReLU", LEAKY, {}, "act"), ("tiling BM64", {"tiling": lib.TILING_BM64}, {}, "tiling"),
        ("taps 1", {"base.taps": 1}, {}, "taps"), ("dil 2", {"base.dil": 2}, {}, "dil"), ("cout_pad 256", {"base.cout_pad": 256}, {}, "cout_pad"),
        ("add_hi", {"base.add_hi": P}, {}, "residual"), ("add_lo", {"base.add_lo": P}, {}, "residual"), ("border_hp", {"base.border_hp": 30}, {}, "border"),
        ("repad", {"base.repad": 1}, {}, "repad"), ("plain with out_mode 0", {"base.out_mode": 0, "base.out_hi": P, "base.out_lo": P}, {}, "out_mode"),
        ("tail of 128 outputs", {**TAIL, "base.tail_cout_pad": 128}, {}, "tail"),
    ],
    "magnet_conv_mfma_f16p": [
        NULL_ARGS, *[(n, s, {}, w) for n, s, w in PLANES], ("add_lo", {"base.add_lo": P}, {}, "add_lo"), ("act LeakyReLU", LEAKY, {}, "act"),
        ("tiling BM256", {"tiling": lib.TILING_BM256}, {}, "tiling"), *[(n, s, {}, w) for n, s, w in FUSED], ("cout_pad 256", {"base.cout_pad": 256}, {}, "cout_pad"),
        ("cout_pad 16", {"base.cout_pad": 16}, {}, "cout_pad"),
    ],
    "magnet_conv_mfma_splitk_workspace": [NULL_ARGS, *SPLITK_FORM],
    "magnet_conv_mfma_splitk": [NULL_ARGS, *SPLITK_FORM, *SPLITK_CALL],
    "magnet_conv_mfma_f16d": [NULL_ARGS, *F16D_FORM],
}
# the fp16 split-K form: conv_f16d_check first, then what is left of the split-K checks (the activation is checked by the former)
_LEFT = [c for c in SPLITK_FORM if c[0] not in {f[0] for f in F16D_FORM}]
OWN["magnet_conv_mfma_f16d_splitk_workspace"] = [NULL_ARGS, *F16D_FORM, *_LEFT]
OWN["magnet_conv_mfma_f16d_splitk"] = [NULL_ARGS, *F16D_FORM, *_LEFT, *[c for c in SPLITK_CALL if c[0].startswith("work")]]
# two violations whose codes differ: the first check in the entry point's order answers
TWO = [
    ("magnet_conv_mfma", "two: in_hi NULL, out_mode 5", {"base.in_hi": None, "base.out_mode": 5}, {}, "NULL input"),
    ("magnet_conv_mfma", "two: out_mode 5, in_hi misaligned", {"base.out_mode": 5, "base.in_hi": 24}, {}, "out_mode"),
    ("magnet_conv_mfma", "two: rows 0, w_hi misaligned", {"base.rows": 0, "base.w_hi": 24}, {}, "rows"),
    ("magnet_conv_mfma", "two: in_hi misaligned, dil 9", {"base.in_hi": 24, "base.dil": 9}, {}, "aligned"),
    ("magnet_conv_mfma", "two: out_f32 NULL, cin 16", {"base.out_f32": None, "base.cin": 16}, {}, "NULL output"),
    ("magnet_conv_mfma", "two: addend misaligned, in_ld 100", {"base.addend": 24, "base.in_ld": 100}, {}, "addend"),
    ("magnet_conv_mfma_ex", "two: act 7, in_hi NULL", {"act": 7, "base.in_hi": None}, {}, "act"),
    ("magnet_conv_mfma_ex", "two: tiling 8, bias misaligned", {"tiling": 8, "base.bias": 24}, {}, "tiling"),
    ("magnet_conv_mfma_f16", "two: in_lo, in_hi NULL", {"base.in_lo": P, "base.in_hi": None}, {}, "in_lo"),
    ("magnet_conv_mfma_f16p", "two: cout_pad 256, w_hi misaligned", {"base.cout_pad": 256, "base.w_hi": 24}, {}, "cout_pad"),
    ("magnet_conv_mfma_splitk", "two: work NULL, tiling BM256", {"tiling": lib.TILING_BM256}, {"work": None}, "tiling"),
    ("magnet_conv_mfma_splitk", "two: work misaligned, act 7", {"act": 7}, {"work": 24}, "work"),
    ("magnet_conv_mfma_splitk", "two: work misaligned, in_hi NULL", {"base.in_hi": None}, {"work": 24}, "work"),
    ("magnet_conv_mfma_splitk", "two: work_bytes short, w_hi misaligned", {"base.w_hi": 24}, {"work_bytes": 8}, "work_bytes"),
    ("magnet_conv_mfma_f16d", "two: bias NULL, cout_pad 64", {"base.bias": None, "base.cout_pad": 64}, {}, "cout_pad"),
    ("magnet_conv_mfma_f16d_splitk", "two: in_lo, split_k 1", {"base.in_lo": P}, {"split_k": 1}, "in_lo"),
    ("magnet_conv_mfma_f16d_splitk", "two: work NULL, out_mode 2", {"base.out_mode": 2, "base.out_hi": P}, {"work": None}, "out_mode"),
]


def replay(L, entry, overrides, call):
    """Call `entry` of the loaded library L with the base set of BASES, `overrides` on its fields and `call` on its other arguments.
    Returns (answer, magnet_last_error() as str)."""
    x = lib.MagnetConvExArgs()
    c = x.base
    c.in_hi = c.in_lo = c.w_hi = c.w_lo = c.bias = c.out_hi = c.out_lo = c.out_f32 = P
    c.rows, c.cin, c.cout_pad, c.taps, c.wp, c.out_mode = 510, 160, 256, 9, 17, 1
    for path, v in {**BASES[entry][0], **overrides}.items():
        obj, name = (x.base, path[5:]) if path.startswith("base.") else (x, path)
        setattr(obj, name, v)
    args = {**BASES[entry][1], **call}
    struct = None if "args" in args else ctypes.byref(x.base if entry == "magnet_conv_mfma" else x)
    f = getattr(L, entry)
    if entry.endswith("_workspace"):
        rc = f(struct, args["split_k"])
    elif "split_k" in args:
        rc = f(struct, args["split_k"], args["work"], args["work_bytes"], None)
    else:
        rc = f(struct, None)
    return int(rc), L.magnet_last_error().decode("utf-8", "replace")


def main(library, out):
    lib.LIB_PATH = os.path.abspath(library)                            # before the first load(): the library to record, not this tree's
    L = lib.load()
    assert L._name == lib.LIB_PATH, (L._name, lib.LIB_PATH)
    assert L.magnet_device_count() == 0, "run this on a machine without a GPU: the base argument sets hold fake pointers"
    cases = []

    def record(entry, name, overrides, call, word, common):
        rc, msg = replay(L, entry, overrides, call)
        code = -rc if entry.endswith("_workspace") else rc
        from_run = entry == "magnet_conv_mfma" or msg.startswith("magnet_conv_mfma:") or ": out_mode must be " in msg      # conv_mfma_run's messages
        if common and not (code > 0 and from_run):
            return                                                     # the entry point's own check came first, or this is no violation on its route
        assert 0 < code <= lib.E_SHAPE, f"{entry} / {name}: answered {rc} ({msg!r}): not a refusal"
        who = entry[:-len("_workspace")] if entry.endswith("_workspace") else entry       # a query speaks under its launch's name
        assert from_run or msg.startswith(who + ":"), (entry, name, msg)
        word = None if from_run else word                              # the whole message is pinned
        assert from_run or word in msg, (entry, name, word, msg)
        cases.append({"entry": entry, "name": name, "set": overrides, "call": call, "code": code, "message": msg, "exact": bool(from_run), "who": who,
                      "word": word})

    for entry in BASES:                                                # the base sets are valid: accepted (then no device to launch on), and not recorded
        rc, msg = replay(L, entry, {}, {})
        assert rc < 0 or (entry.endswith("_workspace") and rc == 2 * 510 * 256 * 4), f"{entry}: the base set is refused: {rc} {msg!r}"
    for entry, own in OWN.items():
        for name, overrides, call, word in own:
            record(entry, name, overrides, call, word, False)
    for entry in LAUNCHES:
        for name, overrides in COMMON:
            record(entry, name, overrides, {}, None, True)
    for entry, name, overrides, call, word in TWO:
        record(entry, name, overrides, call, word, False)
    ids = [(c["entry"], c["name"]) for c in cases]
    assert len(ids) == len(set(ids))
    with open(out, "w") as f:
        json.dump({"cases": cases}, f, indent=0, sort_keys=True)
        f.write("\n")
    per = {e: sum(c["entry"] == e for c in cases) for e in BASES}
    print(f"{len(cases)} refusals ({sum(c['exact'] for c in cases)} with the message pinned) of {lib.LIB_PATH} -> {out}")
    print(per)


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "conv_refusals.json"))
