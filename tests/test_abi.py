"""The C-ABI library loads and exports every symbol include/magnet_hip.h declares; the binding's prototype
table, the ctypes mirrors of all argument structs and its constants agree with the header; argument errors
come back as codes (no compute is launched here — that is what the -m gpu tests do)."""
import ctypes
import functools
import os
import re
import subprocess
import tempfile

import pytest

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADER = os.path.join(REPO, "include", "magnet_hip.h")


def _header():
    """include/magnet_hip.h without its comments."""
    return re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)


def _declarations():
    """{name: (return type, [parameter declarations])} of every `MAGNET_API <ret> magnet_x(<params>);`, in header order."""
    decls = {}
    for ret, name, params in re.findall(r"MAGNET_API\s+([\w\s\*]+?)\b(magnet_\w+)\s*\(([^()]*)\)\s*;", _header()):
        params = " ".join(params.split())
        decls[name] = (" ".join(ret.split()), [] if params == "void" else [p.strip() for p in params.split(",")])
    return decls


def _declared_symbols():
    return sorted(_declarations())


def _struct_fields():
    """{struct: [field names]} of every `typedef struct Magnet* { ... } Magnet*;`, in header order."""
    out = {}
    for name, body in re.findall(r"typedef\s+struct\s+(Magnet\w+)\s*\{(.*?)\}\s*\1\s*;", _header(), flags=re.S):
        out[name] = [f for decl in body.split(";") for f in re.findall(r"(\w+)\s*(?:\[\d+\])?\s*(?:,|$)", decl.strip())]
    return out


STRUCTS = _struct_fields()
# the Python mirror (magnet_amd/lib.py) of every enum value and #define the package uses is "MAGNET_" + its name
CONSTANTS = ("E_NULL", "E_DIM", "E_DTYPE", "E_ALIGN", "E_NODEVICE", "E_SHAPE", "FEAT_F32", "FEAT_BF16", "MAX_CANDIDATES", "NLL_BLOCKS",
             "NLL_MAX_ITER", "BN_BLOCKS", "ACT_BASE", "ACT_LEAKY_RELU", "TILING_FLAT", "TILING_BM256")


@functools.lru_cache(maxsize=None)
def _c_probe():
    """What the C compiler makes of the header, from one gcc run: {struct: (sizeof, [(offsetof, sizeof) per field])} and {macro / enum
    name: value}."""
    prog = '#include "%s"\n#include <stdio.h>\n#include <stddef.h>\nint main(){\n' % HEADER
    for s, fields in STRUCTS.items():
        prog += 'printf("S %s %%zu", sizeof(%s));' % (s, s)
        for f in fields:
            prog += 'printf(" %%zu %%zu", offsetof(%s, %s), sizeof(((%s *)0)->%s));' % (s, f, s, f)
        prog += 'printf("\\n");\n'
    for c in ("HIP_VERSION",) + CONSTANTS:
        prog += 'printf("C MAGNET_%s %%lld\\n", (long long)MAGNET_%s);\n' % (c, c)
    prog += "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c"); exe = os.path.join(d, "t")
        open(c, "w").write(prog)
        subprocess.check_call(["gcc", c, "-o", exe])
        lines = [ln.split() for ln in subprocess.check_output([exe]).decode().splitlines()]
    structs = {ln[1]: (int(ln[2]), list(zip(map(int, ln[3::2]), map(int, ln[4::2])))) for ln in lines if ln[0] == "S"}
    return structs, {ln[1]: int(ln[2]) for ln in lines if ln[0] == "C"}


def test_header_declares_expected_entry_points():
    syms = _declared_symbols()
    assert {"magnet_cost_volume_cw", "magnet_pack_features", "magnet_gaussian_update",
            "magnet_upsample_depth", "magnet_version", "magnet_last_error"} <= set(syms)
    assert len(syms) == len(re.findall(r"^MAGNET_API\b", _header(), flags=re.M)) >= 48      # the parser misses no declaration


def test_library_exports_every_declared_symbol(hip_lib):
    from magnet_amd import lib
    for s in _declared_symbols():
        assert hasattr(hip_lib, s), f"{s} declared in include/magnet_hip.h but not exported"
    assert set(_declared_symbols()) == set(lib.API_SYMBOLS)
    assert hip_lib.magnet_version() == _c_probe()[1]["MAGNET_HIP_VERSION"]


_C_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float,
              "double": ctypes.c_double}


def _ctypes_for(c_decl, L, is_param):
    """The ctypes types that may stand for one C return type or parameter declaration of the header."""
    words = re.sub(r"\bconst\b", " ", c_decl).replace("*", " ").split()
    if is_param:
        assert len(words) == 2, f"unnamed or unparsed parameter {c_decl!r}"
    base, stars = words[0], c_decl.count("*")
    if stars == 0:
        return (_C_SCALARS[base],)
    assert stars == 1, c_decl
    if base.startswith("Magnet"):
        return (ctypes.POINTER(getattr(L, base)),)
    if base == "char" and not is_param:
        return (ctypes.c_char_p,)
    return (ctypes.c_void_p,) + ((ctypes.POINTER(_C_SCALARS[base]),) if base in _C_SCALARS else ())


def _proto_mismatches(table, L):
    """Every way the prototype table {name: (restype, argtypes)} differs from the header's declarations ([] = it matches)."""
    decls = _declarations()
    errs = []
    if list(table) != list(decls):
        errs.append(f"names / order: table only {sorted(set(table) - set(decls))}, header only {sorted(set(decls) - set(table))}")
    for name in set(table) & set(decls):
        (restype, argtypes), (ret, params) = table[name], decls[name]
        if restype not in _ctypes_for(ret, L, False):
            errs.append(f"{name}: restype {restype} for `{ret}`")
        if len(argtypes) != len(params):
            errs.append(f"{name}: {len(argtypes)} argtypes for {len(params)} parameters")
        errs += [f"{name}: argument {i} is {a} for `{p}`" for i, (a, p) in enumerate(zip(argtypes, params))
                 if a not in _ctypes_for(p, L, True)]
    return errs


def test_prototype_table_matches_the_header():
    from magnet_amd import lib as L
    assert len(_declarations()) >= 48
    assert _proto_mismatches(L._PROTOS, L) == []
    assert L.API_SYMBOLS == tuple(_declarations())


def test_prototype_comparison_rejects_wrong_tables():
    """Negative control of _proto_mismatches: an int64_t typed 32 bits wide, a dropped parameter, another struct's pointer, a missing
    entry."""
    from magnet_amd import lib as L

    def changed(name, edit):
        table = dict(L._PROTOS)
        restype, argtypes = table[name]
        table[name] = (restype, edit(list(argtypes)))
        return table

    def narrow(argtypes):
        argtypes[argtypes.index(ctypes.c_int64)] = ctypes.c_int32
        return argtypes

    for name in ("magnet_pack_split", "magnet_pack_f16", "magnet_cost_volume_f_backward_ws"):
        errs = _proto_mismatches(changed(name, narrow), L)
        assert len(errs) == 1 and name in errs[0] and "int64_t" in errs[0], errs
    errs = _proto_mismatches(changed("magnet_upsample_depth", lambda a: a[:-1]), L)
    assert len(errs) == 1 and "8 argtypes for 9" in errs[0], errs
    errs = _proto_mismatches(changed("magnet_wgrad", lambda a: [ctypes.POINTER(L.MagnetWgradExArgs)] + a[1:]), L)
    assert len(errs) == 1 and "magnet_wgrad: argument 0" in errs[0], errs
    errs = _proto_mismatches(changed("magnet_conv_mfma", lambda a: [ctypes.c_void_p] + a[1:]), L)
    assert len(errs) == 1 and "magnet_conv_mfma: argument 0" in errs[0], errs               # a struct pointer is not "any pointer"
    table = dict(L._PROTOS)
    table["magnet_wgrad_workspace"] = (ctypes.c_int, table["magnet_wgrad_workspace"][1])
    assert len(_proto_mismatches(table, L)) == 1                                             # int64_t return read as int
    del table["magnet_wgrad_workspace"]
    assert any("header only ['magnet_wgrad_workspace']" in e for e in _proto_mismatches(table, L))


def test_every_entry_point_is_typed_after_load(hip_lib):
    """No function reached through load() is left with ctypes' default of 32-bit int arguments."""
    from magnet_amd import lib as L
    assert len(L.API_SYMBOLS) == len(set(L.API_SYMBOLS)) >= 48
    for name in L.API_SYMBOLS:
        f = getattr(hip_lib, name)
        restype, argtypes = L._PROTOS[name]
        assert f.argtypes is not None and list(f.argtypes) == argtypes, name
        assert f.restype is restype, name


def test_every_header_struct_has_a_mirror():
    from magnet_amd import lib as L
    mirrors = {n for n, v in vars(L).items() if isinstance(v, type) and issubclass(v, ctypes.Structure) and v is not ctypes.Structure}
    assert mirrors == set(STRUCTS) and len(STRUCTS) >= 11


@pytest.mark.parametrize("struct", list(STRUCTS))
def test_struct_layout_matches_c(hip_lib, struct):
    from magnet_amd import lib as L
    A = getattr(L, struct)
    fields = [f[0] for f in A._fields_]
    assert fields == STRUCTS[struct]                          # the header's fields, all of them, in its order
    size, layout = _c_probe()[0][struct]
    assert size == ctypes.sizeof(A)
    assert layout == [(getattr(A, f).offset, getattr(A, f).size) for f in fields]


def test_constants_match_the_header():
    from magnet_amd import lib as L
    values = _c_probe()[1]
    for name in CONSTANTS:
        assert getattr(L, name) == values["MAGNET_" + name], name


def test_argument_errors_are_codes_not_crashes(hip_lib):
    from magnet_amd.lib import MagnetCostVolumeArgs
    assert hip_lib.magnet_cost_volume_cw(None, None) == 1                       # MAGNET_E_NULL
    assert b"NULL" in hip_lib.magnet_last_error()
    a = MagnetCostVolumeArgs()                                                  # all zero
    assert hip_lib.magnet_cost_volume_cw(ctypes.byref(a), None) == 1
    assert hip_lib.magnet_pack_features(None, None, 1, 8, 4, 4, 0, 0, None) == 1
    assert hip_lib.magnet_pack_features(16, 16, 1, 7, 4, 4, 0, 0, None) == 2       # MAGNET_E_DIM (F % 8)
    assert hip_lib.magnet_pack_features(16, 16, 1, 8, 4, 4, 9, 0, None) == 3       # MAGNET_E_DTYPE
    assert hip_lib.magnet_pack_features(16, 24, 1, 8, 4, 4, 0, 0, None) == 4
    assert hip_lib.magnet_pack_features(16, 16, 1, 8, 4, 4, 0, 2, None) == 2       # pad in {0,1}
    assert hip_lib.magnet_pack_gmm(None, 16, 1, 4, 4, None) == 1       # MAGNET_E_ALIGN
    assert hip_lib.magnet_gaussian_update(16, 16, 16, 0, 5, None) == 2
    assert hip_lib.magnet_upsample_depth(16, 16, 16, 1, 2, 4, 4, 3, None) == 2  # k must be 1,2,4,8
    # convolution / F-Net entry points
    from magnet_amd.lib import MagnetConvArgs
    c = MagnetConvArgs()
    assert hip_lib.magnet_conv_mfma(ctypes.byref(c), None) == 1
    c.in_hi = c.in_lo = c.w_hi = c.w_lo = c.bias = c.out_hi = c.out_lo = 16
    c.rows, c.cin, c.cout_pad, c.taps, c.wp = 128, 48, 128, 9, 10
    assert hip_lib.magnet_conv_mfma(ctypes.byref(c), None) == 2                 # cin % 32
    c.cin = 64; c.cout_pad = 48
    assert hip_lib.magnet_conv_mfma(ctypes.byref(c), None) == 2                 # unsupported width
    c.cout_pad = 64; c.taps = 5
    assert hip_lib.magnet_conv_mfma(ctypes.byref(c), None) == 2                 # taps in {1,4,9}
    c.taps = 9; c.repad = 1
    assert hip_lib.magnet_conv_mfma(ctypes.byref(c), None) == 2 and b"repad" in hip_lib.magnet_last_error()
    c.repad = 0; c.border_hp, c.border_pad = 7, 1                               # 128 rows are not a whole number of 7x10 grids
    assert hip_lib.magnet_conv_mfma(ctypes.byref(c), None) == 2
    c.border_hp = 0; c.tail_w_hi = 16
    assert hip_lib.magnet_conv_mfma(ctypes.byref(c), None) == 1                 # fused tail without its other pointers
    assert hip_lib.magnet_fnet_stem(None, 16, 16, 16, 16, 1, 8, 8, None) == 1
    assert hip_lib.magnet_fnet_stem(16, 16, 16, 16, 16, 1, 1, 8, None) == 2
    assert hip_lib.magnet_space_to_depth(16, 16, 16, 16, 1, 12, 4, 4, 2, None) == 2     # C % 8
    assert hip_lib.magnet_avgpool_cl(16, 16, 320, 1, 8, 8, 2, 16, 128, 16, 16, None) == 2   # window larger than the map
    assert hip_lib.magnet_upsample_bilinear_cl(16, 32, 1, 2, 32, 16, 24, 320, 1, 8, 8, 2, None) == 4   # out_lo misaligned
    assert hip_lib.magnet_cost_volume_f_backward(None, 16, 16, 16, None) == 1
    # D over the limit
    a.ref_feat_cl = a.src_feat_pad = a.src_gmm_pad = a.poses = a.is_valid = a.intM = a.rays = a.cost = 16
    a.d_volume = 16
    a.B = a.V = a.h = a.w = 1; a.F = 8; a.D = 257
    assert hip_lib.magnet_cost_volume_cw(ctypes.byref(a), None) == 2
    assert b"MAGNET_MAX_CANDIDATES" in hip_lib.magnet_last_error()


def test_product_path_never_imports_the_oracle():
    """The oracle is test infrastructure: nothing under magnet_amd/ may import, load or link it."""
    pkg = os.path.join(REPO, "magnet_amd")
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".cpp", ".h")):
                txt = open(os.path.join(root, f)).read()
                for needle in ("libmagnet_oracle", "import oracle", "from oracle", "oracle.oracle",
                               "magnet_oracle_", "cost_volume_oracle.h"):
                    assert needle not in txt, f"{f} references the oracle ({needle})"


def test_host_raises_without_gpu_tensors(hip_lib):
    import torch
    from magnet_amd import lib
    x = torch.zeros(1, 8, 4, 4)
    with pytest.raises(lib.MagnetError, match="no CPU fallback"):
        lib.pack_features(x)
    with pytest.raises(lib.MagnetError, match="no CPU fallback"):
        lib.gaussian_update(torch.zeros(1, 2, 4, 4), torch.zeros(1, 2, 4, 4))


def test_graft_entry_version_check_follows_the_header():
    """__graft_entry__.build() compares the built library with include/magnet_hip.h, not with a literal that goes stale on an ABI bump
    (round 4: the literal said 301 while the header said 302 — the driver's build check would have failed)."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "__graft_entry__.py")).read()
    assert "MAGNET_HIP_VERSION" in src and not re.search(r"magnet_version\(\)\s*==\s*\d", src)
