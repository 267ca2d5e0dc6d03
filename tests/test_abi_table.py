"""``_native.SIGNATURES`` is the one place a ctypes signature lives, and it equals
include/preganplus.h: names, parameter counts, per-position kinds, return types
and the mirrored structs.  CPU: the library parts load it, no GPU call."""
import ctypes
import os
import re
import types

import pytest

from preganplus_amd import _native
from preganplus_amd._native import SIGNATURES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALARS = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "size_t": ctypes.c_size_t,
           "float": ctypes.c_float, "double": ctypes.c_double}
RETURNS = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "const char*": ctypes.c_char_p}
STRUCT = re.compile(r"typedef\s+struct\s*\w*\s*\{(.*?)\}\s*(\w+)\s*;", re.S)


def c_kind(decl):
    """Kind of a C parameter 'type name': a SCALARS key, 'ptr' or 'fn'."""
    typ = " ".join(decl.replace("const ", " ").split()).rsplit(" ", 1)[0]
    return "ptr" if "*" in decl else "fn" if typ == "pgp_collective_fn" else {k: k for k in SCALARS}[typ]


def ct_kind(t):
    if issubclass(t, ctypes.Array):
        return (ct_kind(t._type_), t._length_)
    if t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer):
        return "ptr"
    return "fn" if issubclass(t, ctypes._CFuncPtr) else {v: k for k, v in SCALARS.items()}[t]


def parse_header():
    """({name: (return type, [parameter kind])}, {struct name: body}), comments and preprocessor lines dropped."""
    with open(os.path.join(ROOT, "include", "preganplus.h")) as f:
        txt = re.sub(r"/\*.*?\*/|//[^\n]*|(?m:^\s*#[^\n]*$)", " ", f.read(), flags=re.S)
    protos = {}
    for ret, name, args in re.findall(r"([\w\s*]+?)\b(pgp_\w+)\s*\(([^()]*)\)\s*;", STRUCT.sub(" ", txt)):
        protos[name] = ("".join(ret.split()).replace("const", "const "),
                        [c_kind(a) for a in args.split(",") if a.strip() != "void"])
    return protos, {name: body for body, name in STRUCT.findall(txt)}


def struct_fields(body):
    """[(field, kind)] of a struct body; 'float *P, *G;' and 'double lr[3];' included."""
    out = []
    for base, rest in re.findall(r"(?:const\s+)?(long long|\w+)\s*([^;]*);", body):
        for d in rest.split(","):
            name, arr = re.match(r"\s*\*?\s*(\w+)\s*(?:\[(\d+)\])?\s*$", d).groups()
            kind = "ptr" if "*" in d else base
            out.append((name, (kind, int(arr)) if arr else kind))
    return out


def table_errors(table, protos):
    """Every disagreement between a signature table and the prototypes, by function and position."""
    errs = [f"{n}: in the header or the table alone" for n in set(protos) ^ set(table)]
    for name in sorted(set(table) & set(protos)):
        (restype, argtypes), (ret, kinds) = table[name], protos[name]
        if RETURNS[ret] is not restype:
            errs.append(f"{name}: returns {ret}, restype {restype.__name__}")
        if len(argtypes) != len(kinds):
            errs.append(f"{name}: {len(kinds)} parameters, {len(argtypes)} argtypes")
        errs += [f"{name}: parameter {i} is {k}, argtype {t.__name__}"
                 for i, (k, t) in enumerate(zip(kinds, argtypes)) if ct_kind(t) != k]
    return errs


PROTOS, STRUCTS = parse_header()


def test_names_and_signatures_match_the_header():
    assert set(PROTOS) == set(SIGNATURES) and len(PROTOS) >= 10   # and the parser found more than nothing
    assert table_errors(SIGNATURES, PROTOS) == []


@pytest.mark.parametrize("cls, c_name", [(_native._AdamTensor, "pgp_adam_tensor"),
                                         (_native._OnlineTensor, "pgp_online_tensor"),
                                         (_native._OnlineDesc, "pgp_online_desc")])
def test_structs_match_the_header(cls, c_name):
    assert [(n, ct_kind(t)) for n, t in cls._fields_] == struct_fields(STRUCTS[c_name])


def test_library_exports_and_carries_the_table():
    L = _native.lib()
    assert L._pgp_missing == ()
    for name, (restype, argtypes) in SIGNATURES.items():
        assert hasattr(L, name), name
        assert list(getattr(L, name).argtypes) == argtypes and getattr(L, name).restype is restype, name


def test_an_older_build_binds_what_it_has():
    gone = ("pgp_encoder_form_info", "pgp_gobi_create_many")
    L = types.SimpleNamespace(**{n: types.SimpleNamespace() for n in SIGNATURES if n not in gone})
    bound = lambda: {n: (getattr(L, n).restype, getattr(L, n).argtypes) for n in SIGNATURES if n not in gone}
    assert _native.bind(L) is L and L._pgp_missing == gone and not any(hasattr(L, n) for n in gone)
    first = bound()
    assert first == {n: SIGNATURES[n] for n in first}
    assert _native.bind(L) is L and L._pgp_missing == gone and bound() == first


def test_signatures_live_in_one_place():
    assign = r"\.(?:argtypes|restype)\s*=(?!=)"
    for top in ("preganplus_amd", "tests", "tools"):
        for d, _, files in os.walk(os.path.join(ROOT, top)):
            for path in (os.path.join(d, f) for f in files if f.endswith(".py") and f != "_native.py"):
                with open(path) as f:
                    src = f.read()
                assert top != "preganplus_amd" or not re.search(assign, src), path
                assert not set(re.findall(r"(pgp_\w+)" + assign, src)) & set(SIGNATURES), path


def test_the_checker_rejects_a_wrong_table():
    a, fwd = SIGNATURES["pgp_adamw_table_many"][1], list(SIGNATURES["pgp_forward1_many"][1])
    assert a[0] is ctypes.c_int and a[2] is ctypes.c_void_p
    fwd.remove(ctypes.c_void_p)
    for name, sig in (("pgp_forward1_many", (ctypes.c_int, fwd)),                              # a pointer dropped
                      ("pgp_adamw_table_many", (ctypes.c_int, [a[2], a[1], a[0]] + a[3:])),    # int and pointer swapped
                      ("pgp_master_len", (ctypes.c_int, SIGNATURES["pgp_master_len"][1]))):    # size_t result as int
        errs = table_errors(dict(SIGNATURES, **{name: sig}), PROTOS)
        assert errs and all(e.startswith(name + ":") for e in errs), (name, errs)
